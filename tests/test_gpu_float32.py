"""Float32 and Int32 expression matrices on the GPU: reo_set_matrix_f32 / _i32 and their device forms.

Float32 is compared in Float32 arithmetic, as the reference's is_greater compares a Matrix{Float32} (src/RankCompV3.jl:71-77): the
yardstick is the numpy restatement float32_cases.f32_pair_counts, and on the planted cases (float32_cases.planted) it differs from
the Float64 oracle on the widened values.  Int32 has Int64's semantics and must reproduce the Int64 path bit for bit."""
import numpy as np
import pytest

import float32_cases as fc

pytestmark = pytest.mark.gpu

P_ATOL = 1e-6      # the tolerances of test_gpu_parity.py
STAT_RTOL = 1e-7


def _check_result(res, exp):
    assert np.array_equal(res[:, 2:11], exp[:, 2:11]), "tallies differ"
    assert np.allclose(res[:, :2], exp[:, :2], rtol=0, atol=P_ATOL), np.abs(res[:, :2] - exp[:, :2]).max()
    assert np.allclose(res[:, 11:], exp[:, 11:], rtol=STAT_RTOL, atol=1e-9), np.abs(res[:, 11:] - exp[:, 11:]).max()


def _device_copy(X, pad=0):
    """A column-major copy of X in HBM with leading dimension G + pad: (tensor to keep alive, pointer, ld)."""
    import torch
    G, S = X.shape
    t = torch.zeros((S, G + pad), dtype=torch.from_numpy(X[:1, :1].copy()).dtype, device="cuda:0")
    t[:, :G] = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda:0")
    torch.cuda.synchronize()
    return t, t.data_ptr(), G + pad


def _load(pkg, ctx, X, gid, ngroups, how):
    """how: matrix_first | groups_first (the pipelined upload) | device (a resident matrix with a leading dimension)."""
    keep = None
    if how == "matrix_first":
        ctx.set_matrix(X); ctx.set_groups(gid, ngroups); ctx.compute_thresholds(0.01)
    elif how == "groups_first":
        ctx.set_groups(gid, ngroups); ctx.compute_thresholds(0.01); ctx.set_matrix(X)
    else:
        keep, ptr, ld = _device_copy(X, pad=8)
        name = {np.dtype(np.float32): "f32", np.dtype(np.int32): "i32", np.dtype(np.float64): "f64", np.dtype(np.int64): "i64"}[X.dtype]
        ctx.set_matrix_device(ptr, X.shape[0], X.shape[1], ld, name, keepalive=keep)
        ctx.set_groups(gid, ngroups); ctx.compute_thresholds(0.01)
    return keep


@pytest.mark.parametrize("how", ["matrix_first", "groups_first", "device"])
def test_float32_is_compared_in_float32_arithmetic(pkg, oracle, how):
    G, S, seed = 256, 64, 0x5EED0F32
    X = fc.planted(G, S, 24, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    egt, eeq = fc.f32_pair_counts(X, gid, 2)
    ogt, oeq = oracle.pair_counts(X.astype(np.float64), gid, 2, 0, G, 0, G)
    with pkg.Context(device=0, seed=seed) as ctx:
        _load(pkg, ctx, X, gid, 2, how)
        gt, eq = ctx.pair_counts(0, G, 0, G)
        info = ctx.info()
    off = ~np.eye(G, dtype=bool)   # (the diagonal is never evaluated; the library reports it tied)
    print(f"{how}: entries that differ from the Float32 restatement: gt {(gt != egt)[off].sum()} eq {(eq != eeq)[off].sum()}; "
          f"from the Float64 oracle: gt {(gt != ogt)[off].sum()} eq {(eq != oeq)[off].sum()}")
    assert np.array_equal(gt[off], egt[off].astype(np.uint16)) and np.array_equal(eq[off], eeq[off].astype(np.uint16))
    assert not np.array_equal(eq[off], oeq[off]) and not np.array_equal(gt[off], ogt[off])
    assert info["transform_in_lds"] == 2 and info["has_ties"] == 1


@pytest.mark.parametrize("ngroups", [2, 3])
def test_float32_whole_run_against_the_float32_restatement(pkg, oracle, ngroups):
    """Codes, tallies, trace and statistics of every comparison: the codes assembled here from f32_pair_counts, the oracle's tie coins
    and the rule of :376-377,385-386; tallies and the loop from the oracle."""
    G, S, seed = 300, 40, 0x5EED0F33 + ngroups
    X = fc.planted(G, S, 20, seed)
    gid = (np.arange(S) * ngroups // S).astype(np.int32)
    sizes = np.bincount(gid, minlength=ngroups)
    ref0 = pkg.synth.ref_mask(G, 90, seed)
    differs = 0
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, ngroups); thr_all = ctx.compute_thresholds(0.01); ctx.set_matrix(X)
        for k in range(1 if ngroups == 2 else ngroups):
            thr = [oracle.threshold(int(sizes[k])), oracle.threshold(int(S - sizes[k]))]
            assert thr_all[:, k].tolist() == thr
            code = fc.f32_build_codes(X, gid, ngroups, k, thr, seed, oracle.tie_wins)
            differs += int((code != oracle.build_codes(X.astype(np.float64), gid, ngroups, k, thr, seed)).sum())
            ctx.build_pairs(k)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), code), k
            assert np.array_equal(ctx.tally(ref0), oracle.tally(code, ref0)), k
            exp, iters, trace = oracle.iterate(code, ref0, 1.0, 0.05, 6, 1)
            res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 6, 1)
            assert it == iters and tr == trace, k
            _check_result(res, exp)
    print(f"class codes that differ from the Float64 oracle's: {differs}")


def _sample_blocks(G, rng, n=3):
    blocks = [(0, 24, 0, 48), (G - 24, G, G - 48, G), (G - 24, G, 0, 48)]
    for _ in range(n):
        i0 = int(rng.integers(0, G - 24)); j0 = int(rng.integers(0, G - 48))
        blocks.append((i0, i0 + 24, j0, j0 + 48))
    return blocks


@pytest.mark.parametrize("G", [9000, 21000, 30000, 61000, 70000])
def test_float32_in_every_form_of_the_ranking(pkg, G):
    """t_sample_wide <4, true> / <3, true> / <4, false> / <3, false> and t_sample_big on values whose differences are exact in both
    arithmetics: same positions and bands as the Float64 path on the widened values, hence the same everything."""
    S, seed = 64, 0x5EED0F40 + G
    X = fc.exact_grid(G, S, seed, n_inf=40)
    X[G - 1, :5] = np.inf; X[0, :5] = -np.inf                # the first and the last gene: the ends of the code ranges
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, G // 5, seed)
    blocks = _sample_blocks(G, np.random.default_rng(G))
    out = {}
    for name, M in (("f32", X), ("f64", X.astype(np.float64))):
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_matrix(M); ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            counts = [ctx.pair_counts(*b) for b in blocks]
            ctx.build_pairs(0)
            res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 3, 1)
            out[name] = (counts, res, it, tr, ctx.info())
    (c32, r32, it32, tr32, i32), (c64, r64, it64, tr64, i64) = out["f32"], out["f64"]
    assert i32["transform_in_lds"] == i64["transform_in_lds"] == (2 if G <= 65535 else 3)
    assert i32["has_ties"] == i64["has_ties"] == 1
    for b, (g32, e32), (g64, e64) in zip(blocks, c32, c64):
        assert np.array_equal(g32, g64) and np.array_equal(e32, e64), (G, b)
    assert it32 == it64 and tr32 == tr64
    assert np.array_equal(r32, r64, equal_nan=True)


def test_float32_with_18_bit_positions(pkg):
    """131 584 genes (18 planes), 8 samples: sampled blocks only."""
    G, S, seed = 131584, 8, 0x5EED0F48
    X = fc.exact_grid(G, S, seed, n_inf=16)
    gid = (np.arange(S) % 2).astype(np.int32)
    blocks = _sample_blocks(G, np.random.default_rng(7), n=5)
    out = {}
    for name, M in (("f32", X), ("f64", X.astype(np.float64))):
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_matrix(M); ctx.set_groups(gid, 2)
            out[name] = ([ctx.pair_counts(*b) for b in blocks], ctx.info())
    assert out["f32"][1]["transform_in_lds"] == out["f64"][1]["transform_in_lds"] == 3
    for b, (g32, e32), (g64, e64) in zip(blocks, out["f32"][0], out["f64"][0]):
        assert np.array_equal(g32, g64) and np.array_equal(e32, e64), b


def test_float32_nan_is_refused(pkg):
    G, S = 400, 12
    X = fc.exact_grid(G, S, 3)
    X[17, 5] = np.nan
    gid = (np.arange(S) % 2).astype(np.int32)
    for how in ("matrix_first", "groups_first", "device"):
        with pkg.Context(device=0, seed=1) as ctx:
            with pytest.raises(pkg.DimensionMismatch) as e:
                _load(pkg, ctx, X, gid, 2, how)
                ctx.pair_counts(0, 8, 0, 8)
            assert "expression matrix contains NaN" in str(e.value) and "+-Inf are accepted" in str(e.value), how


@pytest.mark.parametrize("kind", ["log0", "column", "group", "rows"])
def test_float32_infinities_as_the_float64_path(pkg, kind):
    """The layouts of test_infinities_are_compared_as_the_reference_compares_them on values whose differences are exact: counts,
    class table, tallies and the run of the Float32 path equal those of the Float64 path, in both orders of calls."""
    G, S, seed = 500, 24, 0x5EED0F62
    X64 = pkg.synth.with_infinities(fc.exact_grid(G, S, seed, n_inf=0).astype(np.float64), seed, kind)
    X = X64.astype(np.float32)
    assert np.array_equal(X.astype(np.float64), X64) and np.isinf(X).sum() > G
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 150, seed)
    out = {}
    for name, M in (("f64", X64), ("f32", X)):
        for how in ("matrix_first", "groups_first"):
            with pkg.Context(device=0, seed=seed) as ctx:
                _load(pkg, ctx, M, gid, 2, how)
                cnt = ctx.pair_counts(0, G, 0, G)
                ctx.build_pairs(0)
                assert ctx.info()["transform_in_lds"] == 2
                code = ctx.get_codes(0, G, 0, G)
                tal = ctx.tally(ref0)
                res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
                out[name, how] = (cnt, code, tal, res, it, tr)
    ref = out["f64", "matrix_first"]
    for key, got in out.items():
        assert np.array_equal(got[0][0], ref[0][0]) and np.array_equal(got[0][1], ref[0][1]), key
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), key
        assert got[4] == ref[4] and got[5] == ref[5] and np.array_equal(got[3], ref[3], equal_nan=True), key


@pytest.mark.parametrize("family", ["t1", "t0", "extremes"])
def test_int32_equals_int64(pkg, family):
    G, S, seed = 2600, 72, 0x5EED0F70
    if family == "t1":
        X64 = pkg.synth.t1_counts(G, S, seed)
    elif family == "t0":
        X64 = pkg.synth.t0_ranks(G, S, seed)
    else:
        rng = np.random.default_rng(seed)
        X64 = rng.integers(-(1 << 31), 1 << 31, size=(G, S), dtype=np.int64)
        X64[:, 3] = pkg.synth.t1_counts(G, S, seed)[:, 3]
        X64[5, 3] = -(1 << 31); X64[G - 9, 3] = (1 << 31) - 1        # a column holding INT32_MIN and INT32_MAX
        X64[:40, 7] = (1 << 31) - 1; X64[40:80, 7] = -(1 << 31)
    X32 = X64.astype(np.int32)
    assert np.array_equal(X32.astype(np.int64), X64)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 600, seed)
    blocks = _sample_blocks(G, np.random.default_rng(3)) + [(0, 90, 0, 90)]
    out = {}
    for name, M, hows in (("i64", X64, ("matrix_first",)), ("i32", X32, ("matrix_first", "groups_first", "device"))):
        for how in hows:
            with pkg.Context(device=0, seed=seed) as ctx:
                _load(pkg, ctx, np.asfortranarray(M), gid, 2, how)
                cnt = [ctx.pair_counts(*b) for b in blocks]
                ctx.build_pairs(0)
                code = ctx.get_codes(0, G, 0, G)
                res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 6, 1)
                info = ctx.info()
                if name == "i32" and how != "device":
                    assert info["upload_link_bytes"] == 4 * G * S
                out[name, how] = (cnt, code, res, it, tr, info["transform_in_lds"], info["has_ties"])
    ref = out["i64", "matrix_first"]
    for key, got in out.items():
        for (g, e), (rg, re_) in zip(got[0], ref[0]):
            assert np.array_equal(g, rg) and np.array_equal(e, re_), key
        assert np.array_equal(got[1], ref[1]), key
        assert got[3] == ref[3] and got[4] == ref[4] and np.array_equal(got[2], ref[2], equal_nan=True), key
        assert got[5:] == ref[5:], key


def test_float32_crosses_the_link_as_it_is(pkg):
    G, S, seed = 3000, 200, 0x5EED0F80
    X = np.asfortranarray(pkg.synth.float_expr(G, S, seed).astype(np.float32))
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    for how in ("matrix_first", "groups_first"):
        with pkg.Context(device=0, seed=seed) as ctx:
            _load(pkg, ctx, X, gid, 2, how)
            ctx.build_pairs(0)
            info = ctx.info()
        print(f"{how}: {info['upload_link_bytes']} bytes on the link for {G} x {S} float32 ({4 * G * S} = 4 G S)")
        assert 0 < info["upload_link_bytes"] <= 4 * G * S


def _same_res(a, b):
    assert a.shape == b.shape
    assert list(a[:, 0]) == list(b[:, 0])
    for q in range((a.shape[1] - 1) // 16):
        assert np.array_equal(a[:, 1 + 16 * q: 16 + 16 * q].astype(np.float64), b[:, 1 + 16 * q: 16 + 16 * q].astype(np.float64), equal_nan=True)
        assert list(a[:, 16 + 16 * q]) == list(b[:, 16 + 16 * q])


@pytest.mark.parametrize("kind", ["f32", "i32", "f16"])
def test_torch_device_tensor_as_data(pkg, kind):
    """identify_degs with a torch tensor on the GPU: column-major (used in place, with a leading dimension) and row-major (made
    column-major on the device) give the `res` of the numpy call on the same values; float16 is cast on the device."""
    import torch
    G, S, seed = 1200, 48, 0x5EED0F90
    if kind == "i32":
        X = pkg.synth.t1_counts(G, S, seed).astype(np.int32)
    elif kind == "f32":
        X = fc.planted(G, S, 30, seed)
    else:
        X = fc.exact_grid(G, S, seed).astype(np.float16)
    group = pkg.synth.groups(S)
    names = [f"g{i}" for i in range(G)]
    ref0 = pkg.synth.ref_mask(G, 300, seed)
    exp = pkg.identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
    row_major = torch.from_numpy(np.ascontiguousarray(X)).to("cuda:0")
    assert row_major.stride() == (S, 1)
    tall = torch.zeros((S, G + 16), dtype=row_major.dtype, device="cuda:0")
    tall[:, :G] = row_major.t()
    col_major = tall[:, :G].t()
    assert col_major.stride() == (1, G + 16) and torch.equal(col_major, row_major)
    for t in (col_major, row_major):
        ptr, g, s, ld, dtype, keep = pkg._ffi.device_matrix(t)
        assert (g, s) == (G, S) and dtype == {"f32": "f32", "i32": "i32", "f16": "f64"}[kind]
        if t is col_major and kind != "f16":
            assert ptr == t.data_ptr() and ld == G + 16      # used in place
        else:
            assert ld == G and keep.stride() == (1, G)
        got = pkg.identify_degs(t, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        _same_res(got, exp)

@pytest.mark.parametrize("source", ["host", "device"])
def test_float32_in_two_shards_on_one_device(pkg, monkeypatch, source):
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    G, S, seed = 3300, 72, 0x5EED0FA0
    X = fc.planted(G, S, 40, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 700, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        code0 = ctx.get_codes(0, G, 0, G)
        res0, it0, tr0 = ctx.identify_degs(ref0, 1.0, 0.05, 6, 1)
    with pkg.Context(seed=seed, n_gpus=2) as ctx:
        if source == "host":
            ctx.set_matrix(X)
        else:
            keep, ptr, ld = _device_copy(X, pad=24)
            ctx.set_matrix_device(ptr, G, S, ld, "f32", keepalive=keep)
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["tiles_owned"] < info["tiles_total"]
        assert np.array_equal(ctx.get_codes(0, G, 0, G), code0)
        res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 6, 1)
        assert it == it0 and tr == tr0 and np.array_equal(res, res0, equal_nan=True)


def test_int32_device_matrix_in_two_shards_on_one_device(pkg, monkeypatch):
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    G, S, seed = 3300, 72, 0x5EED0FA1
    X64 = pkg.synth.t1_counts(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X64); ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        code0 = ctx.get_codes(0, G, 0, G)
    keep, ptr, ld = _device_copy(X64.astype(np.int32), pad=24)
    for source in ("host", "device"):
        with pkg.Context(seed=seed, n_gpus=2) as ctx:
            if source == "host":
                ctx.set_matrix(X64.astype(np.int32))
            else:
                ctx.set_matrix_device(ptr, G, S, ld, "i32", keepalive=keep)
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            ctx.build_pairs(0)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), code0), source
