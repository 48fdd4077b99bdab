"""Row-major host matrices on the GPU (reo_set_matrix_rm_*): read in place, transposed on the device by t_widen_transpose.  The yardstick
in every case is the column-major entry on np.asfortranarray(X) in the same process and under the same settings (that path is pinned
against the oracle by test_gpu_parity.py / test_gpu_float32.py): class table, tallies, identify_degs, has_ties and the bytes on the
link must be equal bit for bit.  Every row-major run asserts info()["rowmajor_upload"] == 1 (or calls the _rm_ symbol itself), so none of
this passes by quietly taking the old route."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P_ATOL = 1e-6      # the tolerances of test_gpu_parity.py (oracle comparison only; everything else is bit-equality)
STAT_RTOL = 1e-7
ENV = ("REO_EAGER_UPLOAD", "REO_UPLOAD_THREADS", "REO_EAGER_CHUNK", "REO_EAGER_RANGES", "REO_ROWMAJOR", "REO_ROWMAJOR_COPY")


def _setenv(monkeypatch, **kw):
    for name in ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("REO_ROWMAJOR", "1")   # the route under test (the mirror takes it only when asked to)
    for name, val in kw.items():
        if val is not None:
            monkeypatch.setenv(name, str(val))


def _padded(X, pad, at=3):
    """X as a column slice of a wider C-ordered array: ld = S + pad, the rest filled with a value that would change every result"""
    if pad == 0:
        return np.ascontiguousarray(X)
    G, S = X.shape
    wide = np.full((G, S + pad), 77, dtype=X.dtype)
    wide[:, at:at + S] = X
    return wide[:, at:at + S]


def _run(pkg, X, group, seed, order, rowmajor, ref0=None, degs=True, n_gpus=None):
    """codes, tally, identify_degs, has_ties, link bytes of one context; rowmajor: X must take the new route (else the old one)"""
    gid, lev = pkg.encode_groups(group)
    G = X.shape[0]
    kw = dict(seed=seed, n_gpus=n_gpus) if n_gpus else dict(device=0, seed=seed)
    with pkg.Context(**kw) as ctx:
        if order == "matrix_first":
            ctx.set_matrix(X)
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01)
        if order != "matrix_first":
            ctx.set_matrix(X)
        info = ctx.info()
        assert info["rowmajor_upload"] == (1 if rowmajor else 0), (order, info["rowmajor_upload"])
        out = dict(link=info["upload_link_bytes"], ranges=info["eager_range_launches"], per_k=[])
        for k in range(1 if len(lev) == 2 else len(lev)):
            ctx.build_pairs(k)
            codes = ctx.get_codes(0, G, 0, G)
            tal = ctx.tally(ref0) if ref0 is not None else None
            deg = ctx.identify_degs(ref0, 1.0, 0.05, 6, 0) if (degs and ref0 is not None) else None
            out["per_k"].append((codes, tal, deg, ctx.info()["has_ties"]))
    return out


def _same(a, b, what):
    assert a["link"] == b["link"], (what, "link bytes", a["link"], b["link"])
    assert len(a["per_k"]) == len(b["per_k"])
    for (c0, t0, d0, h0), (c1, t1, d1, h1) in zip(a["per_k"], b["per_k"]):
        assert np.array_equal(c0, c1), (what, "class table")
        assert h0 == h1, (what, "has_ties")
        if t0 is not None:
            assert np.array_equal(t0, t1), (what, "tallies")
        if d0 is not None:
            assert d0[1] == d1[1] and d0[2] == d1[2], (what, "iterations / trace")
            assert np.array_equal(d0[0], d1[0], equal_nan=True), (what, "statistics")


def _data(pkg, kind, G, S, seed):
    if kind == "i64": return pkg.synth.t1_counts(G, S, seed)
    if kind == "i32": return pkg.synth.t1_counts(G, S, seed).astype(np.int32)
    if kind == "f64": return pkg.synth.float_expr(G, S, seed)
    if kind == "f32": return pkg.synth.float_expr(G, S, seed).astype(np.float32)
    if kind == "f16": return pkg.synth.float_expr(G, S, seed).astype(np.float16)
    raise ValueError(kind)


SETTINGS = [  # (REO_EAGER_UPLOAD, REO_UPLOAD_THREADS, REO_EAGER_CHUNK)
    (None, None, None), ("1", None, None), ("0", None, None), ("2", "0", None), ("2", "3", "37"), ("2", None, "37"), ("1", "0", "37"), ("0", "3", None),
    ("0", "0", None),
]


@pytest.mark.parametrize("kind", ["i64", "f64", "f32", "i32", "f16"])
@pytest.mark.parametrize("G", [2, 63, 65, 700])
def test_tile_and_chunk_edges(pkg, monkeypatch, kind, G):
    """G on both sides of the 32 x 32 tile and below it, S = 41 (a whole tile and a part), chunks of 37 + 4 columns, a dense array and
    a column slice with a pitch (odd for Float32: rows of the staging image then start anywhere), every way off the host, both call
    orders, every element type (float16 through the C-order cast)."""
    S, seed = 41, 0x5EED0A00 + G
    X = _data(pkg, kind, G, S, seed)
    group = pkg.synth.groups(S)
    ref0 = np.arange(G) % 3 != 1 if G < 10 else pkg.synth.ref_mask(G, max(2, G // 5), seed)
    # Float32: ld = 41 and 53, both odd; float16 reaches the library through the cast of a C-contiguous array only
    pads = (0,) if kind == "f16" else (0, 12 if kind == "f32" else 11)
    for eager, threads, chunk in SETTINGS:
        _setenv(monkeypatch, REO_EAGER_UPLOAD=eager, REO_UPLOAD_THREADS=threads, REO_EAGER_CHUNK=chunk)
        for order in ("matrix_first", "groups_first"):
            want = _run(pkg, np.asfortranarray(X), group, seed, order, False, ref0, degs=G >= 10)
            for pad in pads:
                Xr = _padded(X, pad)
                if kind != "f16":
                    assert Xr.strides == ((S + pad) * X.itemsize, X.itemsize)
                got = _run(pkg, Xr, group, seed, order, True, ref0, degs=G >= 10)
                _same(want, got, (kind, G, eager, threads, chunk, order, pad))
                assert got["link"] > 0


def test_against_the_oracle(pkg, oracle, monkeypatch):
    """not only self-referential: G = 300, S = 40 counts, row-major, against oracle.build_codes / tally / iterate"""
    _setenv(monkeypatch)
    G, S, seed = 300, 40, 0x5EED0A10
    X = pkg.synth.t1_counts(G, S, seed)
    assert X.flags.c_contiguous
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    for order in ("matrix_first", "groups_first"):
        with pkg.Context(device=0, seed=seed) as ctx:
            if order == "matrix_first": ctx.set_matrix(X)
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            if order != "matrix_first": ctx.set_matrix(X)
            assert ctx.info()["rowmajor_upload"] == 1
            ctx.build_pairs(0)
            thr = ctx.get_thresholds()[:, 0]
            code = oracle.build_codes(X.astype(np.float64), gid, 2, 0, thr, seed)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), code)
            assert np.array_equal(ctx.tally(ref0), oracle.tally(code, ref0))
            res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, 4, 5)
            exp, eit, etr = oracle.iterate(code, ref0, 1.0, 0.05, 4, 5)
            assert it == eit and tr == etr
            assert np.array_equal(res[:, 2:11], exp[:, 2:11])
            assert np.allclose(res[:, :2], exp[:, :2], rtol=0, atol=P_ATOL)
            assert np.allclose(res[:, 11:], exp[:, 11:], rtol=STAT_RTOL, atol=1e-9)


@pytest.mark.parametrize("kind", ["growing", "float_mixed", "huge_int"])
def test_the_ladder_changes_on_the_way(pkg, monkeypatch, kind):
    """the patterns of test_pipelined_upload_equals_matrix_first at G = 1100, S = 96, steps at columns 40 and 70, chunks of 32: the form
    of a chunk on the link climbs I16 -> I32 -> (F32 ->) RAW exactly as for the column-major matrix, with its link-byte bounds"""
    G, S, seed = 1100, 96, 0x5EED0A20
    rng = np.random.default_rng(12)
    if kind == "growing":
        X = rng.integers(0, 30000, size=(G, S)); X[:, 40:] += 40000; X[17, 75] = 2 ** 31 - 1; X[G - 1, 90] = -2 ** 31 - 1
    elif kind == "float_mixed":
        X = rng.integers(0, 900, size=(G, S)).astype(np.float64); X[:, 40:] += 70000.0; X[:, 70:] += np.float32(0.25); X[11, 72] = -0.0
        X[:, 85:] = rng.normal(8, 2, size=(G, S - 85))
    else:
        X = rng.integers(-2 ** 40, 2 ** 40, size=(G, S))
    assert X.flags.c_contiguous
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, G // 5, seed)
    # the last two: host threads on and REO_ROWMAJOR_COPY=2d -- narrowed chunks through the 4-byte pinned slots next to RAW chunks as
    # 2-D copies into the 8-byte device slots, on both upload paths
    for eager, threads, chunk, copy in (("2", None, "32", None), ("2", "3", "32", None), ("0", None, None, None), ("1", "0", "32", None),
                                        ("2", None, None, None), ("2", None, "32", "2d"), ("0", "3", None, "2d")):
        _setenv(monkeypatch, REO_EAGER_UPLOAD=eager, REO_UPLOAD_THREADS=threads, REO_EAGER_CHUNK=chunk, REO_ROWMAJOR_COPY=copy)
        for order in ("groups_first", "matrix_first"):
            want = _run(pkg, np.asfortranarray(X), group, seed, order, False, ref0)
            for pad in (0, 5):
                got = _run(pkg, _padded(X, pad), group, seed, order, True, ref0)
                _same(want, got, (kind, eager, threads, chunk, copy, order, pad))
                link = got["link"]
                if kind == "huge_int" or threads == "0":
                    assert link == X.size * 8, (kind, link)
                elif chunk == "32" and order == "groups_first":
                    assert X.size * 2 < link < X.size * 8, (kind, link)      # chunk by chunk: the narrowest form that fits
                else:
                    assert X.size * 2 <= link <= X.size * 8, (kind, link)


@pytest.mark.parametrize("kind", ["unequal", "interleaved", "three_groups"])
def test_groups(pkg, monkeypatch, kind):
    G, S, seed = 700, 41, 0x5EED0A30
    rng = np.random.default_rng(13)
    X = pkg.synth.t1_counts(G, S, seed)
    group = {"unequal": ["u"] * 9 + ["v"] * (S - 9), "interleaved": [("u", "v")[int(b)] for b in rng.integers(0, 2, S)],
             "three_groups": ["a"] * 12 + ["b"] * 15 + ["c"] * 14}[kind]
    ref0 = pkg.synth.ref_mask(G, 140, seed)
    for chunk in (None, "16"):
        _setenv(monkeypatch, REO_EAGER_CHUNK=chunk)
        for order in ("groups_first", "matrix_first"):
            want = _run(pkg, np.asfortranarray(X), group, seed, order, False, ref0)
            for pad in (0, 11):
                _same(want, _run(pkg, _padded(X, pad), group, seed, order, True, ref0), (kind, chunk, order, pad))


def test_ranges(pkg, monkeypatch):
    """the pair kernel's sides over ranges of blocks, fed by transposed chunks"""
    G, S, seed = 1100, 300, 0x5EED0A40
    X = pkg.synth.t1_counts(G, S, seed)
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 220, seed)
    _setenv(monkeypatch, REO_EAGER_RANGES="4", REO_EAGER_CHUNK="32")
    want = _run(pkg, np.asfortranarray(X), group, seed, "groups_first", False, ref0)
    for pad in (0, 7):
        got = _run(pkg, _padded(X, pad), group, seed, "groups_first", True, ref0)
        _same(want, got, ("ranges", pad))
        assert got["ranges"] >= 4 and got["ranges"] == want["ranges"]


def test_above_the_gene_limit_of_the_pipelined_path(pkg, monkeypatch):
    """G = 66 000: upload_columns, chunks of 63 + 1 columns, indices beyond 2^22 elements per chunk; pair counts on the corner blocks and
    three random ones against the column-major run (no class table: 66 000^2 pairs)"""
    _setenv(monkeypatch)
    G, S, seed = 66000, 64, 0x5EED0A50
    rng = np.random.default_rng(14)
    X = rng.integers(0, 50000, size=(G, S))                  # C-ordered Int64: I32 on the link
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    blocks = [(0, 40, 0, 40), (0, 40, G - 40, G), (G - 40, G, G - 40, G)]
    for _ in range(3):
        i, j = (int(v) for v in rng.integers(0, G - 48, 2))
        blocks.append((i, i + 48, j, j + 48))
    out = []
    for A, rm in ((np.asfortranarray(X), 0), (X, 1)):
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_matrix(A)
            assert ctx.info()["rowmajor_upload"] == rm
            ctx.set_groups(gid, 2)
            out.append(([ctx.pair_counts(*b) for b in blocks], ctx.info()["upload_link_bytes"]))
    assert out[0][1] == out[1][1] == X.size * 4
    for (g0, e0), (g1, e1) in zip(out[0][0], out[1][0]):
        assert np.array_equal(g0, g1) and np.array_equal(e0, e1)


def test_infinities_and_nan(pkg, monkeypatch):
    _setenv(monkeypatch)
    G, S, seed = 300, 41, 0x5EED0A60
    X = pkg.synth.float_expr(G, S, seed)
    X[0, 3] = np.inf; X[0, 30] = -np.inf; X[G - 1, 3] = np.inf; X[G - 1, 40] = -np.inf; X[G - 1, 0] = np.inf
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    for order in ("groups_first", "matrix_first"):
        for A in (X, X.astype(np.float32)):
            want = _run(pkg, np.asfortranarray(A), group, seed, order, False, ref0)
            _same(want, _run(pkg, _padded(A, 11), group, seed, order, True, ref0), ("inf", order, A.dtype))
    # a NaN is refused by the call that reads the matrix: set_matrix when the groups are known, build_pairs otherwise -- in both layouts
    Xn = pkg.synth.float_expr(G, S, seed); Xn[3, 5] = np.nan
    gid, lev = pkg.encode_groups(group)
    for A in (np.asfortranarray(Xn), Xn):
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            with pytest.raises(pkg.DimensionMismatch, match="contains NaN") as e:
                ctx.set_matrix(A)
            assert e.value.status == pkg._ffi.REO_EINVAL
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_matrix(A)
            assert ctx.info()["rowmajor_upload"] == (0 if A.flags.f_contiguous else 1)
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            with pytest.raises(pkg.DimensionMismatch, match="contains NaN"):
                ctx.build_pairs(0)


def test_arguments(pkg, monkeypatch):
    _setenv(monkeypatch)
    L = pkg._ffi.lib()
    G, S, seed = 300, 24, 0x5EED0A70
    X = pkg.synth.t1_counts(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 60, seed)
    want = _run(pkg, np.asfortranarray(X), group, seed, "groups_first", False, ref0)
    for name, A in (("i64", X), ("f64", X.astype(np.float64)), ("f32", X.astype(np.float32)), ("i32", X.astype(np.int32))):
        fn = getattr(L, "reo_set_matrix_rm_" + name)
        with pkg.Context(device=0, seed=seed) as ctx:
            ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
            for args, words in (((A.ctypes.data, G, S, S - 1), (str(S - 1), str(S))), ((None, G, S, S), ("null",)),
                                ((A.ctypes.data, 1, S, S), ("1 x",)), ((A.ctypes.data, G, 1, S), ("x 1",))):
                assert fn(ctx._h, ctypes.c_void_p(args[0]), *args[1:]) == pkg._ffi.REO_EINVAL, (name, args[1:])
                msg = L.reo_last_error().decode()
                assert msg and all(w in msg for w in words), (name, args[1:], msg)
            # the context is still usable
            pkg._ffi.check(fn(ctx._h, A.ctypes.data, G, S, S))
            ctx.G, ctx.S = G, S
            assert ctx.info()["rowmajor_upload"] == 1
            ctx.build_pairs(0)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), want["per_k"][0][0]), name
            if name in ("i64", "i32"):
                assert np.array_equal(ctx.tally(ref0), want["per_k"][0][1])


def test_two_shards_on_one_device(pkg, monkeypatch):
    _setenv(monkeypatch)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    G, S, seed = 3300, 72, 0x5EED0A80
    X = pkg.synth.float_expr(G, S, seed).astype(np.float32)
    assert X.flags.c_contiguous
    group = pkg.synth.groups(S)
    ref0 = pkg.synth.ref_mask(G, 700, seed)
    for order in ("matrix_first", "groups_first"):
        want = _run(pkg, np.asfortranarray(X), group, seed, order, False, ref0)
        one = _run(pkg, X, group, seed, order, True, ref0)
        two = _run(pkg, X, group, seed, order, True, ref0, n_gpus=2)
        _same(want, one, ("one context", order))
        two["link"] = want["link"]       # (the leader's upload is not pipelined in a multi context: only the results are compared)
        _same(want, two, ("two shards", order))


def test_second_matrix_on_the_same_context(pkg, monkeypatch):
    _setenv(monkeypatch)
    seed = 0x5EED0A90
    A = pkg.synth.t1_counts(500, 41, seed)                     # row-major
    B = np.asfortranarray(pkg.synth.float_expr(333, 50, seed + 1))   # column-major, another shape and type
    refA, refB = pkg.synth.ref_mask(500, 100, seed), pkg.synth.ref_mask(333, 60, seed)
    wantA = _run(pkg, np.asfortranarray(A), pkg.synth.groups(41), seed, "groups_first", False, refA)
    wantB = _run(pkg, B, pkg.synth.groups(50), seed, "groups_first", False, refB)
    for first in ("rm", "cm"):
        with pkg.Context(device=0, seed=seed) as ctx:
            for which in ((first, "cm" if first == "rm" else "rm", first)):
                X, S, ref, want = (A, 41, refA, wantA) if which == "rm" else (B, 50, refB, wantB)
                gid, lev = pkg.encode_groups(pkg.synth.groups(S))
                ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
                ctx.set_matrix(X)
                assert ctx.info()["rowmajor_upload"] == (1 if which == "rm" else 0)
                ctx.build_pairs(0)
                G = X.shape[0]
                assert np.array_equal(ctx.get_codes(0, G, 0, G), want["per_k"][0][0]), (first, which)
                assert np.array_equal(ctx.tally(ref), want["per_k"][0][1]), (first, which)
                r = ctx.identify_degs(ref, 1.0, 0.05, 6, 0)
                assert r[1] == want["per_k"][0][2][1] and np.array_equal(r[0], want["per_k"][0][2][0], equal_nan=True)


def test_public_call(pkg, monkeypatch):
    """pkg.identify_degs on a C-ordered array: the new route equals the old one (REO_ROWMAJOR=0) bit for bit, and takes it"""
    G, S, seed = 900, 41, 0x5EED0AA0
    group = pkg.synth.groups(S)
    names = [f"g{i}" for i in range(G)]
    ref0 = pkg.synth.ref_mask(G, 150, seed)
    for X in (pkg.synth.t1_counts(G, S, seed), pkg.synth.float_expr(G, S, seed).astype(np.float32)):
        assert X.flags.c_contiguous
        _setenv(monkeypatch, REO_ROWMAJOR="0")
        old = pkg.run_identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
        _setenv(monkeypatch)
        new = pkg.run_identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
        assert old.info["rowmajor_upload"] == 0 and new.info["rowmajor_upload"] == 1
        assert old.info["upload_link_bytes"] == new.info["upload_link_bytes"]
        assert old.iters_run == new.iters_run and old.trace == new.trace
        assert np.array_equal(old.result, new.result, equal_nan=True) and np.array_equal(old.labels, new.labels)
        a = pkg.identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        monkeypatch.setenv("REO_ROWMAJOR", "0")
        b = pkg.identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed)
        assert a.shape == b.shape == (G, 17) and list(a[:, 0]) == list(b[:, 0]) and list(a[:, 16]) == list(b[:, 16])
        assert np.array_equal(a[:, 1:16].astype(np.float64), b[:, 1:16].astype(np.float64), equal_nan=True)
