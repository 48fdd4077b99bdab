"""Sample calls on the GPU (reo_sample_calls; csrc/samplecalls.hip): up, down or neither per gene and sample, with Benjamini-Hochberg per
sample column made on the device.  The expected value everywhere is the existing route on the same context -- st =
ctx.sample_tests(q, pm, counts=False), st.calls(a, b) and (st.padj() <= b).sum(0) -- compared byte for byte
(tests/sample_calls_cases.py: same)."""
import numpy as np
import pytest

from query_cases import halves, planted_ranks
import sample_calls_cases as cc

pytestmark = pytest.mark.gpu


def check(ctx, q, pm, a, b, tag=None, st=None):
    st = st if st is not None else ctx.sample_tests(q, pm, counts=False)
    got = ctx.sample_calls(a, b, q, pm)
    calls, cut = cc.same(got, st, a, b, tag)
    return got, st, calls, cut


@pytest.mark.parametrize("n", [1, 31, 32, 33, 65])
def test_tile_edges_of_the_transposes(pkg, n):
    """n rows against S = 70 with the interleaved 33 / 37 labels (the slot map is not the identity): tiles of 32 x 32 end inside the rows
    and inside the samples.  Then the smallest S there is, one sample per group."""
    G, seed = 80, 9
    labels = cc.interleaved_33_37()
    X = cc.tie_rich(G, 70, seed, labels == "b")
    rng = np.random.default_rng(seed + n)
    q = rng.integers(0, G, size=n).astype(np.int32)                              # repeats are rows of their own
    pm = rng.random(G) < 0.7
    with cc.open_ctx(pkg, X, labels, pval_reo=0.05) as ctx:
        got, st, calls, cut = check(ctx, q, pm, 1.0, 0.2, f"n={n}")
        assert got.calls.shape == (n, 70)
        if n >= 31:
            assert (calls == 1).any() and (calls == -1).any() and 0 < cut.max() and cut.min() < n
            assert len({tuple(c) for c in calls.T.tolist()}) > 3                  # the columns differ: their order is checked
        check(ctx, q, pm, 0.05, 0.05, f"n={n} both thresholds", st)
    X2 = cc.tie_rich(G, 2, seed, np.array([False, True]))
    with cc.open_ctx(pkg, X2, np.array(["a", "b"], dtype=object), pval_reo=0.5) as ctx:
        got, st, calls, cut = check(ctx, q, pm, 1.0, 1.0, f"n={n} S=2")
        assert got.calls.shape == (n, 2) and (cut == n).all()


def test_thresholds_and_the_all_zero_mask(pkg):
    G, seed = 127, 4
    labels = cc.interleaved_33_37()
    X = cc.tie_rich(G, 70, seed, labels == "b")
    q = np.concatenate([np.arange(G), [G - 1, 0, 0, 32]]).astype(np.int32)
    pm = np.random.default_rng(seed).random(G) < 0.7
    with cc.open_ctx(pkg, X, labels, pval_reo=0.05) as ctx:
        st = ctx.sample_tests(q, pm, counts=False)
        seen = set()
        for a in (0.0, 0.05, 1.0):
            for b in (0.0, 0.05, 1.0):
                got, _, calls, cut = check(ctx, q, pm, a, b, "thresholds", st)
                seen.add((int((calls != 0).sum()), int(cut.sum())))
                if b == 1.0:
                    assert (cut == q.size).all()
                if a == 0.0 or b == 0.0:
                    assert ((calls != 0) <= (st.pval == 0.0)).all()
        assert len(seen) >= 4                                                    # the thresholds bite differently
        assert np.array_equal(got.calls[G - 1], got.calls[G]) and np.array_equal(got.calls[0], got.calls[G + 1])
        zero = np.zeros(G, dtype=bool)
        none = ctx.sample_tests(q, zero, counts=False)
        assert (none.p_up == 1.0).all() and (none.p_down == 1.0).all()            # every p = 1
        for a, b in ((1.0, 1.0), (1.0, 0.05), (0.05, 0.999), (0.0, 0.0)):
            got, _, calls, cut = check(ctx, q, zero, a, b, "zero mask", none)
            assert (got.calls == 0).all() and (got.n_up == 0).all() and (got.n_down == 0).all()
            assert (got.cut == (q.size if b == 1.0 else 0)).all()
        raw_calls = np.full((q.size, 70), 9, dtype=np.int8)                       # cut, n_up and n_down are optional
        ctx.sample_calls_raw(q, np.ascontiguousarray(pm, dtype=np.uint8), 1.0, 0.2, raw_calls, None, None, None)
        assert raw_calls.tobytes() == st.calls(1.0, 0.2).tobytes()


def test_histogram_tile_seam(pkg):
    """G = 127, S = 70; the rows are the genes over and over, cut to CALL_BINS - 1, CALL_BINS, CALL_BINS + 1 and 2 CALL_BINS + 1: long ties,
    ranks either side of the seam of the histogram tiles, and (padj_deg = 1: every row within the cut) a running sum carried across two
    seams."""
    G, seed, B = 127, 21, pkg._ffi.CALL_BINS
    labels = cc.interleaved_33_37()
    X = cc.tie_rich(G, 70, seed, labels == "b")
    pm = np.random.default_rng(seed).random(G) < 0.8
    with cc.open_ctx(pkg, X, labels, pval_reo=0.05) as ctx:
        for n in (B - 1, B, B + 1, 2 * B + 1):
            q = np.tile(np.arange(G, dtype=np.int32), n // G + 1)[:n]
            st = ctx.sample_tests(q, pm, counts=False)
            got, _, calls, cut = check(ctx, q, pm, 1.0, 0.2, f"seam n={n}", st)
            print(f"n={n}: cut at padj_deg 0.2 between {cut.min()} and {cut.max()}, calls {int((calls != 0).sum())}")
            assert cut.max() > 0 and (calls != 0).any()
            _, _, _, cut5 = check(ctx, q, pm, 0.05, 0.9, f"seam n={n} 0.9", st)
            _, _, _, cut1 = check(ctx, q, pm, 1.0, 1.0, f"seam n={n} 1.0", st)
            assert (cut1 == n).all()
            print(f"n={n}: cut at padj_deg 0.9 between {cut5.min()} and {cut5.max()}")
        assert n == 2 * B + 1 and cut1.max() > 2 * B                             # the carried sum: a cut beyond two tiles


def test_batch_seam(pkg, monkeypatch):
    G, seed = 300, 77
    labels = halves(40)
    X = cc.tie_rich(G, 40, seed, labels == "g1")
    rng = np.random.default_rng(seed)
    q = rng.choice(G, 7, replace=False).astype(np.int32)
    pm = rng.random(G) < 0.6
    with cc.open_ctx(pkg, X, labels) as ctx:
        ref, _, calls, _ = check(ctx, q, pm, 1.0, 0.2, "default batch")
        assert (calls != 0).any()
        for b in ("1", "3"):
            monkeypatch.setenv("REO_SAMPLE_CALLS_BATCH", b)                      # (read per call); 7 queries in batches of 3: a short last batch
            cc.bitwise(ctx.sample_calls(1.0, 0.2, q, pm), ref)
        monkeypatch.delenv("REO_SAMPLE_CALLS_BATCH")
        monkeypatch.setenv("REO_SAMPLE_TESTS_BATCH", "1")                        # the other entry's variable is not read here
        cc.bitwise(ctx.sample_calls(1.0, 0.2, q, pm), ref)


def plane_case(pkg, G, q, marks, seed, tag):
    """the case of the sample tests' plane_case (tests/test_gpu_sample_tests.py): S = 8, the same matrix, queries and mask"""
    S = 8
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, 30000, size=(G, 1)) + rng.integers(0, 6000, size=(G, S))).astype(np.int64)
    X[:20000, 1::2] += 9000
    X = np.asfortranarray(X)
    labels = np.array(["a", "b"] * (S // 2), dtype=object)
    q = np.asarray(q, dtype=np.int32)
    pm = np.zeros(G, dtype=bool)
    pm[rng.choice(G, 194, replace=False)] = True
    pm[list(marks)] = True
    with cc.open_ctx(pkg, X, labels, pval_reo=0.3) as ctx:
        got, st, calls, cut = check(ctx, q, pm, 1.0, 0.2, tag)
        assert (calls != 0).any()
        check(ctx, q, pm, 0.05, 1.0, tag + ", pval_deg", st)


def test_17_plane_layout(pkg):
    """G = 66 000, S = 8, the six queries of the sample tests' case: the other plane layout behind the same calls"""
    plane_case(pkg, 66000, [65999, 0, 40000, 65535, 65536, 7], [0, 4095, 4096, 65535, 65536, 65999], 61, "17 planes")


@pytest.mark.parametrize("k,treat", [(2, None), (1, 2)])
def test_three_groups_and_a_contrast(pkg, k, treat):
    """7 / 40 / 23 samples in a shuffled order: comparison k = 2 against the rest, and the contrast of group 1 against group 2 alone"""
    G, S, seed = 90, 70, 41
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.array(["u"] * 7 + ["v"] * 40 + ["w"] * 23, dtype=object))
    gid, lev = pkg.encode_groups(labels)
    X = cc.tie_rich(G, S, seed, gid != k)
    with cc.open_ctx(pkg, X, labels, k=k, treat=treat) as ctx:
        q = np.arange(G, dtype=np.int32)
        got, st, calls, cut = check(ctx, q, rng.random(G) < 0.8, 1.0, 0.2, f"three groups k={k} treat={treat}")
        assert got.calls.shape == (G, S) and (calls == 1).any() and (calls == -1).any()
        assert len({tuple(c) for c in calls.T.tolist()}) > 3


def test_after_a_real_identify_degs(pkg):
    G, S, seed = 400, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 150, seed)
    names = [f"g{i}" for i in range(G)]
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        ref = ctx.ref_mask()
        q = np.arange(G, dtype=np.int32)
        null, st, calls, cut = check(ctx, q, None, 1.0, 0.05, "NULL mask")       # partner_mask=None: the reference set of the tallies
        cc.bitwise(ctx.sample_calls(1.0, 0.05, q, ref), null)
        cc.bitwise(ctx.sample_calls(1.0, 0.05), null)                             # genes=None: all genes
        treated = np.asarray(gid) != 0
        up, dn = null.calls[:30][:, treated], null.calls[30:60][:, treated]      # the planted genes, in the treated samples
        assert (up == 1).mean() > 0.5 and (dn == -1).mean() > 0.5 and not (up == -1).any() and not (dn == 1).any()
        assert (null.calls[:, ~treated] != 0).mean() < 0.05
        assert np.array_equal(ctx.ref_mask(), ref)                               # the call outdates nothing
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == (iters, trace) and np.array_equal(again[0], result, equal_nan=True)
    args = (X, group, names, 0.01, 1.0, 0.05, ref0, 8, 1)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    off = pkg.run_identify_degs(*args, seed=seed, device=0, sample_calls=False)
    on = pkg.run_identify_degs(*args, seed=seed, device=0, sample_calls=True)
    assert set(plain.comparisons[0]) == cc.TODAY == set(off.comparisons[0]) and set(on.comparisons[0]) == cc.TODAY | {"sample_calls"}
    for r in (off, on):
        assert np.array_equal(r.result, plain.result, equal_nan=True) and r.trace == plain.trace and np.array_equal(r.result, result, equal_nan=True)
    cc.bitwise(on.comparisons[0]["sample_calls"], null)


def test_cells_to_degs_with_sample_calls(pkg):
    seed, G, C = 8, 150, 240
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.integers(1, 30, size=(G, 1)).astype(float), size=(G, C)).astype(np.int64)
    X[: G // 6, C // 2:] *= 3
    X[G // 6: G // 3, : C // 2] *= 3
    labels = ["a"] * (C // 2) + ["b"] * (C - C // 2)
    args = (X, labels, [f"gene{i}" for i in range(G)], 8, 0.01, 1.0, 0.3, np.arange(G) >= G // 3, 8, 1)
    both = pkg.identify_degs_cells(*args, seed=seed, device=0, sample_tests=True, sample_calls=True)
    only = pkg.identify_degs_cells(*args, seed=seed, device=0, sample_calls=True)
    cm = both.run.comparisons[0]
    assert set(only.run.comparisons[0]) == cc.TODAY | {"sample_calls"} and set(cm) == cc.TODAY | {"sample_tests", "sample_calls"}
    assert np.array_equal(cm["result"], only.run.result, equal_nan=True)
    st = cm["sample_tests"]
    light = pkg.SampleTests(st.genes, st.n_above_ctrl, st.n_below_ctrl, None, None, None, st.p_up, st.p_down)
    calls, _ = cc.same(cm["sample_calls"], light, 1.0, 0.3, "cells")              # the run's own thresholds
    assert (calls != 0).any()
    cc.bitwise(only.run.comparisons[0]["sample_calls"], cm["sample_calls"])


def test_reoa_writes_the_same_sample_calls_file(pkg, tmp_path):
    """reoa(use_testdata="yes", sample_calls=True) writes the file that sample_tests=True writes, byte for byte; both options: one file;
    neither: none"""
    dirs = {name: tmp_path / name for name in ("off", "host", "dev", "both")}
    for d in dirs.values():
        d.mkdir()
    kw = dict(use_testdata="yes", seed=0x5EED0001, device=0)
    off = pkg.reoa(work_dir=str(dirs["off"]), **kw)
    assert "sample_calls" not in off.attrs["run"].comparisons[0] and not list(dirs["off"].glob("*sample_calls*"))
    pkg.reoa(work_dir=str(dirs["host"]), sample_tests=True, **kw)
    dev = pkg.reoa(work_dir=str(dirs["dev"]), sample_calls=True, **kw)
    both = pkg.reoa(work_dir=str(dirs["both"]), sample_tests=True, sample_calls=True, **kw)
    name = "fn_expr_group1_group2_sample_calls.tsv"
    want = (dirs["host"] / name).read_bytes()
    assert want.count(b"\n") > 1                                                 # there are calls
    base = {p.name for p in dirs["off"].iterdir()}
    for key in ("dev", "both"):
        assert (dirs[key] / name).read_bytes() == want
        assert sorted(p.name for p in dirs[key].iterdir() if p.name not in base) == [name]
    assert set(dev.attrs["run"].comparisons[0]) == cc.TODAY | {"sample_calls"}
    assert set(both.attrs["run"].comparisons[0]) == cc.TODAY | {"sample_calls", "sample_tests"}
    assert np.array_equal(dev.attrs["run"].result, off.attrs["run"].result, equal_nan=True)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    G, S = 70, 10
    labels = halves(S)
    X = cc.tie_rich(G, S, 5, labels == "g1")
    q = np.arange(G, dtype=np.int32)
    ones = np.ones(G, dtype=np.uint8)
    calls = np.full((G, S), 9, dtype=np.int8)
    ints = np.full(S, -7, dtype=np.int32)
    E = pkg._ffi.REO_EINVAL
    P = pkg._ffi._ptr
    o = lambda a: None if a is None else P(a)   # noqa: E731

    def raw(ctx, genes, n, pm, a, b, out):                                       # the entry itself: a null pointer and a count are separate things
        pkg._ffi.check(ctx._L.reo_sample_calls(ctx._h, o(genes), n, o(pm), a, b, o(out), P(ints), P(ints), P(ints)))

    def untouched():
        return (calls == 9).all() and (ints == -7).all()

    with cc.open_ctx(pkg, X, labels) as ctx:
        msgs = []
        cases = [((None, G, ones, 1.0, 0.05, calls), "genes and calls must not be null"),
                 ((q, G, ones, 1.0, 0.05, None), "genes and calls must not be null"),
                 ((q, 0, ones, 1.0, 0.05, calls), "n_genes = 0"), ((q, -3, ones, 1.0, 0.05, calls), "n_genes = -3"),
                 ((q, (1 << 29) - 1, ones, 1.0, 0.05, calls), r"n_genes = 536870911.*2\^29 - 2"),
                 ((np.array([0, G], dtype=np.int32), 2, ones, 1.0, 0.05, calls), rf"genes\[1\] = {G} is outside \[0, {G}\)"),
                 ((np.array([-1], dtype=np.int32), 1, ones, 1.0, 0.05, calls), r"genes\[0\] = -1"),
                 ((q, G, None, 1.0, 0.05, calls), "partner_mask is null.*reo_identify_degs")]
        for name, at in (("pval_deg", 3), ("padj_deg", 4)):
            for bad, shown in ((float("nan"), "-?nan"), (-0.1, "-0.1"), (1.5, "1.5")):
                args = [q, G, ones, 1.0, 0.05, calls]
                args[at] = bad
                cases.append((tuple(args), rf"{name} = {shown} is not a number in \[0, 1\]"))
        for args, pattern in cases:
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                raw(ctx, *args)
            assert e.value.status == E and "reo_sample_calls" in e.value.message
            msgs.append(e.value.message)
            assert untouched(), pattern                                          # a refused call writes nothing
        assert len(set(msgs)) == 13, msgs
        ctx.identify_degs(np.ones(G, dtype=bool), 1.0, 0.05, 2, 1)
        assert ctx.sample_calls(1.0, 0.05, q).calls.shape == (G, S)                # now there is a reference set
        ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="partner_mask is null.*reo_tally"):
            raw(ctx, q, G, None, 1.0, 0.05, calls)
        assert untouched()
        ctx.sample_calls(1.0, 0.05, q, ones)                                      # an explicit mask still works
        with pytest.raises(pkg.DimensionMismatch, match="partner mask length"):
            ctx.sample_calls(1.0, 0.05, q, ones[:-1])
    with pkg.Context(device=0, seed=1) as ctx:                                   # no table built
        ctx.G, ctx.S = G, S
        with pytest.raises(pkg.DimensionMismatch, match="no class table"):
            raw(ctx, q, G, ones, 1.0, 0.05, calls)
        assert untouched()
    with pkg.Context(device=0, seed=3) as ctx:                                   # a shard's part of the table: as reo_tally
        gid, lev = pkg.encode_groups(labels)
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.1); ctx.set_shard(0, 2); ctx.set_matrix(X)
        ctx.build_pairs(0)
        with pytest.raises(pkg.ReoError) as t:
            ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.ReoError) as e:
            raw(ctx, q, G, ones, 1.0, 0.05, calls)
        assert e.value.status == t.value.status == pkg._ffi.REO_ECOMM and e.value.message == t.value.message
        assert untouched()
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_sample_calls is not available on a reo_create_multi context"):
            raw(ctx, q, G, ones, 1.0, 0.05, calls)
        assert untouched()
