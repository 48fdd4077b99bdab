"""Leave-one-out cross-validation of the k-TSP selection on the GPU (reo_top_pairs_loo; csrc/toppairsloo.hip): every fold decided on the
device from one set of candidate pairs.  The expected values come from the numpy restatement of the definition
(tests/top_pairs_loo_cases.py: per fold the oracle of the search on the relabelled groups, a greedy walk, the outcome from the values) and
every comparison is exact.  The shapes are the smallest at which the kernels can still go wrong: a block seam inside a side and folds on
both sides of it, ties in the held-out sample, a group on neither side, a side that is a union of groups, thousands of candidates at one
|N| so that the fold's own rank shift decides, all keys equal, and the first gene counts of the 15- and 16-plane chains."""
import numpy as np
import pytest

import masked_pairs_cases as mpc
from query_cases import planted_ranks
import top_pairs_cases as tpc
import top_pairs_loo_cases as lc

pytestmark = pytest.mark.gpu

K = 5


def open_case(pkg, name, seed=11):
    """matrix and groups of a named case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = tpc.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def check(got, exp, tag=None):
    """field by field against a restatement, with the dtypes and shapes of the interface"""
    S, kmax = exp.gene_i.shape
    assert got.gene_i.dtype == np.int32 and got.gene_j.dtype == np.int32 and got.gene_i.shape == (S, kmax), tag
    assert got.num.dtype == np.int64 and got.rank_num.dtype == np.int64 and got.outcome.dtype == np.int8 and got.side.dtype == np.int8, tag
    for f in lc.FIELDS:
        assert np.array_equal(getattr(got, f), getattr(exp, f)), (tag, f, np.argwhere(getattr(got, f) != getattr(exp, f))[:5].tolist())


@pytest.mark.parametrize("name", lc.CASES)
def test_every_fold_equals_the_restatement(pkg, name):
    exp, band, full = lc.expected(name, K), lc.expected_candidates(name, K), tpc.expected(name)
    if name == "float300":                                                       # 33 / 31 interleaved: side A has 33 slots, a block seam inside it
        assert full.sizes == (33, 31)
    if name.startswith("count"):                                                 # ties in the held-out sample: outcome 0, and eq words
        assert (exp.outcome[exp.gene_i >= 0] == 0).any()
    if name == "separated":                                                      # asserted from the oracle: the fold's own Gamma decides picks,
        assert band.n_candidates == 8400 and lc.gamma_decides_otherwise(name, K) >= 1   # and otherwise than the full data's Gamma would
    ctx, a, b = open_case(pkg, name)
    with ctx:
        got = ctx.top_pairs_loo(K, a=a, b=b)
    check(got, exp, name)
    assert (got.a, got.b) == (a, b) and tuple(int(v) for v in got.side_sizes) == full.sizes
    assert (got.cut, got.n_candidates) == (band.cut, band.n_candidates), name
    if name == "three_0_2":                                                      # group 1 is on neither side: no folds there
        assert (got.side == 2).sum() == 33 and (got.gene_i[got.side == 2] == -1).all() and not got.num[got.side == 2].any()
    if name == "level":                                                          # T = 0, every key is 0: the picks in (i, j) order, every vote 0
        assert got.cut == 0 and got.n_candidates == 4950
        assert (got.gene_i == np.arange(0, 2 * K, 2)).all() and (got.gene_j == np.arange(1, 2 * K, 2)).all()
        assert not got.num.any() and not got.votes().any() and (got.error_rate() == 1.0).all()
    v = got.votes()
    assert v.shape == exp.gene_i.shape and np.array_equal(v, np.cumsum(np.sign(exp.num) * exp.outcome, axis=1))


@pytest.mark.parametrize("G", [4096, 32768])
def test_the_15_and_16_plane_chains(pkg, G):
    """k_loo_words is compiled per number of position planes: 15 from 4 096 genes, 16 from 32 768.  Sides of 40 and 24 samples: a block
    seam inside side A, and a cut above 0; the expected picks of every fold from top_pairs_cases.moved_oracle's rule on the training columns."""
    X, gid, genes = tpc.moved_case(G, 31 + G, moved=10, sizes=(40, 24))
    exp = lc.moved_expected(X, gid, genes, 2)
    assert exp.cut > 0
    for s in (0, 1, X.shape[1] - 1):                                             # single folds through moved_oracle itself
        f = lc.moved_fold(X, gid, genes, s, 2)
        assert all(np.array_equal(x, y) for x, y in zip(f, (exp.gene_i[s], exp.gene_j[s], exp.num[s], exp.rank_num[s], exp.outcome[s])))
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        got = ctx.top_pairs_loo(2)
    check(got, exp, G)
    assert got.cut == exp.cut and 0 < got.n_candidates < G * (G - 1) // 2


@pytest.mark.parametrize("name", ["float300", "three_0_2"])
def test_the_result_does_not_depend_on_the_band_or_the_buffer(pkg, monkeypatch, name):
    exp, band = lc.expected(name, K), lc.expected_candidates(name, K)
    X = tpc.case(name)[0]
    ctx, a, b = open_case(pkg, name)
    with ctx:
        first = ctx.top_pairs_loo(K, a=a, b=b)
        again = ctx.top_pairs_loo(K, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PAIRS_LOO_ALL", "1")                          # (read per call) T = 0: every pair is a candidate
        every = ctx.top_pairs_loo(K, a=a, b=b)
        monkeypatch.delenv("REO_TOP_PAIRS_LOO_ALL")
        monkeypatch.setenv("REO_TOP_PAIRS_LOO_CAP", str(band.n_candidates + 1))   # the first emit overflows its 16 records and is resized
        monkeypatch.setenv("REO_TOP_PAIRS_LOO_FIRST", "16")
        resized = ctx.top_pairs_loo(K, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PAIRS_LOO_CAP", str(band.n_candidates - 1))
        P = pkg._ffi._ptr
        S = X.shape[1]
        gi, gj = np.full((S, K), -7, dtype=np.int32), np.full((S, K), -7, dtype=np.int32)
        num, gam = np.full((S, K), -7, dtype=np.int64), np.full((S, K), -7, dtype=np.int64)
        out, side, stats = np.full((S, K), -7, dtype=np.int8), np.full(S, -7, dtype=np.int8), np.full(4, -7, dtype=np.int64)
        with pytest.raises(pkg.ReoError, match=f"reo_top_pairs_loo: {band.n_candidates} pairs reach the cut \\|N\\| >= {band.cut}, at most "
                                               f"{band.n_candidates - 1} candidate records") as e:
            pkg._ffi.check(ctx._L.reo_top_pairs_loo(ctx._h, a, -1 if b is None else b, None, K, P(gi), P(gj), P(num), P(gam), P(out), P(side), P(stats)))
        assert e.value.status == pkg._ffi.REO_ENOMEM
        assert all((x == -7).all() for x in (gi, gj, num, gam, out, side, stats))   # a refused call writes nothing
        monkeypatch.delenv("REO_TOP_PAIRS_LOO_CAP")
        monkeypatch.delenv("REO_TOP_PAIRS_LOO_FIRST")
        after = ctx.top_pairs_loo(K, a=a, b=b)
    for got, tag in ((first, "first"), (again, "again"), (every, "every pair"), (resized, "resized"), (after, "after a refusal")):
        check(got, exp, (name, tag))
    G = X.shape[0]
    assert (every.cut, every.n_candidates) == (0, G * (G - 1) // 2) and (resized.cut, resized.n_candidates) == (first.cut, first.n_candidates)


def test_the_per_fold_route_on_the_device_gives_the_same(pkg):
    """count_i64: every fold through set_groups (the sample set aside) + top_pairs + disjoint + pair_support(outcomes=True)"""
    name = "count_i64"
    X, gid, ng, a, b = tpc.case(name)
    side = lc.sides_of(gid, ng, a, b)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        got = ctx.top_pairs_loo(K, a=a, b=b)
        for s in range(X.shape[1]):
            g = lc.fold_groups(side, s)                                          # (the library numbers groups in order of first appearance)
            _, first = np.unique(g, return_index=True)
            number = np.empty(3, dtype=np.int32)
            number[np.argsort(first)] = np.arange(3)
            ctx.set_groups(number[g], 3)
            tp = ctx.top_pairs(4000, a=int(number[0]), b=int(number[1]))
            at = tp.disjoint(K)
            assert at.size == K
            ps = ctx.pair_support((tp.gene_i[at], np.arange(K + 1, dtype=np.int64), tp.gene_j[at]), outcomes=True)
            assert np.array_equal(got.gene_i[s], tp.gene_i[at]) and np.array_equal(got.gene_j[s], tp.gene_j[at]), s
            assert np.array_equal(got.num[s], tp.num[at]) and np.array_equal(got.rank_num[s], tp.rank_num[at]), s
            assert np.array_equal(got.outcome[s], ps.outcome[:, s].astype(np.int8) - 1), s


def test_gene_mask(pkg):
    name = "float300"
    X, gid, ng, a, b = tpc.case(name)
    mask = tpc.half_mask(X.shape[0])
    exp = lc.restate_candidates(X, gid, ng, a, b, 3, mask)
    assert lc.same(exp, lc.restate(X, gid, ng, a, b, 3, mask))
    ctx, a, b = open_case(pkg, name)
    with ctx:
        got = ctx.top_pairs_loo(3, a=a, b=b, gene_mask=mask)
        check(got, exp, "half of the genes")
        assert (got.cut, got.n_candidates) == (exp.cut, exp.n_candidates)
        assert mask[got.gene_i].all() and mask[got.gene_j].all()
        three = np.zeros(X.shape[0], dtype=bool)
        three[[3, 150, 299]] = True
        few = ctx.top_pairs_loo(3, a=a, b=b, gene_mask=three)                     # three genes: one disjoint pair, -1 afterwards
        check(few, lc.restate(X, gid, ng, a, b, 3, three), "three genes")
        assert (few.gene_i[:, 0] >= 0).all() and (few.gene_i[:, 1:] == -1).all() and (few.gene_j[:, 1:] == -1).all()
        assert (few.cut, few.n_candidates) == (0, 3)
        one = np.zeros(X.shape[0], dtype=bool)
        one[7] = True
        none = ctx.top_pairs_loo(3, a=a, b=b, gene_mask=one)                      # no eligible pair: no pick anywhere
        assert (none.gene_i == -1).all() and none.n_candidates == 0 and (none.side == lc.sides_of(gid, ng, a, b)).all()
        bad = np.ones(X.shape[0], dtype=np.uint8)
        bad[7] = 2
        with pytest.raises(pkg.DimensionMismatch, match=r"reo_top_pairs_loo: gene_mask\[7\] = 2"):
            ctx.top_pairs_loo(3, a=a, b=b, gene_mask=bad)
        with pytest.raises(pkg.DimensionMismatch, match="gene_mask has shape"):
            ctx.top_pairs_loo(3, gene_mask=np.ones(X.shape[0] + 1, dtype=bool))


def test_kmax_of_64(pkg):
    exp = lc.expected("level", 64)                                               # 100 genes: 50 disjoint pairs, then -1
    assert (exp.gene_i[:, 49] == 98).all() and (exp.gene_i[:, 50:] == -1).all()
    ctx, a, b = open_case(pkg, "level")
    with ctx:
        check(ctx.top_pairs_loo(64, a=a, b=b), exp, "kmax = 64")


def test_a_side_of_two_samples_runs_and_a_side_of_one_is_refused(pkg):
    X, _, gid = mpc.count_case(60, (2, 7), 0.0, 21)
    X = np.asfortranarray(X)
    exp = lc.restate(X, gid, 2, 0, None, 3)
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        got = ctx.top_pairs_loo(3)
        check(got, exp, "sides of 2 and 7")
        assert tuple(got.side_sizes) == (2, 7)
        check(ctx.top_pairs_loo(3, a=1, b=0), lc.restate(X, gid, 2, 1, 0, 3), "sides of 7 and 2")
    ctx, a, b = open_case(pkg, "rank130")                                        # sizes (1, 20)
    with ctx:
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_loo: side A has 1 samples, a fold leaves one out"):
            ctx.top_pairs_loo(3, a=a, b=b)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_loo: side B has 1 samples"):
            ctx.top_pairs_loo(3, a=1, b=0)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    X, gid, ng, a, b = tpc.case("three_0_2")
    G, S = X.shape
    ctx, _, _ = open_case(pkg, "three_0_2")
    with ctx:
        for kw, pattern in ((dict(kmax=0), "kmax = 0, between 1 and 64"), (dict(kmax=65), "kmax = 65, between 1 and 64"),
                            (dict(kmax=5, a=0, b=0), "b == a == 0"), (dict(kmax=5, a=3), "a = 3 is outside the groups \\[0, 3\\)"),
                            (dict(kmax=5, a=0, b=3), "b = 3 is outside the groups")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                ctx.top_pairs_loo(**kw)
            assert e.value.status == pkg._ffi.REO_EINVAL and "reo_top_pairs_loo" in e.value.message
        # a refused call writes nothing
        P = pkg._ffi._ptr
        gi, gj = np.full((S, 2), -7, dtype=np.int32), np.full((S, 2), -7, dtype=np.int32)
        num, gam = np.full((S, 2), -7, dtype=np.int64), np.full((S, 2), -7, dtype=np.int64)
        out, side, stats = np.full((S, 2), -7, dtype=np.int8), np.full(S, -7, dtype=np.int8), np.full(4, -7, dtype=np.int64)
        with pytest.raises(pkg.DimensionMismatch, match="b == a"):
            pkg._ffi.check(ctx._L.reo_top_pairs_loo(ctx._h, 2, 2, None, 2, P(gi), P(gj), P(num), P(gam), P(out), P(side), P(stats)))
        with pytest.raises(pkg.DimensionMismatch, match="kmax = 65"):
            pkg._ffi.check(ctx._L.reo_top_pairs_loo(ctx._h, 0, 2, None, 65, P(gi), P(gj), P(num), P(gam), P(out), P(side), P(stats)))
        with pytest.raises(pkg.DimensionMismatch, match="must not be null"):
            pkg._ffi.check(ctx._L.reo_top_pairs_loo(ctx._h, 0, 2, None, 2, P(gi), P(gj), P(num), None, P(out), P(side), P(stats)))
        assert all((x == -7).all() for x in (gi, gj, num, gam, out, side, stats))
        pkg._ffi.check(ctx._L.reo_top_pairs_loo(ctx._h, 0, 2, None, 2, P(gi), P(gj), P(num), P(gam), P(out), P(side), P(stats)))
        exp = lc.expected("three_0_2", 2)
        assert np.array_equal(gi, exp.gene_i) and np.array_equal(num, exp.num) and np.array_equal(side, exp.side)
        assert stats[1] > 0 and stats[2] >= 1 and stats[3] == 32                 # candidates, histogram passes, folds
        ctx.set_valid_mask(np.ones((G, S), dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_loo compares on the bit planes of the whole matrix.*while a mask is set"):
            ctx.top_pairs_loo(5)
        ctx.set_valid_mask(None)
        check(ctx.top_pairs_loo(2, a=0, b=2), exp, "mask cleared")
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_loo is not available on a sharded context"):
            ctx.top_pairs_loo(5)
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.top_pairs_loo(5)
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="no groups"):
            ctx.top_pairs_loo(5)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_loo is not available on a reo_create_multi context"):
            ctx.top_pairs_loo(5)


def test_a_call_disturbs_nothing(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    exp = lc.restate(X, gid, len(lev), 0, None, 3)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        first = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        tp0 = ctx.top_pairs(50)                                                  # (tie-free data: makes the gene-order planes, and sets its own timers)
        codes, ref, info = ctx.get_codes(0, G, 0, G), ctx.ref_mask(), ctx.info()
        got = ctx.top_pairs_loo(3)
        check(got, exp, "after a build")
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes) and np.array_equal(ctx.ref_mask(), ref)
        after = ctx.info()
        own = ("top_pairs_loo_words_us", "top_pairs_loo_select_us")              # (its own two timers; the search's timers keep the last top_pairs')
        assert all(after[k] == info[k] for k in info if k not in own), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        assert after["top_pairs_loo_words_us"] > 0 and after["top_pairs_loo_select_us"] > 0
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == first[1:] and np.array_equal(again[0], first[0], equal_nan=True)
        tp = ctx.top_pairs(50)
        o = tpc.oracle(X, gid, len(lev), 0, None)
        assert np.array_equal(tp.gene_i, o.gene_i[:50]) and np.array_equal(tp.gene_j, o.gene_j[:50]) and np.array_equal(tp.num, o.num[:50])
        assert np.array_equal(tp.rank_num, o.rank_num[:50]) and np.array_equal(tp.gene_i, tp0.gene_i)


def test_run_identify_degs_carries_the_cross_validation(pkg):
    today = {"k", "result", "labels", "iters_run", "trace"}
    X, gid, ng, a, b = tpc.case("count_i64")
    G = X.shape[0]
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    plain = pkg.run_identify_degs(*args, seed=3, device=0)
    on = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs_loo=3)
    assert set(plain.comparisons[0]) == today and set(on.comparisons[0]) == today | {"top_pairs_loo"}   # independent of top_pairs
    assert np.array_equal(on.result, plain.result, equal_nan=True) and on.trace == plain.trace
    got = on.comparisons[0]["top_pairs_loo"]
    check(got, lc.expected("count_i64", 3), "two groups")
    assert (got.a, got.b) == (0, None)
    both = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=10, top_pairs_loo=3)
    assert set(both.comparisons[0]) == today | {"top_pairs", "top_pairs_loo"} and lc.same(both.comparisons[0]["top_pairs_loo"], got)
    # three groups, one contrast: a and b are the contrast's groups
    X, gid, ng, _, _ = tpc.case("three_0_2")
    G = X.shape[0]
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    run = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)], top_pairs_loo=3)
    got = run.comparisons[0]["top_pairs_loo"]
    assert len(run.comparisons) == 1 and (got.a, got.b) == (0, 2)
    check(got, lc.expected("three_0_2", 3), "contrast (0, 2)")
    # the reference's comparisons of three groups: group k against every other sample
    run = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs_loo=3)
    assert [(cm["top_pairs_loo"].a, cm["top_pairs_loo"].b) for cm in run.comparisons] == [(0, None), (1, None), (2, None)]
    check(run.comparisons[1]["top_pairs_loo"], lc.expected("three_1_rest", 3), "group 1 against the rest")


def test_reoa_writes_the_two_files(pkg, tmp_path):
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path), seed=0x5EED0001, device=0, top_pairs_loo=3)
    run = df.attrs["run"]
    loo = run.comparisons[0]["top_pairs_loo"]
    cv = (tmp_path / "fn_expr_group1_group2_top_pairs_cv.tsv").read_text().split("\n")
    assert cv[0].split("\t") == ["k", "n_folds", "n_wrong", "n_undecided", "error"] and cv[-1] == "" and len(cv) == 3 + 2
    e = loo.errors()
    assert cv[1].split("\t") == ["1", str(int(e["n_folds"][0])), str(int(e["n_wrong"][0])), str(int(e["n_undecided"][0])), repr(loo.error_rate(1))]
    folds = (tmp_path / "fn_expr_group1_group2_top_pairs_loo.tsv").read_text().split("\n")
    assert folds[0].split("\t") == ["sample", "side", "votes_1", "votes_2", "votes_3"] and folds[-1] == ""
    assert len(folds) == int((loo.side != 2).sum()) + 2 and int(e["n_folds"][0]) == int((loo.side != 2).sum())
    assert folds[1].split("\t")[1] in ("A", "B") and folds[1].split("\t")[2:] == [str(int(v)) for v in loo.votes()[0]]


def test_cells_to_degs_carries_the_cross_validation(pkg, monkeypatch):
    seed, G, C = 8, 150, 240
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.integers(1, 30, size=(G, 1)).astype(float), size=(G, C)).astype(np.int64)
    X[: G // 6, C // 2:] *= 3
    X[G // 6: G // 3, : C // 2] *= 3
    labels = ["a"] * (C // 2) + ["b"] * (C - C // 2)
    args = (X, labels, [f"gene{i}" for i in range(G)], 8, 0.01, 1.0, 0.3, np.arange(G) >= G // 3, 8, 1)
    plain = pkg.identify_degs_cells(*args, seed=seed, device=0)
    on = pkg.identify_degs_cells(*args, seed=seed, device=0, top_pairs_loo=3)
    monkeypatch.setenv("REO_TOP_PAIRS_LOO_ALL", "1")                              # every pair a candidate: the same folds by another band
    every = pkg.identify_degs_cells(*args, seed=seed, device=0, top_pairs_loo=3)
    assert set(on.run.comparisons[0]) == set(plain.run.comparisons[0]) | {"top_pairs_loo"}
    assert np.array_equal(on.run.result, plain.run.result, equal_nan=True) and on.run.trace == plain.run.trace
    loo = on.run.comparisons[0]["top_pairs_loo"]
    S = loo.side.size
    assert loo.gene_i.shape == (S, 3) and (loo.side != 2).all() and int(loo.side_sizes.sum()) == S == int(loo.errors()["n_folds"][0])
    assert (loo.gene_i >= 0).all() and (loo.gene_i < loo.gene_j).all() and (loo.gene_j < len(on.run.gene_names)).all()
    assert lc.same(loo, every.run.comparisons[0]["top_pairs_loo"]) and every.run.comparisons[0]["top_pairs_loo"].cut == 0
