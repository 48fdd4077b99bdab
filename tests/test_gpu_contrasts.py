"""Pairwise group contrasts on the GPU (reo_build_pairs_contrast): the class table of group ctrl against group treat, classified from the
per-group count planes that the one-vs-rest comparisons share.

Expected codes "by composition": gt, eq = oracle.pair_counts over all groups; for i < j and group g, nre_g = gt_g + oracle.tie_wins(seed, i, j,
g, eq_g) (called only where eq_g > 0); ic = nre_ctrl >= m1 ? 3 : (S_ctrl - nre_ctrl >= m1 ? 1 : 2), `it` likewise from nre_treat, S_treat,
m2, with m1 = thr[0, ctrl], m2 = thr[0, treat]; code = 3 (ic - 1) + (it - 1), mirrored with 8 - code; off-diagonal entries only."""
import numpy as np
import pytest

import sharding_mirror

pytestmark = pytest.mark.gpu

P_ATOL = 1e-6      # pval / padj, as tests/test_gpu_parity.py
STAT_RTOL = 1e-7   # delta1, delta2, se, z1


def _check_result(res, exp):
    assert np.array_equal(res[:, 2:11], exp[:, 2:11]), "tallies differ"
    assert np.allclose(res[:, :2], exp[:, :2], rtol=0, atol=P_ATOL), np.abs(res[:, :2] - exp[:, :2]).max()
    assert np.allclose(res[:, 11:], exp[:, 11:], rtol=STAT_RTOL, atol=1e-9), np.abs(res[:, 11:] - exp[:, 11:]).max()


def _nre(oracle, X, gid, C, seed, r0, r1, c0, c1):
    """[r1 - r0, c1 - c0, C] int64: nre_g of the ordered pairs (r, c) of the block; meaningful where r < c (coins are drawn for i < j only)."""
    gt, eq = oracle.pair_counts(np.asarray(X, dtype=np.float64), gid, C, r0, r1, c0, c1)
    n = gt.astype(np.int64)
    for a, b, g in zip(*np.nonzero(eq)):
        if r0 + a < c0 + b:
            n[a, b, g] += oracle.tie_wins(seed, int(r0 + a), int(c0 + b), int(g), int(eq[a, b, g]))
    return n


def _classify(n, sizes, thr, ctrl, treat):
    def side(v, S, m):
        return np.where(v >= m, 3, np.where(S - v >= m, 1, 2))
    ic = side(n[:, :, ctrl], int(sizes[ctrl]), int(thr[0, ctrl]))
    it = side(n[:, :, treat], int(sizes[treat]), int(thr[0, treat]))
    return 3 * (ic - 1) + (it - 1)


def composed_rows(oracle, X, gid, C, thr, seed, i0, i1, contrasts, cache=None):
    """{(ctrl, treat): [i1 - i0, G] codes of rows [i0, i1)} and the off-diagonal mask of the block."""
    G = X.shape[0]
    sizes = np.bincount(gid, minlength=C)
    key = (i0, i1)
    if cache is None or key not in cache:
        up = _nre(oracle, X, gid, C, seed, i0, i1, 0, G)      # pairs (i, j), used where i < j
        lo = _nre(oracle, X, gid, C, seed, 0, G, i0, i1)      # pairs (j, i), used where j < i: the mirror's source
        if cache is not None:
            cache[key] = (up, lo)
    else:
        up, lo = cache[key]
    ii, jj = np.arange(i0, i1)[:, None], np.arange(G)[None, :]
    out = {}
    for ctrl, treat in contrasts:
        cu = _classify(up, sizes, thr, ctrl, treat)
        cl = _classify(lo, sizes, thr, ctrl, treat)
        out[ctrl, treat] = np.where(ii < jj, cu, 8 - cl.T).astype(np.uint8)
    return out, ii != jj


# ---- test 1 / 6: three groups, three element kinds

G1, S1, SEED1 = 260, 47, 77
ORDERED = [(0, 1), (0, 2), (2, 1), (1, 0), (2, 0), (1, 2)]
DEGS = {("int64", 0, 1): 12, ("float64", 0, 1): 12, ("ranks", 0, 1): 12,      # DEGs of the last pass, from the CPU oracle's traces
        ("int64", 0, 2): 11, ("float64", 0, 2): 11, ("ranks", 0, 2): 12,
        ("int64", 2, 1): 24, ("float64", 2, 1): 24, ("ranks", 2, 1): 24}


@pytest.fixture(scope="module")
def case1(pkg, oracle):
    labels = np.array(["a"] * 14 + ["b"] * 17 + ["c"] * 16)[np.random.default_rng(3).permutation(S1)]
    gid, levels = pkg.encode_groups(labels)
    assert np.bincount(gid).tolist() == [17, 16, 14]
    ref0 = np.zeros(G1, dtype=bool)
    ref0[np.random.default_rng(9).choice(G1, 80, replace=False)] = True

    def base():
        rng = np.random.default_rng(77)
        X = rng.integers(0, 40, (G1, 1)) + rng.integers(0, 6, (G1, S1))
        X[0:6, gid == 1] += 12
        X[6:12, gid == 1] -= 12
        X[12:18, gid == 2] += 12
        X[18:24, gid == 2] -= 12
        return rng, X

    # each kind from the generator as the draw of X leaves it (the state at which the recorded DEG counts below were made)
    rng, X = base()
    Xf = X + rng.integers(0, 20, (G1, S1)) * 0.05
    rng, X = base()
    Y = X + rng.permutation(G1 * S1).reshape(G1, S1) / (G1 * S1)
    R = np.argsort(np.argsort(Y, axis=0), axis=0)
    kinds = {"int64": X.astype(np.int64), "float64": Xf.astype(np.float64), "ranks": R.astype(np.float32)}
    thr = np.array([[oracle.threshold(int(n), 0.05) for n in (17, 16, 14)], [oracle.threshold(int(S1 - n), 0.05) for n in (17, 16, 14)]])
    assert thr[0].tolist() == [13, 13, 12]
    exp = {}
    for kind, M in kinds.items():
        codes, off = composed_rows(oracle, M, gid, 3, thr, SEED1, 0, G1, ORDERED)
        for (c, t), code in codes.items():
            assert set(np.unique(code[off]).tolist()) == set(range(9)), (kind, c, t)     # every one of the nine codes occurs
            full = np.where(off, code, 255).astype(np.uint8)                     # (the diagonal as oracle.build_codes leaves it)
            res, iters, trace = oracle.iterate(full, ref0, 1.0, 0.05, 8, 1)
            exp[kind, c, t] = (code, oracle.tally(full, ref0), res, iters, trace)
            if (kind, c, t) in DEGS:
                assert trace[-1][0] == DEGS[kind, c, t] and 1 <= trace[-1][0] <= G1 // 4, (kind, c, t, trace)
    return {"labels": labels, "gid": gid, "levels": levels, "ref0": ref0, "kinds": kinds, "thr": thr, "exp": exp, "off": ~np.eye(G1, dtype=bool)}


@pytest.mark.parametrize("kind", ["int64", "float64", "ranks"])
def test_three_groups_every_ordered_contrast(pkg, case1, kind):
    c1 = case1
    with pkg.Context(device=0, seed=SEED1) as ctx:
        ctx.set_matrix(c1["kinds"][kind]); ctx.set_groups(c1["gid"], 3)
        thr = ctx.compute_thresholds(0.05)
        assert np.array_equal(thr, c1["thr"])
        assert ctx.info()["contrast_treat"] == -1                                   # no table yet
        for c, t in ORDERED:
            code, cont, res, iters, trace = c1["exp"][kind, c, t]
            ctx.build_contrast(c, t)
            info = ctx.info()
            assert info["contrast_treat"] == t and info["shared_group_counts"] == 1 and info["has_ties"] == (0 if kind == "ranks" else 1)
            got = ctx.get_codes(0, G1, 0, G1)
            assert np.array_equal(got[c1["off"]], code[c1["off"]]), (kind, c, t)
            assert np.array_equal(ctx.tally(c1["ref0"]), cont), (kind, c, t)
            r, it, tr = ctx.identify_degs(c1["ref0"], 1.0, 0.05, 8, 1)
            assert it == iters and tr == trace, (kind, c, t, tr, trace)
            _check_result(r, res)
            assert ctx.info()["contrast_treat"] == t
        ctx.build_pairs(1)
        assert ctx.info()["contrast_treat"] == -1                                   # group 1 against the rest


# ---- test 2 / 7: against a two-group run on the two groups' columns

G2, S2, SEED2, C2 = 1100, 83, 0x5EED0011, 5


@pytest.fixture(scope="module")
def case2(pkg):
    gid = np.random.default_rng(5).integers(0, C2, S2).astype(np.int32)
    gid[:C2] = np.arange(C2)  # every group present
    return {"gid": gid, "ref0": pkg.synth.ref_mask(G2, 300, SEED2),
            "t0": pkg.synth.t0_ranks(G2, S2, SEED2), "t1": pkg.synth.t1_counts(G2, S2, SEED2)}


def _subset(gid, ctrl, treat):
    """Columns of the two groups in their own order, and their ids in a two-group context: the group that appears first gets id 0."""
    sel = np.flatnonzero((gid == ctrl) | (gid == treat))
    first = gid[sel[0]]
    sub = np.where(gid[sel] == first, 0, 1).astype(np.int32)
    return sel, sub, (0 if first == ctrl else 1)


@pytest.mark.parametrize("family,contrasts", [("t0", [(0, 1), (3, 1), (4, 2), (2, 0)]), ("t1", [(0, 1), (1, 0)])])
def test_contrast_equals_two_group_run_on_the_columns(pkg, oracle, case2, family, contrasts):
    X, gid, ref0 = case2[family], case2["gid"], case2["ref0"]
    off = ~np.eye(G2, dtype=bool)
    with pkg.Context(device=0, seed=SEED2) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, C2); thr = ctx.compute_thresholds(0.05)
        for c, t in contrasts:
            ctx.build_contrast(c, t)
            got = ctx.get_codes(0, G2, 0, G2)
            res = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
            sel, sub, k = _subset(gid, c, t)
            if family == "t1":
                assert k == (0 if c == 0 else 1)     # ids 0 and 1 keep their coin keys in the subset run
            m = [int(thr[0, c]), int(thr[0, t])]
            code = oracle.build_codes(X[:, sel].astype(np.float64), sub, 2, k, m, SEED2)
            assert np.array_equal(got[off], code[off]), (family, c, t)
            with pkg.Context(device=0, seed=SEED2) as two:
                two.set_matrix(np.asfortranarray(X[:, sel])); two.set_groups(sub, 2)
                thr2 = two.compute_thresholds(0.05)
                assert [int(thr2[0, k]), int(thr2[1, k])] == m                      # the rest of a two-group run IS the other group
                two.build_pairs(k)
                assert np.array_equal(two.get_codes(0, G2, 0, G2)[off], got[off]), (family, c, t)
                res2 = two.identify_degs(ref0, 1.0, 0.05, 8, 1)
            assert res[1] == res2[1] and res[2] == res2[2] and np.array_equal(res[0][:, 2:11], res2[0][:, 2:11]), (family, c, t)


def test_contrast_with_ties_on_row_blocks(pkg, oracle, case2):
    """t1 (ties), contrast (3, 1): the subset run would draw other coins, so the expected codes are composed -- rows [0, 64) and [1024, 1100)"""
    X, gid = case2["t1"], case2["gid"]
    with pkg.Context(device=0, seed=SEED2) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, C2); thr = ctx.compute_thresholds(0.05)
        ctx.build_contrast(3, 1)
        assert ctx.info()["has_ties"] == 1
        for i0, i1 in ((0, 64), (1024, 1100)):
            codes, off = composed_rows(oracle, X, gid, C2, thr, SEED2, i0, i1, [(3, 1)])
            got = ctx.get_codes(i0, i1, 0, G2)
            assert np.array_equal(got[off], codes[3, 1][off]), (i0, i1)


def test_two_shards_add_up(pkg, case2):
    """Contrast (3, 1) of the t1 data on two shards of one device: the shards' raw counters add up to the unsharded tallies."""
    X, gid, ref0 = case2["t1"], case2["gid"], case2["ref0"]
    with pkg.Context(device=0, seed=SEED2) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, C2); ctx.compute_thresholds(0.05)
        ctx.build_contrast(3, 1)
        whole = ctx.tally(ref0)
    tot = 0
    for rank in range(2):
        with pkg.Context(device=0, seed=SEED2) as ctx:
            ctx.set_matrix(X); ctx.set_groups(gid, C2); ctx.compute_thresholds(0.05); ctx.set_shard(rank, 2)
            ctx.build_contrast(3, 1)
            assert ctx.info()["contrast_treat"] == 1
            with pytest.raises(pkg.ReoError):
                ctx.tally(ref0)                      # REO_ECOMM: nothing has exchanged the table
            tot = tot + sharding_mirror.raw_counters(ctx.get_codes(0, G2, 0, G2), ref0)
    assert np.array_equal(sharding_mirror.derive_tallies(tot, ref0), whole)


# ---- test 3: order and cache

def test_order_of_builds_and_the_cached_planes(pkg, case2):
    X, gid = case2["t1"], case2["gid"]
    with pkg.Context(device=0, seed=SEED2) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, C2); ctx.compute_thresholds(0.05)
        ctx.build_pairs(2)
        nbytes = ctx.info()["group_count_bytes"]
        assert nbytes > 0
        ctx.build_contrast(0, 1)
        a = ctx.get_codes(0, G2, 0, G2)
        ctx.build_pairs(0)
        rest = ctx.get_codes(0, G2, 0, G2)
        ctx.build_contrast(0, 1)
        b = ctx.get_codes(0, G2, 0, G2)
        assert np.array_equal(a, b) and not np.array_equal(a, rest)
        assert ctx.info()["group_count_bytes"] == nbytes                            # counted once, never grown
    with pkg.Context(device=0, seed=SEED2) as ctx:                                  # the FIRST build is a contrast: it makes the planes
        ctx.set_matrix(X); ctx.set_groups(gid, C2); ctx.compute_thresholds(0.05)
        ctx.build_contrast(0, 1)
        assert ctx.info()["group_count_bytes"] == nbytes and ctx.info()["shared_group_counts"] == 1
        assert np.array_equal(ctx.get_codes(0, G2, 0, G2), a)


# ---- test 4: two groups

def test_two_groups_route_to_build_pairs(pkg):
    G, S, seed = 65, 10, 4
    X = pkg.synth.t1_counts(G, S, seed)
    gid = np.array([0, 1] * 5, dtype=np.int32)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 2); ctx.compute_thresholds(0.05)
        for k in (0, 1):
            ctx.build_pairs(k)
            want = ctx.get_codes(0, G, 0, G)
            ctx.build_contrast(k, 1 - k)
            assert np.array_equal(ctx.get_codes(0, G, 0, G), want), k
        ctx.build_pairs(0)
        assert not np.array_equal(ctx.get_codes(0, G, 0, G), want)                  # (the two comparisons do differ)


# ---- test 5: refusals

def _refused(pkg, ctx, ctrl, treat, needle, codes, G):
    with pytest.raises(pkg.DimensionMismatch) as e:
        ctx.build_contrast(ctrl, treat)
    assert "reo_build_pairs_contrast: " in str(e.value) and needle in str(e.value), str(e.value)
    if codes is not None:                            # the table built before and the reference mask survive
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes)
        assert ctx.ref_mask().shape == (G,)


def test_refusals_leave_the_table_and_the_mask(pkg, monkeypatch):
    G, S, seed = 64, 30, 6
    X = pkg.synth.t1_counts(G, S, seed)
    gid = (np.arange(S) % 3).astype(np.int32)
    ref0 = pkg.synth.ref_mask(G, 20, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3)
        _refused(pkg, ctx, 0, 1, "thresholds not set", None, G)
        ctx.compute_thresholds(0.05)
        ctx.build_contrast(2, 0)
        ctx.identify_degs(ref0, 1.0, 0.05, 4, 1)
        codes = ctx.get_codes(0, G, 0, G)
        for c, t, needle in ((-1, 1, "ctrl = -1 is outside [0, 3)"), (3, 1, "ctrl = 3 is outside [0, 3)"), (0, 3, "treat = 3 is outside [0, 3)"),
                             (0, -2, "treat = -2 is outside [0, 3)"), (1, 1, "ctrl = treat = 1")):
            _refused(pkg, ctx, c, t, needle, codes, G)
        assert ctx.info()["contrast_treat"] == 0
    with pytest.raises(pkg.DimensionMismatch, match="reo_build_pairs_contrast: null context"):
        pkg._ffi.check(pkg._ffi.lib().reo_build_pairs_contrast(None, 0, 1))
    # the planes switched off: one-vs-rest recounts, a contrast has nothing to classify from
    monkeypatch.setenv("REO_SHARE_GROUP_COUNTS", "0")
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3); ctx.compute_thresholds(0.05)
        ctx.build_pairs(1)
        ctx.identify_degs(ref0, 1.0, 0.05, 4, 1)
        codes = ctx.get_codes(0, G, 0, G)
        _refused(pkg, ctx, 0, 1, "REO_SHARE_GROUP_COUNTS=0", codes, G)
    monkeypatch.delenv("REO_SHARE_GROUP_COUNTS")
    # a reo_create_multi context (the one-device seam of the multi-GPU tests)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=seed, n_gpus=2) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3); ctx.compute_thresholds(0.05)
        ctx.build_pairs(1)
        ctx.identify_degs(ref0, 1.0, 0.05, 4, 1)
        codes = ctx.get_codes(0, G, 0, G)
        _refused(pkg, ctx, 0, 1, "reo_create_multi", codes, G)


def test_more_than_65535_samples_are_refused(pkg):
    G, S, seed = 64, 65600, 8
    X = np.asfortranarray(np.random.default_rng(seed).integers(0, 50, (G, S)).astype(np.int32))
    gid = (np.arange(S) % 3).astype(np.int32)
    ref0 = pkg.synth.ref_mask(G, 20, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3); ctx.compute_thresholds(0.05)
        ctx.build_pairs(0)
        ctx.identify_degs(ref0, 1.0, 0.05, 2, 1)
        codes = ctx.get_codes(0, G, 0, G)
        _refused(pkg, ctx, 0, 1, "more than 65535 samples (65600", codes, G)


# ---- test 6: the explain chain after a contrast

def test_explain_chain_after_a_contrast(pkg, case1):
    c1 = case1
    X = c1["kinds"]["int64"]
    names = [f"g{i}" for i in range(G1)]
    run = pkg.run_identify_degs(X, c1["labels"], names, 0.05, 1.0, 0.05, c1["ref0"], 8, 1, seed=SEED1, device=0,
                                contrasts=[("a", "c")], pairs="reversed", sample_scores=True, pair_support=True)
    assert run.levels == c1["levels"] and len(run.comparisons) == 1 and run.res.shape == (G1, 17)
    cm = run.comparisons[0]
    ctrl, treat = c1["levels"].index("a"), c1["levels"].index("c")
    assert (cm["k"], cm["ctrl"], cm["treat"]) == (ctrl, "a", "c")
    _check_result(cm["result"], c1["exp"]["int64", ctrl, treat][2])
    pl, ps = cm["pairs"], cm["pair_support"]
    n_deg = int((cm["labels"] != "no change").sum())
    assert n_deg >= 1 and len(pl.genes) == n_deg and cm["sample_scores"].net.shape == (n_deg, S1) and int(pl.rowptr[-1]) > 0
    with pkg.Context(device=0, seed=SEED1) as ctx:
        ctx.set_matrix(X); ctx.set_groups(c1["gid"], 3); thr = ctx.compute_thresholds(0.05)
        ctx.build_contrast(ctrl, treat)
        assert np.array_equal(ctx.tally(cm["ref_mask"]), cm["result"][:, 2:11].astype(np.int32))
        codes = ctx.get_codes(0, G1, 0, G1)
    rows = ps.entry_genes
    assert np.array_equal(pl.code, codes[rows, pl.partner]) and np.array_equal(ps.code, pl.code)
    sizes = np.asarray(ps.group_sizes)
    assert sizes.tolist() == [17, 16, 14]
    m1, m2 = int(thr[0, ctrl]), int(thr[0, treat])
    n13, n31 = pl.code == 2, pl.code == 6
    assert n13.any() and n31.any() and (n13 | n31).all()
    gt, eq = ps.n_gt, ps.n_eq
    assert (sizes[ctrl] - gt[n13, ctrl] >= m1).all() and (gt[n13, treat] + eq[n13, treat] >= m2).all()
    assert (gt[n31, ctrl] + eq[n31, ctrl] >= m1).all() and (sizes[treat] - gt[n31, treat] >= m2).all()
    assert np.array_equal(ps.delta(ctrl, treat), gt[:, ctrl] / sizes[ctrl] - gt[:, treat] / sizes[treat])
    assert not np.array_equal(ps.delta(ctrl, treat), ps.delta(ctrl))


# ---- test 8: the 17-plane layout

def test_more_than_65535_genes(pkg, oracle):
    G, S, seed = 65600, 9, 12
    rng = np.random.default_rng(seed)
    X = np.asfortranarray(np.argsort(np.argsort(rng.random((G, S)), axis=0), axis=0).astype(np.float64))   # per-sample ranks: tie-free
    gid = np.array([0, 1, 2] * 3, dtype=np.int32)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3); thr = ctx.compute_thresholds(0.05)
        ctx.build_contrast(2, 0)
        info = ctx.info()
        assert info["has_ties"] == 0 and info["shared_group_counts"] == 1 and info["contrast_treat"] == 0
        for i0 in (0, 32768, 65568):
            codes, off = composed_rows(oracle, X, gid, 3, thr, seed, i0, i0 + 32, [(2, 0)])
            got = ctx.get_codes(i0, i0 + 32, 0, G)
            assert np.array_equal(got[off], codes[2, 0][off]), i0
            assert len(np.unique(got[off])) >= 3
