"""The masked build on the GPU (reo_set_valid_mask, reo_build_pairs_masked, reo_pair_counts_masked; csrc/maskedpairs.hip): pair classes from
the samples where both genes of a pair are valid.  The expected values come from the numpy restatement of the definition
(tests/masked_pairs_cases.py): the counts first (reo_pair_counts_masked over the whole matrix), then the whole class table (reo_get_codes).
With an all-ones mask the table is that of the plain build, byte for byte.  Every comparison of counts and codes is exact."""
import numpy as np
import pytest

import masked_pairs_cases as mpc

pytestmark = pytest.mark.gpu

P_ATOL, STAT_RTOL = 1e-6, 1e-7   # tests/test_gpu_parity.py: pval / padj; delta1, delta2, se, z1


def open_masked(pkg, X, V, gid, seed):
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, int(np.max(gid)) + 1)
    ctx.set_matrix(X)
    if V is not None:
        ctx.set_valid_mask(V)
    return ctx


def check_counts_and_codes(pkg, X, V, gid, seed, ks=(0,), min_complete=None, pval_reo=0.01, tag=None):
    """counts, then codes, against the restatement; returns the restated codes of the last k"""
    G = X.shape[0]
    ng = int(np.max(gid)) + 1
    sizes = np.bincount(gid, minlength=ng)
    counts = mpc.masked_counts(X, V, gid, ng)
    with open_masked(pkg, X, V, gid, seed) as ctx:
        got = ctx.pair_counts_masked(0, G, 0, G)
        for name, g, w in zip(("n_gt", "n_eq", "n_avail"), got, counts):
            assert g.dtype == np.int32 and g.shape == w.shape, (tag, name)
            assert np.array_equal(g, w), (tag, name, int((g != w).sum()))
        strip = ctx.pair_counts_masked(G // 3, G // 3 + 5, 1, G - 1)               # a rectangle off the origin
        assert all(np.array_equal(s, w[G // 3: G // 3 + 5, 1: G - 1]) for s, w in zip(strip, counts)), tag
        for k in ks:
            mc = mpc.default_min_complete(sizes, k, pval_reo) if min_complete is None else min_complete
            used = ctx.build_pairs_masked(k, pval_reo, min_complete)
            assert tuple(used) == tuple(mc), (tag, k)
            want = mpc.masked_codes(counts, k, pval_reo, mc, seed)
            code = ctx.get_codes(0, G, 0, G)
            assert np.array_equal(code, want), (tag, k, int((code != want).sum()))
            info = ctx.info()
            assert info["masked_build"] == 1 and info["contrast_treat"] == -1 and info["k1_slot_order"] == 0, (tag, k)
    return want


def test_float64_two_interleaved_groups_with_the_special_genes(pkg):
    """G = 72, 37 / 43, 25 % missing, one gene never observed in the control group, one complete, one with exactly 5 control samples,
    one with a whole 32-slot block invalid: all nine codes and both reasons for class 2 occur in the expected table"""
    X, V, gid, seed = mpc.first_case()
    code, why = mpc.masked_codes(mpc.masked_counts(X, V, gid, 2), 0, 0.01, (8, 8), seed, detail=True)
    assert set(np.unique(code)) == set(range(9)) | {255}
    assert why["short_c"].any() and why["nomaj_c"].any() and why["nomaj_t"].any()
    assert why["short_c"][0, 1:].all() and why["short_c"][2, 3:].all()           # never observed / 5 control samples: short against every partner
    got = check_counts_and_codes(pkg, X, V, gid, seed, tag="first")
    assert np.array_equal(got, code)
    check_counts_and_codes(pkg, X, V, gid, seed, min_complete=(3, 12), tag="first, own min_complete")
    check_counts_and_codes(pkg, X, V, gid, seed, ks=(1,), pval_reo=0.05, tag="first, k = 1 at 0.05")


@pytest.mark.parametrize("dtype", [np.int64, np.float32, np.int32])
def test_counts_with_equality_ties_most_control_sides_short(pkg, dtype):
    """G = 64, 20 / 45, 40 % missing: the jointly observed control samples of most pairs stay below 8"""
    X, V, gid = mpc.count_case(64, (20, 45), 0.40, 0x5EED0B02, dtype=dtype)
    counts = mpc.masked_counts(X, V, gid, 2)
    upper = np.triu_indices(64, 1)
    assert (counts[2][:, :, 0][upper] < 8).mean() > 0.5 and (counts[1].sum(axis=2)[upper] > 0).mean() > 0.5
    check_counts_and_codes(pkg, X, V, gid, 0x5EED0B02, tag=str(dtype))


def test_three_groups_every_comparison(pkg):
    X, V, gid = mpc.float_case(48, (33, 31, 40), 0.30, 0x5EED0B03)
    check_counts_and_codes(pkg, X, V, gid, 0x5EED0B03, ks=(0, 1, 2), tag="three groups")


@pytest.mark.parametrize("G,sizes,kind", [(1100, (12, 9), "ranks"), (65, (12, 9), "ties"), (70, (32, 64), "ties"), (70, (1, 20), "ties"),
                                          (63, (33, 2), "ranks")])
def test_seams(pkg, G, sizes, kind):
    """the second 1024-gene pad and 35 table words; one column into the second 64-lane tile and a ragged row tile; groups of exactly 32
    and 64 samples (no padding slot); a group of one sample"""
    seed = 0x5EED0B10 + G + sizes[0]
    X, V, gid = (mpc.rank_case if kind == "ranks" else mpc.float_case)(G, sizes, 0.30, seed)
    check_counts_and_codes(pkg, X, V, gid, seed, ks=(0, 1) if G < 100 else (0,), tag=(G, sizes))


@pytest.mark.parametrize("G,S,family", [(2000, 200, "ranks"), (600, 120, "t1")])
def test_all_ones_mask_is_the_plain_build(pkg, G, S, family):
    """tie-free (the plain build runs in slot order) and tie-rich (coins): the same table byte for byte, compared in row strips"""
    seed = 0x5EED0B20 + G
    gid = pkg.synth.groups(S)
    gid = pkg.encode_groups(gid)[0]
    if family == "ranks":
        rng = np.random.default_rng(seed)
        X = np.stack([rng.permutation(G) for _ in range(S)], axis=1).astype(np.float64)
    else:
        X = pkg.synth.t1_counts(G, S, seed)
    sizes = np.bincount(gid)
    with open_masked(pkg, X, np.ones(X.shape, dtype=bool), gid, seed) as ctx:
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        assert ctx.info()["masked_build"] == 0
        plain = [ctx.get_codes(i0, min(i0 + 500, G), 0, G) for i0 in range(0, G, 500)]
        for mc in (None, (int(sizes[0]), int(sizes.sum() - sizes[0]))):
            ctx.build_pairs_masked(0, 0.01, mc)
            assert ctx.info()["masked_build"] == 1
            for q, i0 in enumerate(range(0, G, 500)):
                assert np.array_equal(ctx.get_codes(i0, min(i0 + 500, G), 0, G), plain[q]), (family, mc, i0)
        av = ctx.pair_counts_masked(0, 3, 0, G)[2]
        assert np.array_equal(av, np.broadcast_to(sizes.astype(np.int32), av.shape))


def nan_matrix(X, V):
    Xn = X.copy()
    Xn[~V] = np.nan
    return Xn


def test_end_to_end_missing_pairwise(pkg, rn):
    """run_identify_degs(missing="pairwise") on the first case: trace and tallies equal the oracle's iteration on the restated table, the
    statistics within the tolerances of tests/test_gpu_parity.py; the run on the zero-filled matrix differs in a tally"""
    X, V, gid, seed = mpc.first_case()
    G = X.shape[0]
    Xn = nan_matrix(X, V)
    keep = Xn.copy()
    names = [f"g{i}" for i in range(G)]
    ref0 = np.ones(G, dtype=bool)
    code = mpc.masked_codes(mpc.masked_counts(X, V, gid, 2), 0, 0.01, (8, 8), seed)
    exp, it, tr = rn.iterate(code, ref0, 1.0, 0.05, 6, 1)
    assert it >= 3 and tr[-1][0] > 0                                             # several passes, DEGs at the end: the case is not hollow
    run =pkg.run_identify_degs(Xn, gid.tolist(), names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0, missing="pairwise", pairs="reversed")
    assert np.array_equal(np.isnan(Xn), np.isnan(keep)) and np.array_equal(Xn[V], keep[V])     # the caller's array is untouched
    assert run.iters_run == it and run.trace == tr, (run.iters_run, it, run.trace, tr)
    assert np.array_equal(run.result[:, 2:11], exp[:, 2:11])
    assert np.allclose(run.result[:, :2], exp[:, :2], rtol=0, atol=P_ATOL), np.abs(run.result[:, :2] - exp[:, :2]).max()
    assert np.allclose(run.result[:, 11:], exp[:, 11:], rtol=STAT_RTOL, atol=1e-9), np.abs(run.result[:, 11:] - exp[:, 11:]).max()
    cm = run.comparisons[0]
    assert cm["min_complete"] == (8, 8) and cm["k"] == 0 and run.info["masked_build"] == 1
    # pairs="reversed": the lists are the reversed classes of the table against the reference set
    pl, ref = cm["pairs"], cm["ref_mask"]
    degs = np.flatnonzero(run.labels != "no change")
    assert pl.genes.tolist() == degs.tolist()
    for q, g in enumerate(pl.genes):
        partner, pcode = pl.row(q)
        want = np.flatnonzero(ref & np.isin(code[g], (2, 6)))
        assert partner.tolist() == want.tolist() and pcode.tolist() == code[g][want].tolist(), g
    # an explicit mask over the same cells with another filler: the same run
    Xf = X.copy()
    Xf[~V] = 1e6
    run_v = pkg.run_identify_degs(Xf, gid.tolist(), names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0, valid=V)
    assert np.array_equal(run_v.result, run.result) and run_v.trace == run.trace
    # filling the holes instead changes the answer
    filled = pkg.run_identify_degs(np.nan_to_num(Xn), gid.tolist(), names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)
    assert filled.info["masked_build"] == 0 and "min_complete" not in filled.comparisons[0]
    assert not np.array_equal(filled.result[:, 2:11], run.result[:, 2:11])
    # defaults: a NaN is refused as always
    with pytest.raises(pkg.DimensionMismatch, match="contains NaN"):
        pkg.run_identify_degs(Xn, gid.tolist(), names, 0.01, 1.0, 0.05, ref0, 6, 1, seed=seed, device=0)


def test_pair_list_in_context_is_consistent_with_get_codes(pkg):
    X, V, gid, seed = mpc.first_case()
    G = X.shape[0]
    with open_masked(pkg, X, V, gid, seed) as ctx:
        ctx.build_pairs_masked(0)
        ctx.identify_degs(np.ones(G, dtype=bool), 1.0, 0.05, 4, 1)
        code, ref = ctx.get_codes(0, G, 0, G), ctx.ref_mask()
        genes = np.arange(0, G, 5, dtype=np.int32)
        pl = ctx.pair_list(genes, "reversed")
        assert pl.rowptr[-1] > 0
        for q, g in enumerate(genes):
            partner, pcode = pl.row(q)
            want = np.flatnonzero(ref & np.isin(code[g], (2, 6)))
            assert partner.tolist() == want.tolist() and pcode.tolist() == code[g][want].tolist(), g
        assert np.array_equal(ctx.tally(ref), np.stack([(code[:, ref] == c).sum(axis=1) for c in range(9)], axis=1))


def test_state_plain_build_new_labels_new_matrix(pkg):
    X, V, gid, seed = mpc.first_case()
    G, S = X.shape
    counts = mpc.masked_counts(X, V, gid, 2)
    with open_masked(pkg, X, V, gid, seed) as ctx:
        thr_before = ctx.compute_thresholds(0.05)
        ctx.build_pairs_masked(0, 0.01)
        masked = ctx.get_codes(0, G, 0, G)
        assert np.array_equal(ctx.get_thresholds(), thr_before)                   # the context's thresholds are neither read nor changed
        # the plain build gives the plain table, info 31 = 0, and the masked one comes back after it
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        plain = ctx.get_codes(0, G, 0, G)
        assert ctx.info()["masked_build"] == 0 and not np.array_equal(plain, masked)
    with open_masked(pkg, X, None, gid, seed) as ctx:
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), plain)                   # ... what a context without a mask builds
    with open_masked(pkg, X, V, gid, seed) as ctx:
        ctx.build_pairs_masked(0)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), masked)
        # other labels, no new set_valid_mask: the restatement for the new labels
        gid2 = np.asarray(([0] * 3 + [1] * 2) * (S // 5), dtype=np.int32)
        ctx.set_groups(gid2, 2)
        assert ctx.info()["masked_build"] == 0
        ctx.build_pairs_masked(1, 0.01, 5)
        c2 = mpc.masked_counts(X, V, gid2, 2)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), mpc.masked_codes(c2, 1, 0.01, (5, 5), seed))
        assert all(np.array_equal(a, b) for a, b in zip(ctx.pair_counts_masked(0, G, 0, G), c2))
        # refused calls leave the table as it is
        for bad, match in (((0, 0.01, 0), "min_complete"), ((2, 0.01, 5), r"comparison 2 outside \[0,2\)"), ((0, 0.0, 5), "pval_reo"),
                           ((0, 1.5, 5), "pval_reo")):
            with pytest.raises(pkg.DimensionMismatch, match=match):
                ctx.build_pairs_masked(*bad)
        assert ctx.info()["masked_build"] == 1
        with pytest.raises(pkg.DimensionMismatch, match="valid mask has shape"):
            ctx.set_valid_mask(V[:, :-1])
        # a matrix of another shape drops the mask
        ctx.set_matrix(X[:, :-5])
        ctx.set_groups(gid2[:-5], 2)
        with pytest.raises(pkg.DimensionMismatch, match="no validity mask"):
            ctx.build_pairs_masked(0)
        with pytest.raises(pkg.DimensionMismatch, match="no validity mask"):
            ctx.pair_counts_masked(0, 4, 0, 4)
        ctx.set_matrix(X)                                                        # the old shape again: the mask stays dropped
        ctx.set_groups(gid, 2)
        with pytest.raises(pkg.DimensionMismatch, match="no validity mask"):
            ctx.build_pairs_masked(0)
        ctx.set_valid_mask(V)
        ctx.build_pairs_masked(0)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), masked)
        assert counts[2].max() <= 43


def test_plane_reading_queries_are_refused_under_a_mask(pkg):
    X, V, gid, seed = mpc.first_case()
    G = X.shape[0]
    with open_masked(pkg, X, V, gid, seed) as ctx:
        ctx.build_pairs_masked(0)
        ctx.identify_degs(np.ones(G, dtype=bool), 1.0, 0.05, 4, 1)
        genes = np.arange(4, dtype=np.int32)
        csr = (np.array([1], dtype=np.int32), np.array([0, 2], dtype=np.int64), np.array([5, 9], dtype=np.int32))
        calls = {"reo_sample_counts": lambda: ctx.sample_counts(genes, "reversed"), "reo_sample_tests": lambda: ctx.sample_tests(genes),
                 "reo_sample_calls": lambda: ctx.sample_calls(1.0, 0.05, genes), "reo_pair_support": lambda: ctx.pair_support(csr)}
        for name, fn in calls.items():
            with pytest.raises(pkg.DimensionMismatch, match=name + " compares on the bit planes.*validity mask"):
                fn()
        with pytest.raises(pkg.DimensionMismatch, match="reo_build_pairs_contrast compares on the bit planes"):
            ctx.build_contrast(0, 1)
        before = ctx.get_codes(0, G, 0, G)
        ctx.set_valid_mask(None)
        for name, fn in calls.items():
            fn()
        assert np.array_equal(ctx.get_codes(0, G, 0, G), before) and ctx.info()["masked_build"] == 1   # clearing the mask leaves the table
        with pytest.raises(pkg.DimensionMismatch, match="no validity mask"):
            ctx.build_pairs_masked(0)


def test_sharded_and_multi_contexts_are_refused(pkg, monkeypatch):
    X, V, gid, seed = mpc.first_case()
    with open_masked(pkg, X, V, gid, seed) as ctx:
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_build_pairs_masked is not available on a sharded context"):
            ctx.build_pairs_masked(0)
        with pytest.raises(pkg.DimensionMismatch, match="reo_pair_counts_masked is not available on a sharded context"):
            ctx.pair_counts_masked(0, 4, 0, 4)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=seed, n_gpus=2) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        ctx.set_valid_mask(V)
        with pytest.raises(pkg.DimensionMismatch, match="reo_build_pairs_masked is not available on a reo_create_multi context"):
            ctx.build_pairs_masked(0)
