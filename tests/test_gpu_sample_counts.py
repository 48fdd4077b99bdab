"""Sample counts on the GPU (reo_sample_counts; csrc/samplecounts.hip): in which samples a gene's selected pairs put it above its partner.
The expected counts come from the numpy restatement of the comparators (tests/sample_counts_cases.py) under a partner set taken from the
already-verified parity hook ctx.get_codes plus the masks, as tests/test_gpu_pair_list.py takes it; where the library can say the same
thing another way (reo_pair_counts, the tallies of identify_degs, the thresholds) that is asserted too."""
import numpy as np
import pytest

import float32_cases as fc
from query_cases import band_matrix, code_rows, halves, planted_ranks, tie_rich
import sample_counts_cases as scc

pytestmark = pytest.mark.gpu

ALL = 0x1FF
N13, N31 = 2, 6
TODAY = {"k", "result", "labels", "iters_run", "trace"}


def open_ctx(pkg, X, labels, pval_reo=0.1, seed=11, k=0, matrix_first=False):
    ctx = pkg.Context(device=0, seed=seed)
    gid, lev = pkg.encode_groups(labels)
    if matrix_first:
        ctx.set_matrix(X)
    ctx.set_groups(gid, len(lev))
    ctx.compute_thresholds(pval_reo)
    if not matrix_first:
        ctx.set_matrix(X)
    ctx.build_pairs(k)
    return ctx


def same(got, exp, tag=None, ties=True):
    n_sel, n_gt, n_eq = exp
    assert got.n_sel.dtype == np.int32 and got.n_gt.dtype == np.int32 and got.n_gt.shape == n_gt.shape, tag
    assert np.array_equal(got.n_sel, n_sel), tag
    assert np.array_equal(got.n_gt, n_gt), tag
    if ties:
        assert got.n_eq.dtype == np.int32 and np.array_equal(got.n_eq, n_eq), tag
        assert np.array_equal(got.n_lt, n_sel[:, None] - n_gt - n_eq) and got.n_lt.min(initial=0) >= 0, tag
    else:
        assert got.n_eq is None, tag


def check(ctx, X, genes, classes, pm, pkg, rows=None, st=None, tag=None, ties=True):
    """one call against the restatement; X is the matrix in the arithmetic that the library compares in"""
    genes = np.asarray(genes, dtype=np.int32)
    rows = rows if rows is not None else code_rows(ctx, genes)
    exp = scc.expected_counts(X, lambda i: rows[i], genes, pkg._ffi.class_mask(classes), pm, st)
    got = ctx.sample_counts(genes, classes, pm, ties=ties)
    assert np.array_equal(got.genes, genes)
    same(got, exp, tag, ties)
    return got, exp


@pytest.mark.parametrize("G", [33, 64, 65, 127])
def test_word_tails_every_class_mask_repeats_and_empty_selections(pkg, G):
    """S = 10 (5 + 5): one block per group, 27 padding slots each.  All 511 class masks on rows either side of the word boundaries, the last
    gene included; "reversed" under a random partner mask; queries repeated and out of order; empty selections; ties=False."""
    S, seed = 10, 5
    labels = halves(S)
    X = tie_rich(G, S, seed, labels == "g1")
    rng = np.random.default_rng(seed)
    with open_ctx(pkg, X, labels) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        assert set(range(9)) <= set(np.unique(codes).tolist()) and (np.diag(codes) == 255).all()
        rows = {i: codes[i] for i in range(G)}
        q = np.array(sorted({0, 1, 30, 31, 32, G // 2, G - 2, G - 1}), dtype=np.int32)
        st = scc.states(X, q)
        ones = np.ones(G, dtype=bool)
        nonzero = 0
        for mask in range(1, ALL + 1):
            got, exp = check(ctx, X, q, mask, ones, pkg, rows, st, mask)
            nonzero += int(exp[2].sum() > 0 and exp[1].sum() > 0)
        assert nonzero > 400                                                     # (greater and tied outcomes both occur under most masks)
        pm = rng.random(G) < 0.6
        check(ctx, X, q, "reversed", pm, pkg, rows, st)
        rep = np.array([G - 1, 0, 0, 32, G - 1, 31, 0], dtype=np.int32)            # repeats, any order: every entry is its own row
        got, _ = check(ctx, X, rep, ALL, pm, pkg, rows)
        assert np.array_equal(got.n_gt[0], got.n_gt[4]) and np.array_equal(got.n_gt[1], got.n_gt[2]) and np.array_equal(got.n_gt[2], got.n_gt[6])
        got, _ = check(ctx, X, q, ALL, np.zeros(G, dtype=bool), pkg, rows, st)    # nothing selected
        assert (got.n_sel == 0).all() and (got.n_gt == 0).all() and (got.n_eq == 0).all()
        only = np.zeros(G, dtype=bool); only[32] = True
        got, _ = check(ctx, X, [32, 0], ALL, only, pkg, rows)                     # the query gene alone: the diagonal is no pair
        assert got.n_sel.tolist() == [0, 1] and (got.n_gt[0] == 0).all() and (got.n_eq[0] == 0).all()
        check(ctx, X, q, ALL, pm, pkg, rows, st, ties=False)
        check(ctx, X, q, 0x44, ones, pkg, rows, st, ties=False)
        got, _ = check(ctx, X, [G - 1], "n22", ones, pkg, rows)                   # n_genes = 1
        assert got.n_gt.shape == (1, S)


def test_interleaved_labels_33_and_37(pkg):
    """G = 127, S = 70, labels a b a b ...: the slot map is not the identity, a has 33 samples (two blocks, 31 pads), b 37 (27 pads)"""
    G, S, seed = 127, 70, 9
    labels = np.array(["a" if (s % 2 == 0 and s < 66) else "b" for s in range(S)], dtype=object)
    assert (labels == "a").sum() == 33 and (labels == "b").sum() == 37
    X = tie_rich(G, S, seed, labels == "b")
    X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)                  # every sample its own pattern: a swapped column shows
    with open_ctx(pkg, X, labels, pval_reo=0.05) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        assert set(range(9)) <= set(np.unique(codes).tolist())
        rows = {i: codes[i] for i in range(G)}
        q = np.arange(G, dtype=np.int32)
        st = scc.states(X, q)
        pm = np.random.default_rng(seed).random(G) < 0.7
        for mask in (ALL, 0x44, 1 << N13, 0x1EF):
            got, exp = check(ctx, X, q, mask, pm, pkg, rows, st, mask)
        assert len({tuple(c) for c in exp[1].T.tolist()}) > S // 2              # the columns differ: their order is checked


@pytest.mark.parametrize("k", [0, 2])
def test_three_unbalanced_groups(pkg, k):
    """7 / 40 / 23 samples in a shuffled order, comparison k against the rest: counts for every sample of every group"""
    G, S, seed = 90, 70, 41
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.array(["u"] * 7 + ["v"] * 40 + ["w"] * 23, dtype=object))
    gid, lev = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, gid == k)
    with open_ctx(pkg, X, labels, k=k) as ctx:
        q = np.arange(G, dtype=np.int32)
        codes = ctx.get_codes(0, G, 0, G)
        rows = {i: codes[i] for i in range(G)}
        st = scc.states(X, q)
        pm = rng.random(G) < 0.7
        got, exp = check(ctx, X, q, ALL, pm, pkg, rows, st)
        assert exp[1].sum() > 0 and exp[2].sum() > 0
        got, exp = check(ctx, X, q, "reversed", np.ones(G, dtype=bool), pkg, rows, st)
        assert exp[0].sum() > 0


def test_counter_depth_tile_seam_and_batch_seam(pkg, monkeypatch):
    """G = 4 500, class 0x1FF, mask all ones: the first tile of 4 096 columns lists 4 095 or 4 096 partners, so lanes take 64 of them (the
    seventh counter plane), and the row spans two tiles.  Then the same eight queries in batches of three."""
    G, S, seed = 4500, 40, 77
    labels = halves(S)
    X = tie_rich(G, S, seed, labels == "g1")
    rng = np.random.default_rng(seed)
    q = np.concatenate([[0, 4095, 4096, 4499], rng.choice(G, 4, replace=False)]).astype(np.int32)
    ones = np.ones(G, dtype=bool)
    with open_ctx(pkg, X, labels) as ctx:
        rows = code_rows(ctx, q)
        st = scc.states(X, q)
        got, exp = check(ctx, X, q, ALL, ones, pkg, rows, st)
        assert (got.n_sel == G - 1).all() and exp[2].max() > 64 and exp[1].max() > 2048
        got44, _ = check(ctx, X, q, "reversed", ones, pkg, rows, st)
        monkeypatch.setenv("REO_SAMPLE_COUNTS_BATCH", "3")                        # (read per call)
        again, _ = check(ctx, X, q, ALL, ones, pkg, rows, st, "batches of 3")
        assert np.array_equal(again.n_gt, got.n_gt) and np.array_equal(again.n_eq, got.n_eq)
        check(ctx, X, q, ALL, ones, pkg, rows, st, "batches of 3", ties=False)
        monkeypatch.setenv("REO_SAMPLE_COUNTS_BATCH", "1")
        check(ctx, X, q, "reversed", ones, pkg, rows, st, "batches of 1")


def test_float64_band(pkg):
    G, S, seed = 70, 12, 3
    X = band_matrix(G, S, seed)
    tied = [scc.sample_states(X[:, s], 2 * k)[1][2 * k + 1] for s in range(S) for k in range(5)]
    assert any(tied) and not all(tied)                                           # planted pairs fall on both sides of the band
    q = np.arange(G, dtype=np.int32)
    with open_ctx(pkg, X, halves(S)) as ctx:
        got, exp = check(ctx, X, q, ALL, np.ones(G, dtype=bool), pkg)
        assert exp[2].sum() > 0
        check(ctx, X, q, "reversed", np.ones(G, dtype=bool), pkg)


def test_float32_rule_on_planted_flip_pairs(pkg):
    G, S, seed = 60, 12, 13
    X = fc.planted(G, S, 4, seed)
    assert X.dtype == np.float32 and fc.disagreements(X)[0] >= 4 * S
    q = np.arange(G, dtype=np.int32)
    ones = np.ones(G, dtype=bool)
    with open_ctx(pkg, np.asfortranarray(X), halves(S)) as ctx:
        assert ctx.info()["resident_dtype"] == 3
        rows = code_rows(ctx, q)
        got, exp = check(ctx, X, q, ALL, ones, pkg, rows)
        widened = scc.expected_counts(X.astype(np.float64), lambda i: rows[i], q, ALL, ones)
        assert not np.array_equal(widened[2], exp[2])                            # the Float64 rule would count other ties


def test_int32_equals_int64(pkg):
    G, S, seed = 65, 10, 23
    labels = halves(S)
    X = tie_rich(G, S, seed, labels == "g1")
    q = np.arange(G, dtype=np.int32)
    pm = np.random.default_rng(seed).random(G) < 0.8
    out = []
    for Xt in (X, X.astype(np.int32)):
        with open_ctx(pkg, np.asfortranarray(Xt), labels) as ctx:
            out.append(check(ctx, X, q, ALL, pm, pkg)[0])
    assert np.array_equal(out[0].n_gt, out[1].n_gt) and np.array_equal(out[0].n_eq, out[1].n_eq) and np.array_equal(out[0].n_sel, out[1].n_sel)


@pytest.mark.parametrize("matrix_first", [True, False])
def test_infinities_and_both_orders_of_calls(pkg, matrix_first):
    """+-Inf, two equal infinities in one sample included: the larger index is the greater one, nothing is tied.  Matrix first, and groups
    first (the pipelined upload)."""
    G, S, seed = 80, 12, 31
    X = pkg.synth.with_infinities(pkg.synth.float_expr(G, S, seed), seed, "log0")
    X[3, 0] = X[7, 0] = np.inf
    X[5, 1] = X[9, 1] = -np.inf
    X[11, 2], X[12, 2] = np.inf, -np.inf
    X = np.asfortranarray(X)
    assert np.isinf(X).sum() > 2 * S
    q = np.arange(G, dtype=np.int32)
    with open_ctx(pkg, X, halves(S), matrix_first=matrix_first) as ctx:
        got, exp = check(ctx, X, q, ALL, np.ones(G, dtype=bool), pkg)
        one7 = np.zeros(G, dtype=bool); one7[7] = True
        one3 = np.zeros(G, dtype=bool); one3[3] = True
        a = ctx.sample_counts([3], ALL, one7)
        b = ctx.sample_counts([7], ALL, one3)
        assert (a.n_gt[0, 0], a.n_eq[0, 0], b.n_gt[0, 0], b.n_eq[0, 0]) == (0, 0, 1, 0)
        check(ctx, X, q, "reversed", np.ones(G, dtype=bool), pkg)


def test_one_hot_mask_against_pair_counts(pkg):
    """partner_mask = {j}, class 0x1FF: n_gt[q, s] is the outcome of the single pair (i, j) in sample s, and its sums over each group's
    samples are reo_pair_counts' -- a second implementation inside the library, with no numpy comparator in between"""
    G, S, seed = 40, 14, 51
    labels = np.array(["a", "b"] * (S // 2), dtype=object)
    gid, _ = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, gid == 1)
    q = np.arange(G, dtype=np.int32)
    with open_ctx(pkg, X, labels) as ctx:
        for j in range(G):
            pm = np.zeros(G, dtype=bool); pm[j] = True
            sc = ctx.sample_counts(q, ALL, pm)
            assert sc.n_sel.tolist() == [int(i != j) for i in range(G)]
            assert set(np.unique(sc.n_gt).tolist()) <= {0, 1} and set(np.unique(sc.n_gt + sc.n_eq).tolist()) <= {0, 1}
            gt, eq = ctx.pair_counts(0, G, j, j + 1)
            for g in range(2):
                keep = q != j
                assert np.array_equal(sc.n_gt[:, gid == g].sum(axis=1)[keep], gt[keep, 0, g].astype(np.int64)), (j, g)
                assert np.array_equal(sc.n_eq[:, gid == g].sum(axis=1)[keep], eq[keep, 0, g].astype(np.int64)), (j, g)


def test_after_a_slot_order_build_the_gene_order_planes_are_intact(pkg):
    G, S, seed = 70, 12, 21
    rng = np.random.default_rng(seed)
    X = rng.permuted(np.tile(3.0 * np.arange(G)[:, None], (1, S)), axis=0)      # tie-free Float64: every sample a permutation of 0, 3, 6, ...
    X[: G // 5, S // 2:] += 60.5                                                # (shifted genes stay 0.5 away from everything else)
    X = np.asfortranarray(X)
    with open_ctx(pkg, X, halves(S), matrix_first=True) as ctx:                  # (groups first would pair the sides as they arrive: identity order)
        assert ctx.info()["k1_slot_order"] == 1 and ctx.info()["has_ties"] == 0
        q = np.arange(G, dtype=np.int32)
        rows = code_rows(ctx, q)
        st = scc.states(X, q)
        for mask in (ALL, 0x44):
            got, exp = check(ctx, X, q, mask, np.ones(G, dtype=bool), pkg, rows, st, mask)
            assert (got.n_eq == 0).all()


def plane_case(pkg, G, q, marks, seed, X=None):
    """S = 8, labels a b a b ..., class 0x1FF under a mask of `marks` and 1 000 random partners; X: Int64 below 30 000 (ties by equality)
    unless given, and a given matrix is tie-free"""
    S = 8
    tie_free = X is not None
    X, pm = scc.plane_case_data(G, marks, seed, X, S)
    labels = np.array(["a", "b"] * (S // 2), dtype=object)
    q = np.asarray(q, dtype=np.int32)
    with open_ctx(pkg, X, labels, pval_reo=0.3) as ctx:
        got, exp = check(ctx, X, q, ALL, pm, pkg)
        assert got.n_sel.tolist() == [int(pm.sum()) - int(pm[i]) for i in q]
        assert exp[1].sum() > 0 and (exp[2].sum() == 0 if tie_free else exp[2].sum() > 0)
        check(ctx, X, q, ALL, pm, pkg, ties=False)


def test_17_plane_layout(pkg):
    """G = 65 600: five pos quads, edge rows of eight uint4, plane k in word k; partners either side of 65 536"""
    plane_case(pkg, 65600, [65599, 0, 40000], [0, 4095, 4096, 65535, 65536, 65599], 61)


def test_after_a_real_identify_degs(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    names = [f"g{i}" for i in range(G)]
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        degs = np.flatnonzero(pkg.label_genes(result, 1.0, 0.05) != "no change").astype(np.int32)
        assert degs.size >= 20 and ctx.info()["has_ties"] == 0
        ref = ctx.ref_mask()
        sc = ctx.sample_counts(degs, "reversed")                                 # partner_mask=None: the reference set of the tallies
        assert np.array_equal(sc.n_sel, (result[degs, 2 + N13] + result[degs, 2 + N31]).astype(np.int32))
        same(sc, scc.expected_counts(X, lambda i: ctx.get_codes(i, i + 1, 0, G)[0], degs, 0x44, ref))
        assert (sc.n_eq == 0).all()
        ss = ctx.sample_scores(degs)
        assert np.array_equal(ss.n_pairs, sc.n_sel) and ss.net.dtype == np.int32 and ss.net.shape == (degs.size, S)
        assert np.array_equal(ss.treat_like + ss.ctrl_like + ss.tied, np.broadcast_to(ss.n_pairs[:, None], (degs.size, S)))
        thr_rest = int(ctx.get_thresholds()[1, 0])
        assert (ss.treat_like[:, gid != 0].sum(axis=1) >= ss.n_pairs.astype(np.int64) * thr_rest).all()   # what n13 and n31 mean
        assert ss.n_pairs.sum() > 0
        assert np.array_equal(ctx.ref_mask(), ref)                               # the call outdates nothing
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == (iters, trace) and np.array_equal(again[0], result, equal_nan=True)
    args = (X, group, names, 0.01, 1.0, 0.05, ref0, 8, 1)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    off = pkg.run_identify_degs(*args, seed=seed, device=0, sample_scores=False)
    on = pkg.run_identify_degs(*args, seed=seed, device=0, sample_scores=True)
    assert set(plain.comparisons[0]) == TODAY == set(off.comparisons[0]) and set(on.comparisons[0]) == TODAY | {"sample_scores"}
    for r in (off, on):
        assert np.array_equal(r.result, plain.result, equal_nan=True) and r.trace == plain.trace and np.array_equal(r.result, result, equal_nan=True)
    got = on.comparisons[0]["sample_scores"]
    for f in ("genes", "n_pairs", "treat_like", "ctrl_like", "tied"):
        assert np.array_equal(getattr(got, f), getattr(ss, f)), f
    assert np.array_equal(got.net, ss.net)


def test_no_degs_gives_an_empty_object(pkg):
    G, S, seed = 60, 8, 2
    X = np.random.default_rng(seed).integers(0, 3, size=(G, S)).astype(np.int64)   # noise only
    run = pkg.run_identify_degs(X, halves(S), [f"g{i}" for i in range(G)], 0.01, 1.0, 1e-9, np.ones(G, dtype=bool), 3, 1, seed=seed, device=0,
                                sample_scores=True)
    ss = run.comparisons[0]["sample_scores"]
    assert (run.labels == "no change").all() and ss.genes.size == 0 and ss.net.shape == (0, S) and ss.n_pairs.size == 0


def test_every_refusal_has_its_message(pkg, monkeypatch):
    G, S = 70, 10
    labels = halves(S)
    X = tie_rich(G, S, 5, labels == "g1")
    q = np.arange(G, dtype=np.int32)
    ones = np.ones(G, dtype=np.uint8)
    n_sel, n_gt = np.zeros(G, dtype=np.int32), np.full((G, S), -7, dtype=np.int32)
    E = pkg._ffi.REO_EINVAL
    with open_ctx(pkg, X, labels) as ctx:
        msgs = []
        P = pkg._ffi._ptr

        def raw(genes, n, mask, pm, gt):                                         # the entry itself: a null pointer and a count are separate things
            pkg._ffi.check(ctx._L.reo_sample_counts(ctx._h, None if genes is None else P(genes), n, None if pm is None else P(pm), mask,
                                                    P(n_sel), None if gt is None else P(gt), None))

        for args, pattern in (((None, G, 0x44, ones, n_gt), "genes and n_gt must not be null"), ((q, G, 0x44, ones, None), "genes and n_gt must not be null"),
                              ((q, 0, 0x44, ones, n_gt), "n_genes = 0"), ((q, -3, 0x44, ones, n_gt), "n_genes = -3"),
                              ((q, (1 << 30) + 1, 0x44, ones, n_gt), r"n_genes = 1073741825.*2\^30"),
                              ((np.array([0, G], dtype=np.int32), 2, 0x44, ones, n_gt), rf"genes\[1\] = {G} is outside \[0, {G}\)"),
                              ((np.array([-1], dtype=np.int32), 1, 0x44, ones, n_gt), r"genes\[0\] = -1"),
                              ((q, G, 0, ones, n_gt), "no class"), ((q, G, 0x200, ones, n_gt), "bits above 8"),
                              ((q, G, 0x44, None, n_gt), "partner_mask is null.*reo_identify_degs")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                raw(*args)
            assert e.value.status == E and "reo_sample_counts" in e.value.message
            msgs.append(e.value.message)
        assert len(set(msgs)) == 9, msgs
        assert (n_gt == -7).all()                                                # a refused call writes nothing
        ctx.sample_counts_raw(q, 0x44, ones, None, n_gt, None)                    # n_sel and n_eq are optional
        assert (n_gt >= 0).all()
        ctx.identify_degs(np.ones(G, dtype=bool), 1.0, 0.05, 2, 1)
        assert ctx.sample_counts(q, 0x44).n_gt.shape == (G, S)                    # now there is a reference set
        ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="partner_mask is null.*reo_tally"):
            ctx.sample_counts(q, 0x44)
        ctx.sample_counts(q, 0x44, ones)                                          # an explicit mask still works
    with pkg.Context(device=0, seed=1) as ctx:                                   # no table built
        ctx.G, ctx.S = G, S
        with pytest.raises(pkg.DimensionMismatch, match="no class table"):
            ctx.sample_counts(q, 0x44, ones)
    with pkg.Context(device=0, seed=3) as ctx:                                   # a shard's part of the table: as reo_tally
        gid, lev = pkg.encode_groups(labels)
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.1); ctx.set_shard(0, 2); ctx.set_matrix(X)
        ctx.build_pairs(0)
        with pytest.raises(pkg.ReoError) as t:
            ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.ReoError) as e:
            ctx.sample_counts(q, ALL, ones)
        assert e.value.status == t.value.status == pkg._ffi.REO_ECOMM and e.value.message == t.value.message
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_sample_counts is not available on a reo_create_multi context"):
            ctx.sample_counts(q, 0x44, ones)


def test_cells_to_degs_with_sample_scores(pkg):
    seed, G, C = 8, 150, 240
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.integers(1, 30, size=(G, 1)).astype(float), size=(G, C)).astype(np.int64)
    X[: G // 6, C // 2:] *= 3
    X[G // 6: G // 3, : C // 2] *= 3
    labels = ["a"] * (C // 2) + ["b"] * (C - C // 2)
    args = (X, labels, [f"gene{i}" for i in range(G)], 8, 0.01, 1.0, 0.3, np.arange(G) >= G // 3, 8, 1)
    plain = pkg.identify_degs_cells(*args, seed=seed, device=0)
    got = pkg.identify_degs_cells(*args, seed=seed, device=0, sample_scores=True)
    cm = got.run.comparisons[0]
    assert set(plain.run.comparisons[0]) == TODAY and set(cm) == TODAY | {"sample_scores"}
    assert np.array_equal(cm["result"], plain.run.result, equal_nan=True)
    degs = np.flatnonzero(cm["labels"] != "no change")
    ss = cm["sample_scores"]
    assert degs.size > 0 and np.array_equal(ss.genes, degs) and ss.net.shape == (degs.size, got.run.info["S"])
    assert np.array_equal(ss.n_pairs, (cm["result"][degs, 2 + N13] + cm["result"][degs, 2 + N31]).astype(np.int32))


def test_reoa_writes_a_sample_scores_file(pkg, tmp_path):
    """reoa(use_testdata="yes", sample_scores=True): <stem>_<fg_name>_sample_scores.tsv beside the result files, one row per DEG"""
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path), seed=0x5EED0001, device=0, sample_scores=True)
    run = df.attrs["run"]
    cm = run.comparisons[0]
    ss = cm["sample_scores"]
    degs = np.flatnonzero(cm["labels"] != "no change")
    assert np.array_equal(ss.genes, degs)
    lines = (tmp_path / "fn_expr_group1_group2_sample_scores.tsv").read_text().split("\n")
    head = lines[0].split("\t")
    assert head[:2] == ["gene", "n_pairs"] and len(head) == 2 + ss.net.shape[1] and lines[-1] == "" and len(lines) == degs.size + 2
    if degs.size:
        assert lines[1].split("\t") == [run.gene_names[int(degs[0])], str(int(ss.n_pairs[0]))] + [str(int(v)) for v in ss.net[0]]
    assert not (tmp_path / "fn_expr_group1_group2_pairs.tsv").exists()
