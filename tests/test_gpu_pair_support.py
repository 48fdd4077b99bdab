"""Pair support on the GPU (reo_pair_support; csrc/pairsupport.hip): per listed pair and group, in how many samples the row's gene lies above
its partner and in how many the two are tied, and the outcome of every single sample.  The expected values come from the numpy restatement
of the comparators (tests/sample_counts_cases.py, sample_states) summed per group; where the library can say the same thing another way
(reo_pair_counts, reo_sample_counts, the class table and its thresholds) that is asserted too.  Every comparison is exact."""
import numpy as np
import pytest

import float32_cases as fc
from query_cases import band_matrix, halves, planted_ranks, tie_rich
import sample_counts_cases as scc

pytestmark = pytest.mark.gpu

ALL = 0x1FF
N13, N31 = 2, 6
TODAY = {"k", "result", "labels", "iters_run", "trace"}


def open_plain(pkg, X, labels, seed=11, matrix_first=False):
    """matrix and groups, nothing else: no thresholds, no class table"""
    ctx = pkg.Context(device=0, seed=seed)
    gid, lev = pkg.encode_groups(labels)
    if matrix_first:
        ctx.set_matrix(X)
    ctx.set_groups(gid, len(lev))
    if not matrix_first:
        ctx.set_matrix(X)
    return ctx


def make_csr(rng, G, lengths, genes=None, distinct=False):
    """a CSR with rows of the given lengths: genes drawn with repeats unless given, partners unsorted, drawn with repeats unless distinct"""
    genes = rng.integers(0, G, size=len(lengths)) if genes is None else np.asarray(genes)
    parts = [rng.choice(np.delete(np.arange(G), int(i)), size=n, replace=not distinct) for i, n in zip(genes, lengths)]
    rowptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return genes.astype(np.int32), rowptr, (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)


def expected(X, gid, ngroups, genes, rowptr, partner):
    """(n_gt, n_eq, outcome) by numpy: int32 entries x ngroups twice, uint8 entries x S; X in the arithmetic the library compares in"""
    X = np.asarray(X)
    ug = np.unique(genes)
    gt, eq = scc.states(X, ug)                                                   # unique genes x G x S
    at = np.searchsorted(ug, np.repeat(genes, np.diff(rowptr)))
    egt, eeq = gt[at, partner, :], eq[at, partner, :]
    assert not (egt & eeq).any()
    n_gt = np.stack([egt[:, gid == g].sum(axis=1) for g in range(ngroups)], axis=1).astype(np.int32)
    n_eq = np.stack([eeq[:, gid == g].sum(axis=1) for g in range(ngroups)], axis=1).astype(np.int32)
    return n_gt.reshape(-1, ngroups), n_eq.reshape(-1, ngroups), (2 * egt + eeq).astype(np.uint8)


def check(ctx, X, gid, csr, pkg, ties=True, outcomes=False, tag=None, exp=None):
    ng = int(gid.max()) + 1
    exp = exp if exp is not None else expected(X, gid, ng, *csr)
    ps = ctx.pair_support(csr, ties=ties, outcomes=outcomes)
    assert isinstance(ps, pkg.PairSupport) and ps.code is None, tag
    for got, want in zip((ps.genes, ps.rowptr, ps.partner), csr):
        assert np.array_equal(got, want), tag
    assert ps.n_gt.dtype == np.int32 and ps.n_gt.shape == exp[0].shape and np.array_equal(ps.n_gt, exp[0]), tag
    assert ps.group_sizes.tolist() == np.bincount(gid, minlength=ng).tolist(), tag
    if ties:
        assert ps.n_eq.dtype == np.int32 and np.array_equal(ps.n_eq, exp[1]), tag
        assert ps.n_lt.min(initial=0) >= 0, tag
    else:
        assert ps.n_eq is None, tag
    if outcomes:
        assert ps.outcome.dtype == np.uint8 and ps.outcome.shape == exp[2].shape and np.array_equal(ps.outcome, exp[2]), tag
        for g in range(ng):                                                      # the outcomes of a group's samples sum to its counts
            assert np.array_equal((ps.outcome[:, gid == g] == 2).sum(axis=1), ps.n_gt[:, g]), (tag, g)
            assert np.array_equal((ps.outcome[:, gid == g] == 1).sum(axis=1), exp[1][:, g]), (tag, g)
    else:
        assert ps.outcome is None, tag
    return ps, exp


@pytest.mark.parametrize("G", [33, 64, 65, 127, 200])
def test_small_layout_lane_and_word_seams(pkg, G):
    """S = 10 (5 + 5): one block per group, 27 padding slots each.  Rows of 0, 1, 63, 64 and 65 entries (one, one, one and two work items)
    with empty rows between them, genes and partners repeated and unsorted; G = 200 adds a row of 129 distinct partners (three items)."""
    S, seed = 10, 5
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, labels == "g1")
    rng = np.random.default_rng(seed + G)
    lengths = [0, 65, 0, 0, 1, 64, 63, 0, 2, 0]
    genes = rng.integers(0, G, size=len(lengths))
    genes[[1, 5]] = G - 1                                                        # the last gene, twice: every entry is its own row
    genes[6] = 0
    csr = make_csr(rng, G, lengths, genes)
    if G >= 130:
        more = make_csr(rng, G, [129, 0, 128], [G - 2, 3, 31], distinct=True)
        csr = (np.concatenate([csr[0], more[0]]), np.concatenate([csr[1], csr[1][-1] + more[1][1:]]), np.concatenate([csr[2], more[2]]))
    with open_plain(pkg, X, labels) as ctx:
        ps, exp = check(ctx, X, gid, csr, pkg, tag=G)
        assert exp[0].sum() > 0 and exp[1].sum() > 0 and (exp[0] + exp[1] < 5).any()   # greater, tied and smaller all occur
        gt16, eq16 = ctx.pair_counts(0, G, 0, G)                                 # the dense parity hook, entry by entry
        rows = ps.entry_genes
        assert np.array_equal(ps.n_gt, gt16[rows, ps.partner, :].astype(np.int32)) and np.array_equal(ps.n_eq, eq16[rows, ps.partner, :].astype(np.int32))
        no_ties, _ = check(ctx, X, gid, csr, pkg, ties=False, exp=exp)
        assert np.array_equal(no_ties.n_gt, ps.n_gt)
        check(ctx, X, gid, csr, pkg, ties=False, outcomes=True, exp=exp)          # outcomes need the le chain without the tied counts too
        one = (np.array([G - 1], dtype=np.int32), np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32))
        check(ctx, X, gid, one, pkg, outcomes=True)                              # one row, one entry
        none = (csr[0], np.zeros(csr[0].size + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
        ps0, _ = check(ctx, X, gid, none, pkg, outcomes=True)                     # rows without entries: REO_OK, nothing listed
        assert ps0.n_gt.shape == (0, 2) and ps0.outcome.shape == (0, S)
        # a PairList goes in as it is and keeps its codes
        pl = pkg.PairList(csr[0], csr[1], csr[2], np.full(csr[2].size, 4, dtype=np.uint8))
        from_list = ctx.pair_support(pl)
        assert np.array_equal(from_list.code, pl.code) and np.array_equal(from_list.n_gt, ps.n_gt) and np.array_equal(from_list.n_eq, ps.n_eq)


def test_three_unbalanced_groups(pkg):
    """7 / 40 / 23 samples in a shuffled order: counts for every group, in reo_set_groups order"""
    G, S, seed = 90, 70, 41
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.array(["u"] * 7 + ["v"] * 40 + ["w"] * 23, dtype=object))
    gid, lev = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, gid == 2)
    csr = make_csr(rng, G, [70, 0, 5, 89], distinct=True)
    with open_plain(pkg, X, labels) as ctx:
        ps, exp = check(ctx, X, gid, csr, pkg, outcomes=True)
        assert ps.group_sizes.tolist() == [int((gid == g).sum()) for g in range(3)] and sorted(ps.group_sizes.tolist()) == [7, 23, 40]
        assert all(exp[0][:, g].max() > 0 and exp[1][:, g].max() > 0 for g in range(3))
        gt16, eq16 = ctx.pair_counts(0, G, 0, G)
        assert np.array_equal(ps.n_gt, gt16[ps.entry_genes, ps.partner, :].astype(np.int32))
        assert np.array_equal(ps.n_eq, eq16[ps.entry_genes, ps.partner, :].astype(np.int32))
        d = ps.delta(2)                                                          # group 2 against everything else, from the counts
        rest = exp[0][:, 0] + exp[0][:, 1]
        assert np.array_equal(d, exp[0][:, 2] / float(ps.group_sizes[2]) - rest / float(ps.group_sizes[0] + ps.group_sizes[1]))


def test_groups_of_31_32_and_33_samples_interleaved(pkg):
    """block tails: a group that ends one slot before, at, and one slot after a block of 32; labels a b c a b c ..."""
    G, seed = 70, 19
    labels = np.array((["a", "b", "c"] * 31) + ["b", "c", "c"], dtype=object)
    S = labels.size
    gid, _ = pkg.encode_groups(labels)
    assert np.bincount(gid).tolist() == [31, 32, 33]
    X = tie_rich(G, S, seed, gid == 1)
    X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)
    rng = np.random.default_rng(seed)
    with open_plain(pkg, X, labels) as ctx:
        check(ctx, X, gid, make_csr(rng, G, [64, 3, 0, 40]), pkg, outcomes=True)


def test_outcomes_in_the_callers_column_order(pkg, monkeypatch):
    """G = 127, S = 70, labels a b a b ...: the slot map is not the identity, a has 33 samples (two blocks, 31 pads), b 37 (27 pads); every
    sample has a pattern of its own.  The outcomes against numpy, against the counts, and -- summed over the partners that reo_pair_list
    lists for a row -- against reo_sample_counts.  Cells the kernel must not write keep their sentinel."""
    G, S, seed = 127, 70, 9
    labels = np.array(["a" if (s % 2 == 0 and s < 66) else "b" for s in range(S)], dtype=object)
    gid, _ = pkg.encode_groups(labels)
    assert (gid == 0).sum() == 33 and (gid == 1).sum() == 37
    X = tie_rich(G, S, seed, labels == "b")
    X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)
    rng = np.random.default_rng(seed)
    csr = make_csr(rng, G, [126, 0, 65, 7], [0, 5, G - 1, 64], distinct=True)
    with open_plain(pkg, X, labels) as ctx:
        ps, exp = check(ctx, X, gid, csr, pkg, outcomes=True)
        assert len({tuple(c) for c in exp[2].T.tolist()}) > S // 2              # the columns differ: their order is checked
        assert set(np.unique(ps.outcome).tolist()) == {0, 1, 2}
        # the same question through the class table: a pair_list row and its sample counts
        ctx.compute_thresholds(0.05)
        ctx.build_pairs(0)
        q = np.array([0, 31, 64, G - 1], dtype=np.int32)
        pm = rng.random(G) < 0.7
        for classes in (ALL, "reversed"):
            pl = ctx.pair_list(q, classes, pm)
            sup = ctx.pair_support(pl, outcomes=True)
            sc = ctx.sample_counts(q, classes, pm)
            assert np.array_equal(sup.code, pl.code) and int(pl.rowptr[-1]) > 0
            for r in range(q.size):
                a, b = int(pl.rowptr[r]), int(pl.rowptr[r + 1])
                assert np.array_equal((sup.outcome[a:b] == 2).sum(axis=0), sc.n_gt[r]), (classes, r)
                assert np.array_equal((sup.outcome[a:b] == 1).sum(axis=0), sc.n_eq[r]), (classes, r)
        # the raw entry: guard bytes behind the outcome rows stay as they were, and a refused call writes nothing at all
        P = pkg._ffi._ptr
        n = csr[2].size
        n_gt, n_eq = np.full((n, 2), -7, dtype=np.int32), np.full((n, 2), -7, dtype=np.int32)
        out = np.full(n * S + 256, 0xAB, dtype=np.uint8)
        pkg._ffi.check(ctx._L.reo_pair_support(ctx._h, P(csr[0]), csr[0].size, P(csr[1]), P(csr[2]), P(n_gt), P(n_eq), P(out)))
        assert np.array_equal(out[: n * S].reshape(n, S), exp[2]) and (out[n * S:] == 0xAB).all()
        assert np.array_equal(n_gt, exp[0]) and np.array_equal(n_eq, exp[1])
        monkeypatch.setenv("REO_PAIR_SUPPORT_BATCH", "50")                         # the guard again with a batch cut inside every long row
        out[:] = 0xAB
        pkg._ffi.check(ctx._L.reo_pair_support(ctx._h, P(csr[0]), csr[0].size, P(csr[1]), P(csr[2]), P(n_gt), None, P(out)))
        assert np.array_equal(out[: n * S].reshape(n, S), exp[2]) and (out[n * S:] == 0xAB).all()
        monkeypatch.delenv("REO_PAIR_SUPPORT_BATCH")
        bad = csr[2].copy()
        bad[-1] = csr[0][-1]                                                     # the very last entry is the diagonal: everything before it is fine
        n_gt[:] = -7; n_eq[:] = -7; out[:] = 0xAB
        with pytest.raises(pkg.DimensionMismatch, match="own row 3"):
            pkg._ffi.check(ctx._L.reo_pair_support(ctx._h, P(csr[0]), csr[0].size, P(csr[1]), P(bad), P(n_gt), P(n_eq), P(out)))
        assert (n_gt == -7).all() and (n_eq == -7).all() and (out == 0xAB).all()


def class_codes(n_gt, sizes, thr, k=0):
    """the class of every entry by the rule of src/RankCompV3.jl:376-377, from the counts of a tie-free matrix: nre = the count in group k,
    not = the count in all other samples; code = 3 (ic - 1) + (it - 1)"""
    nre = n_gt[:, k].astype(np.int64)
    rest = n_gt.sum(axis=1, dtype=np.int64) - nre
    gsi1, gsi2 = int(sizes[k]), int(sizes.sum() - sizes[k])
    ic = np.where(nre >= thr[0, k], 3, np.where(gsi1 - nre >= thr[0, k], 1, 2))
    it = np.where(rest >= thr[1, k], 3, np.where(gsi2 - rest >= thr[1, k], 1, 2))
    return (3 * (ic - 1) + (it - 1)).astype(np.uint8)


def test_against_the_class_table_after_a_real_identify_degs(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    names = [f"g{i}" for i in range(G)]
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); thr = ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        degs = np.flatnonzero(pkg.label_genes(result, 1.0, 0.05) != "no change").astype(np.int32)
        assert degs.size >= 20 and ctx.info()["has_ties"] == 0
        ref = ctx.ref_mask()
        pl = ctx.pair_list(degs, ALL)
        assert int(pl.rowptr[-1]) > 1000 and len(set(pl.code.tolist())) >= 4
        ps = ctx.pair_support(pl)
        assert (ps.n_eq == 0).all() and ps.group_sizes.tolist() == np.bincount(gid).tolist()
        assert np.array_equal(class_codes(ps.n_gt, ps.group_sizes, thr), pl.code)  # the class of every listed pair, recomputed from its support
        d = ps.delta()
        assert (pl.code == N13).any() and (pl.code == N31).any()
        assert (d[pl.code == N13] < 0).all() and (d[pl.code == N31] > 0).all()   # n13: below the partner in the control, above it in the rest
        top = ps.top(5)
        assert np.array_equal(np.abs(d[top]), np.sort(np.abs(d))[::-1][:5])
        assert np.array_equal(ctx.ref_mask(), ref)                               # the call outdates nothing
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == (iters, trace) and np.array_equal(again[0], result, equal_nan=True)
        rev = ctx.pair_list(degs, "reversed")
        sup_rev = ctx.pair_support(rev)
    with open_plain(pkg, X, group, seed=seed) as fresh:                          # no thresholds, no build_pairs: the transform alone
        first = fresh.pair_support(pl, outcomes=True)
        assert np.array_equal(first.n_gt, ps.n_gt) and np.array_equal(first.n_eq, ps.n_eq)
        for g in range(2):
            assert np.array_equal((first.outcome[:, gid == g] == 2).sum(axis=1), ps.n_gt[:, g])
    args = (X, group, names, 0.01, 1.0, 0.05, ref0, 8, 1)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    off = pkg.run_identify_degs(*args, seed=seed, device=0, pairs="reversed")
    on = pkg.run_identify_degs(*args, seed=seed, device=0, pairs="reversed", pair_support=True)
    assert set(plain.comparisons[0]) == TODAY and set(off.comparisons[0]) == TODAY | {"ref_mask", "pairs"}
    assert set(on.comparisons[0]) == TODAY | {"ref_mask", "pairs", "pair_support"}
    for r in (off, on):
        assert np.array_equal(r.result, plain.result, equal_nan=True) and r.trace == plain.trace and np.array_equal(r.result, result, equal_nan=True)
    for f in ("genes", "rowptr", "partner", "code"):
        assert np.array_equal(getattr(on.comparisons[0]["pairs"], f), getattr(off.comparisons[0]["pairs"], f)), f
        assert np.array_equal(getattr(on.comparisons[0]["pair_support"], f), getattr(rev, f)), f
    got = on.comparisons[0]["pair_support"]
    assert np.array_equal(got.n_gt, sup_rev.n_gt) and np.array_equal(got.n_eq, sup_rev.n_eq) and got.outcome is None
    assert np.array_equal(on.comparisons[0]["ref_mask"], off.comparisons[0]["ref_mask"])


def test_no_degs_gives_an_empty_object(pkg):
    G, S, seed = 60, 8, 2
    X = np.random.default_rng(seed).integers(0, 3, size=(G, S)).astype(np.int64)   # noise only
    run = pkg.run_identify_degs(X, halves(S), [f"g{i}" for i in range(G)], 0.01, 1.0, 1e-9, np.ones(G, dtype=bool), 3, 1, seed=seed, device=0,
                                pairs="reversed", pair_support=True)
    ps = run.comparisons[0]["pair_support"]
    assert (run.labels == "no change").all() and ps.genes.size == 0 and ps.n_gt.shape == (0, 2) and ps.n_eq.shape == (0, 2)
    assert ps.group_sizes.tolist() == [4, 4] and ps.top(3).size == 0


def test_after_a_slot_order_build_the_gene_order_planes_are_intact(pkg):
    G, S, seed = 70, 12, 21
    rng = np.random.default_rng(seed)
    X = rng.permuted(np.tile(3.0 * np.arange(G)[:, None], (1, S)), axis=0)      # tie-free Float64: every sample a permutation of 0, 3, 6, ...
    X[: G // 5, S // 2:] += 60.5                                                # (shifted genes stay 0.5 away from everything else)
    X = np.asfortranarray(X)
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    with open_plain(pkg, X, labels, matrix_first=True) as ctx:                   # (groups first would pair the sides as they arrive: identity order)
        ctx.compute_thresholds(0.1)
        ctx.build_pairs(0)
        assert ctx.info()["k1_slot_order"] == 1 and ctx.info()["has_ties"] == 0
        ps, _ = check(ctx, X, gid, make_csr(rng, G, [69, 10, 0, 64], distinct=True), pkg, outcomes=True)
        assert (ps.n_eq == 0).all()


def all_pairs(G):
    """every ordered pair off the diagonal as a CSR"""
    genes = np.arange(G, dtype=np.int32)
    partner = np.concatenate([np.delete(np.arange(G), i) for i in range(G)]).astype(np.int32)
    return genes, (np.arange(G + 1, dtype=np.int64) * (G - 1)), partner


def test_float64_band(pkg):
    G, S, seed = 70, 12, 3
    X = band_matrix(G, S, seed)
    tied = [scc.sample_states(X[:, s], 2 * k)[1][2 * k + 1] for s in range(S) for k in range(5)]
    assert any(tied) and not all(tied)                                           # planted pairs fall on both sides of the band
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    with open_plain(pkg, X, labels) as ctx:
        ps, exp = check(ctx, X, gid, all_pairs(G), pkg, outcomes=True)           # the planted pairs (2k, 2k + 1) from both sides among them
        assert exp[1].sum() > 0
        at = [int(ps.rowptr[2 * k]) + 2 * k for k in range(5)]                    # entry (2k, 2k + 1): the partner list of row 2k skips 2k itself
        assert ps.partner[at].tolist() == [1, 3, 5, 7, 9] and np.array_equal(ps.outcome[at] == 1, np.array(tied).reshape(S, 5).T)


def test_float32_rule_on_planted_flip_pairs(pkg):
    G, S, seed = 60, 12, 13
    X = fc.planted(G, S, 4, seed)
    assert X.dtype == np.float32 and fc.disagreements(X)[0] >= 4 * S
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    csr = all_pairs(G)
    with open_plain(pkg, np.asfortranarray(X), labels) as ctx:
        assert ctx.info()["resident_dtype"] == 3
        ps, exp = check(ctx, X, gid, csr, pkg, outcomes=True)
        widened = expected(X.astype(np.float64), gid, 2, *csr)
        assert not np.array_equal(widened[1], exp[1]) and not np.array_equal(widened[2], exp[2])   # the Float64 rule would call other pairs tied


def test_int32_equals_int64(pkg):
    G, S, seed = 65, 10, 23
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, labels == "g1")
    csr = make_csr(np.random.default_rng(seed), G, [64, 64, 1, 30])
    out = []
    for Xt in (X, X.astype(np.int32)):
        with open_plain(pkg, np.asfortranarray(Xt), labels) as ctx:
            out.append(check(ctx, X, gid, csr, pkg, outcomes=True)[0])
    assert np.array_equal(out[0].n_gt, out[1].n_gt) and np.array_equal(out[0].n_eq, out[1].n_eq) and np.array_equal(out[0].outcome, out[1].outcome)


def test_infinities(pkg):
    """+-Inf, two equal infinities in one sample included: the larger index is the greater one, nothing is tied"""
    G, S, seed = 80, 12, 31
    X = pkg.synth.with_infinities(pkg.synth.float_expr(G, S, seed), seed, "log0")
    X[3, 0] = X[7, 0] = np.inf
    X[5, 1] = X[9, 1] = -np.inf
    X[11, 2], X[12, 2] = np.inf, -np.inf
    X = np.asfortranarray(X)
    assert np.isinf(X).sum() > 2 * S
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    with open_plain(pkg, X, labels) as ctx:
        ps, exp = check(ctx, X, gid, all_pairs(G), pkg, outcomes=True)
        o = {(int(i), int(j)): ps.outcome[e] for e, (i, j) in enumerate(zip(ps.entry_genes, ps.partner)) if (int(i), int(j)) in
             {(3, 7), (7, 3), (5, 9), (9, 5), (11, 12), (12, 11)}}
        assert (o[(3, 7)][0], o[(7, 3)][0]) == (0, 2) and (o[(5, 9)][1], o[(9, 5)][1]) == (0, 2) and (o[(11, 12)][2], o[(12, 11)][2]) == (2, 0)


def big_case(pkg, G, genes, marks, seed, X=None):
    """X: Int64 levels below 200 unless given, and a given matrix is tie-free"""
    S = 8
    rng = np.random.default_rng(seed)
    tie_free = X is not None
    if X is None:
        X = np.asfortranarray(rng.integers(0, 200, size=(G, S)).astype(np.int64))   # (one comparison in 200 is a tie: a few dozen among the listed pairs)
    labels = np.array(["a", "b"] * (S // 2), dtype=object)
    gid, _ = pkg.encode_groups(labels)
    genes = np.asarray(genes)
    parts = []
    for i in genes:
        p = np.concatenate([np.asarray(marks), rng.choice(G, 70, replace=False)])
        parts.append(rng.permutation(p[p != i]))
    rowptr = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    csr = (genes.astype(np.int32), rowptr, np.concatenate(parts).astype(np.int32))
    with open_plain(pkg, X, labels) as ctx:                                      # no table is built: only the transform runs
        ps, exp = check(ctx, X, gid, csr, pkg, outcomes=True)
        assert exp[0].sum() > 0 and (exp[1].sum() == 0 if tie_free else exp[1].sum() > 0) and (exp[2] == 0).any()
        check(ctx, X, gid, csr, pkg, ties=False, exp=exp)


def test_17_plane_layout(pkg):
    """G = 65 600: five pos quads, edge rows of eight uint4, plane k in word k; genes and partners either side of 65 536"""
    big_case(pkg, 65600, [65599, 0, 40000, 65535, 65536], [0, 4095, 4096, 65535, 65536, 65599], 61)


def test_18_plane_layout(pkg):
    """G = 131 584: the eighteenth plane; a dozen rows, genes and partners either side of 65 536 and of 131 072"""
    big_case(pkg, 131584, [131583, 0, 65535, 65536, 131071, 131072, 100000, 7, 131073, 99, 131000, 70000],
             [0, 65535, 65536, 131071, 131072, 131583], 67)


def test_batch_seam(pkg, monkeypatch):
    """REO_PAIR_SUPPORT_BATCH = 1, 3 and 100 against the unbatched call: cuts inside rows and at row ends, empty rows at the cut, with outcomes"""
    G, S, seed = 150, 40, 77
    labels = halves(S)
    gid, _ = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, labels == "g1")
    rng = np.random.default_rng(seed)
    csr = make_csr(rng, G, [0, 129, 0, 0, 64, 7, 100, 0, 3, 0])
    with open_plain(pkg, X, labels) as ctx:
        whole, exp = check(ctx, X, gid, csr, pkg, outcomes=True)
        for batch in ("1", "3", "100"):
            monkeypatch.setenv("REO_PAIR_SUPPORT_BATCH", batch)                    # (read per call)
            again, _ = check(ctx, X, gid, csr, pkg, outcomes=True, tag=batch, exp=exp)
            assert np.array_equal(again.n_gt, whole.n_gt) and np.array_equal(again.n_eq, whole.n_eq) and np.array_equal(again.outcome, whole.outcome)
            check(ctx, X, gid, csr, pkg, ties=False, tag=batch, exp=exp)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    G, S = 70, 10
    labels = halves(S)
    X = tie_rich(G, S, 5, labels == "g1")
    genes = np.array([4, 0, 69], dtype=np.int32)
    rowptr = np.array([0, 2, 2, 5], dtype=np.int64)
    partner = np.array([3, 0, 1, 1, 2], dtype=np.int32)
    n = partner.size
    n_gt, n_eq, out = np.full((n, 2), -7, dtype=np.int32), np.full((n, 2), -7, dtype=np.int32), np.full((n, S), 0xAB, dtype=np.uint8)
    E = pkg._ffi.REO_EINVAL
    P = pkg._ffi._ptr

    def arr(v, dtype):
        return np.array(v, dtype=dtype)

    with open_plain(pkg, X, labels) as ctx:
        def raw(g, ng, rp, pa, gt):                                              # the entry itself: a null pointer and a count are separate things
            pkg._ffi.check(ctx._L.reo_pair_support(ctx._h, None if g is None else P(g), ng, None if rp is None else P(rp),
                                                   None if pa is None else P(pa), None if gt is None else P(gt), P(n_eq), P(out)))

        msgs = []
        for args, pattern in (((None, 3, rowptr, partner, n_gt), "genes, rowptr and n_gt must not be null"),
                              ((genes, 3, None, partner, n_gt), "genes, rowptr and n_gt must not be null"),
                              ((genes, 3, rowptr, partner, None), "genes, rowptr and n_gt must not be null"),
                              ((genes, 0, rowptr, partner, n_gt), "n_genes = 0"), ((genes, -3, rowptr, partner, n_gt), "n_genes = -3"),
                              ((genes, (1 << 30) + 1, rowptr, partner, n_gt), r"n_genes = 1073741825.*2\^30"),
                              ((arr([4, G, 1], np.int32), 3, rowptr, partner, n_gt), rf"genes\[1\] = {G} is outside \[0, {G}\)"),
                              ((arr([-1, 0, 1], np.int32), 3, rowptr, partner, n_gt), r"genes\[0\] = -1"),
                              ((genes, 3, arr([1, 2, 2, 5], np.int64), partner, n_gt), r"rowptr\[0\] = 1"),
                              ((genes, 3, arr([0, 2, 1, 5], np.int64), partner, n_gt), "rowptr decreases at row 1"),
                              ((genes, 3, rowptr, None, n_gt), "partner is null and rowptr lists 5 entries"),
                              ((genes, 3, rowptr, arr([3, 0, 1, G, 2], np.int32), n_gt), rf"partner\[3\] = {G} \(row 2\) is outside \[0, {G}\)"),
                              ((genes, 3, rowptr, arr([3, -1, 1, 1, 2], np.int32), n_gt), r"partner\[1\] = -1 \(row 0\)"),
                              ((genes, 3, rowptr, arr([3, 0, 1, 1, 69], np.int32), n_gt), r"partner\[4\] = 69 is the gene of its own row 2.*diagonal")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                raw(*args)
            assert e.value.status == E and "reo_pair_support" in e.value.message
            msgs.append(e.value.message)
        assert len(set(msgs)) == len(msgs) - 2, msgs                             # (the three null pointers share one message)
        assert (n_gt == -7).all() and (n_eq == -7).all() and (out == 0xAB).all()  # a refused call writes nothing
        raw(genes, 3, arr([0, 0, 0, 0], np.int64), None, n_gt)                    # nothing listed: fine without partners, and nothing is written
        assert (n_gt == -7).all() and (n_eq == -7).all() and (out == 0xAB).all()
        pkg._ffi.check(ctx._L.reo_pair_support(ctx._h, P(genes), 3, P(rowptr), P(partner), P(n_gt), None, None))   # n_eq and outcome are optional
        assert (n_gt >= 0).all() and (n_eq == -7).all() and (out == 0xAB).all()
        with pytest.raises(pkg.DimensionMismatch, match="rowptr has 3 entries for 3 rows"):
            ctx.pair_support((genes, rowptr[:-1], partner))
        with pytest.raises(pkg.DimensionMismatch, match="rowptr lists 5 entries, partner has 4"):
            ctx.pair_support((genes, rowptr, partner[:-1]))
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.pair_support((genes, rowptr, partner))
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="no groups"):
            ctx.pair_support((genes, rowptr, partner))
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_pair_support is not available on a reo_create_multi context") as e:
            ctx.pair_support((genes, rowptr, partner))
        assert e.value.message not in msgs


def test_reoa_writes_a_pair_support_file(pkg, tmp_path):
    """reoa(use_testdata="yes", pairs="reversed", pair_support=True): <stem>_<fg_name>_pair_support.tsv beside the pairs file, one line per
    listed pair; without the option there is no such file"""
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "on"), seed=0x5EED0001, device=0, pairs="reversed", pair_support=True)
    run = df.attrs["run"]
    cm = run.comparisons[0]
    pl, ps = cm["pairs"], cm["pair_support"]
    for f in ("genes", "rowptr", "partner", "code"):
        assert np.array_equal(getattr(pl, f), getattr(ps, f)), f
    lines = (tmp_path / "on" / "fn_expr_group1_group2_pair_support.tsv").read_text().split("\n")
    lv = [str(v) for v in run.levels]
    assert lines[0].split("\t") == ["gene", "partner", "class"] + [f"{v}_{w}" for v in lv for w in ("gt", "eq")] and len(lv) == 2
    n = int(pl.rowptr[-1])
    assert lines[-1] == "" and len(lines) == n + 2
    if n:
        e = n - 1
        want = [run.gene_names[int(ps.entry_genes[e])], run.gene_names[int(ps.partner[e])], pkg._ffi.CLASS_NAMES[int(ps.code[e])]]
        assert lines[n].split("\t") == want + [str(int(v)) for v in (ps.n_gt[e, 0], ps.n_eq[e, 0], ps.n_gt[e, 1], ps.n_eq[e, 1])]
    pairs_file = (tmp_path / "on" / "fn_expr_group1_group2_pairs.tsv").read_bytes()
    pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "off"), seed=0x5EED0001, device=0, pairs="reversed")
    assert not (tmp_path / "off" / "fn_expr_group1_group2_pair_support.tsv").exists()
    assert (tmp_path / "off" / "fn_expr_group1_group2_pairs.tsv").read_bytes() == pairs_file   # the pairs file stays byte for byte
