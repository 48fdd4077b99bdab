"""tests/top_plane_cases.py without a GPU: the subset forms equal the whole-matrix restatements they stand for on small cases, the seeded
cases of tests/test_gpu_top_planes.py have what the kernels must meet -- ties on both sides, counts that a chain blind to the upper planes
gets wrong, equal |N| that Gamma orders and equal keys that (i, j) orders, maxima attained by several pairs -- and every comparison of
the GPU file fails on planted errors."""
import numpy as np
import pytest

import perm_null_cases as pnc
import plane_cases as pc
import top_pairs_cases as tpc
import top_pairs_loo_cases as lc
import top_pairs_null_cases as tnc
import top_partners_cases as tprc
import top_partners_null_cases as tpnc
import top_plane_cases as tc
import wide_sample_cases as wsc
import wide_top_pairs_cases as wt

HEAD = 256     # "the first pairs": with 12 / 9 samples up to a hundred pairs of planted genes are separated in every sample


# ---- the subset forms on small cases

SMALL_G, SMALL_SIDES = 150, (12, 9)


def small(kind):
    X, gid = tc.matrix(SMALL_G, kind, SMALL_SIDES, 0x5EED7B00 + tc.KINDS.index(kind))
    genes = np.array(sorted({0, 63, 64, SMALL_G - 1} | set(np.random.default_rng(3).choice(SMALL_G, 50, replace=False).tolist())), dtype=np.int64)
    return X, gid, genes


def same_oracle(x: tpc.Oracle, y: tpc.Oracle):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("gene_i", "gene_j", "counts", "num", "rank_num")) and x.sizes == y.sizes


@pytest.mark.parametrize("kind", tc.KINDS)
def test_subset_forms_equal_the_whole_matrix_restatements(kind):
    X, gid, genes = small(kind)
    G = X.shape[0]
    mask = tc.mask_of(genes, G)
    in_a, in_b = tprc.side_masks(gid, 2, 0, None)
    full = tpc.oracle(X, gid, 2, 0, None)
    W = tc.terms(X, np.arange(G))
    D = tc.shift_of(W, in_a, in_b)
    assert np.array_equal(D, full.D)                                             # the sort (Int64), the band predicate (Float64)
    if kind != "ties_f64":
        assert np.array_equal(W.sum(axis=0), np.zeros(X.shape[1], dtype=np.int64))   # every pair adds +1 and -1, or nothing
    assert (full.counts[:, 1::2].sum() > 0) == (kind != "ranks")
    assert same_oracle(tc.subset_oracle(X, gid, 2, 0, None, genes, D), tpc.oracle(X, gid, 2, 0, None, mask))
    rows = tc.label_rows(gid, 7, 5)
    assert rows.shape == (5, gid.size) and np.array_equal(rows[0], gid == 0) and (rows.sum(axis=1) == SMALL_SIDES[0]).all()
    assert (rows[1][gid == 1] == 1).all() and rows[1].sum() == SMALL_SIDES[0]   # inverted as far as the sizes allow
    cuts = np.array([0, 1, int(np.abs(full.num).max()), int(np.abs(full.num).max()) + 1])
    got, want = tc.subset_null(X, rows, cuts, genes), tnc.restate(X, rows, cuts, mask)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    n = tc.subset_abs(X, rows, genes)
    assert np.array_equal(n.max(axis=1), want.max_num) and np.array_equal((n >= cuts[2]).sum(axis=1), want.n_reach[:, 2])
    for q in (0, 63, G - 1):
        row = tprc.row_oracle(X, gid, 2, 0, None, D, q)
        assert tprc.same(row, tprc.from_pairs(full, q))
        for lo, hi in ((0, 64), (60, 130), (100, G)):
            chunk = np.zeros(G, dtype=bool)
            chunk[lo:hi] = True
            assert tprc.same(tc.cut_row(row, lo, hi), tprc.row_oracle(X, gid, 2, 0, None, D, q, chunk))
    q = np.array([0, 63, G - 1], dtype=np.int32)
    pcuts = np.array([0, 5, 50], dtype=np.int64)
    a, b = tpnc.query_restate(X, rows, q, pcuts), tpnc.restate(X, rows, q, pcuts)
    assert all(np.array_equal(u, v) for u, v in zip(a[:3], b[:3]))
    got = tc.subset_loo(X, gid, 2, 0, None, 3, genes, W, D)
    want = lc.restate_candidates(X, gid, 2, 0, None, 3, mask)
    assert lc.same(got, want) and (got.cut, got.n_candidates) == (want.cut, want.n_candidates)
    assert lc.same(got, lc.restate(X, gid, 2, 0, None, 3, mask))                 # and the route by candidates is the definition


def test_cases_gene_sets_and_chunks():
    assert len(tc.cases()) == 11 and set(G for G, _ in tc.cases()) == set(pc.PLANE_G + pc.PAD_G)
    forms = {(pc.plane_bits(G), kind != "ranks") for G, kind in tc.cases()}
    assert forms == {(p, t) for p in (12, 15, 16) for t in (False, True)} - {(12, True)}   # (4 095 genes: the tie-free form, as boundary_kind deals it)
    for G, kind in tc.cases():
        genes, q = tc.seam_genes(G, kind), tc.queries(G, kind)
        assert genes.size == tc.N_SEAM and (np.diff(genes) > 0).all() and genes[0] == 0 and genes[-1] == G - 1
        assert set(q.tolist()) <= set(genes.tolist()) and {0, 63, 64, G - 1} <= set(q.tolist()) and 6 <= q.size <= 10
        assert set(range(G - 40, G)) <= set(genes.tolist())
        for seam in (4096, 8192, 32768):
            assert {g for g in (seam - 1, seam) if g < G} <= set(genes.tolist())
        loo = tc.loo_genes(G, kind)
        assert set(loo.tolist()) <= set(genes.tolist()) and 100 <= loo.size <= tc.N_LOO and loo[-1] == G - 1
        ch = tc.chunks(G)
        assert ch[0][0] == 0 and ch[-1][1] == G and all(a[1] == b[0] for a, b in zip(ch, ch[1:])) and len(ch) == -(-G // 1024)
        X, gid = tc.case(G, kind)
        assert X.shape == (G, sum(pc.sides(G))) and X.dtype == (np.float64 if kind == "ties_f64" else np.int64) and X.flags.f_contiguous
        if kind == "ranks":
            assert all(np.array_equal(np.sort(X[:, s]), np.arange(G)) for s in range(X.shape[1]))
    assert len(tc.chunks(9000)) == 9 and len(tc.chunks(65535)) == 64


# ---- what the seeded cases hold

@pytest.mark.parametrize("G,kind", tc.cases())
def test_the_cases_hold_what_the_kernels_must_meet(G, kind):
    e = tc.expected(G, kind)
    o = e.top
    mag = np.abs(o.num)
    assert o.gene_i.size == tc.N_SEAM * (tc.N_SEAM - 1) // 2
    if kind != "ranks":                                                          # ties on both sides, among the pairs and in every row
        assert (o.counts[:, 1] > 0).sum() > 1000 and (o.counts[:, 3] > 0).sum() > 1000
        assert ((o.counts[:, 1] > 0) & (o.counts[:, 3] > 0)).any()
        assert all(r.counts[:, 1].any() and r.counts[:, 3].any() for r in e.rows_full)
    else:
        assert not o.counts[:, 1::2].any() and not any(r.counts[:, 1::2].any() for r in e.rows_full)
    assert len(np.unique(mag[:HEAD])) > 1 and mag[0] > 0                         # the head is not one plateau
    same_n = mag[1:] == mag[:-1]
    same_g = o.rank_num[1:] == o.rank_num[:-1]
    assert (same_n & ~same_g).any() and (same_n & same_g).any()                  # Gamma orders equal |N|; (i, j) orders equal keys
    at_max = (e.null_abs == e.null_abs.max(axis=1)[:, None]).sum(axis=1)
    assert (at_max[2:] > 1).any(), at_max                                        # a shuffled row whose maximum several pairs attain
    assert e.null.n_reach[0, 2] == at_max[0] and not e.null.n_reach[:, 3][0] and (e.null.n_reach[:, 0] == o.gene_i.size).all()
    assert len(set(e.null.max_num.tolist())) > 3
    assert e.pnull.n_multi > 0 and (e.pnull.max_num > 0).all()
    for r, row in enumerate(e.rows_full):
        assert row.partner.size == (tc.N_SEAM if kind == "ties_f64" else G) - 1
        if kind != "ties_f64":
            assert e.pnull.max_num[0, r] == abs(int(row.num[0])) and e.pnull.arg_partner[0, r] == row.partner[np.abs(row.num) == abs(int(row.num[0]))].min()


@pytest.mark.parametrize("G,kind", [c for c in tc.cases() if c[0] in pc.DEEP_G])
def test_the_deep_cases_change_under_truncated_ranks(G, kind):
    """a condition on the cases, as plane_cases.truncated_gt states it: the gt counts of the pairs inside the gene set and of every query
    row change when each sample's ranks lose the planes from 12 (and, at 65 535 genes, from 15) upwards"""
    X, gid = tc.case(G, kind)
    genes, q = tc.seam_genes(G, kind), tc.queries(G, kind)
    R = pc.sample_ranks(X)
    for bits in (12, 15) if G > 32767 else (12,):
        cut, true = tc.truncated_counts(X, gid, genes, genes, bits, R)
        changed = (cut != true).any(axis=-1)
        assert changed[np.triu_indices(genes.size, 1)].mean() >= 0.25, (G, kind, bits)
        cut, true = tc.truncated_counts(X, gid, q, np.arange(G), bits, R)
        assert ((cut != true).any(axis=-1).mean(axis=1) >= 0.25).all(), (G, kind, bits)
    if kind == "ranks":
        cut, true = tc.truncated_counts(X, gid, q, np.arange(G), 18, R)
        assert np.array_equal(cut, true)                                         # tie-free: comparing ranks is comparing values


def test_the_leave_one_out_cases():
    for G, kind in tc.loo_cases():
        want = tc.expected_loo(G, kind)
        assert want.cut > 0 and 0 < want.n_candidates < tc.N_LOO * (tc.N_LOO - 1) // 2 and (want.gene_i >= 0).all()
        assert len({tuple(r) for r in want.gene_i.tolist()}) > 1                 # the folds do not all pick alike
        if kind == "ties":
            assert (want.outcome == 0).any()                                     # a held-out sample tied on a pick


def test_the_cross_and_big_wide_layouts():
    """34 blocks in five chunks with a chunk seam inside each group; the batch seam of the all-genes call; more than 2 048 partners in one
    tile and a background the tails' tolerance is measured for; ranks above plane 11 in every query row; 17 planes on 10 blocks"""
    gid = tc.cross_gid()
    slots = pnc.slot_map(gid, 2)
    per_group = [-(-int(n) // 32) for n in np.bincount(gid)]
    assert gid.size == 1050 and sorted(np.bincount(gid).tolist()) == [520, 530] and per_group == [17, 17] and slots.size == 32 * tc.CROSS_BLOCKS
    chunks = tuple(min(wsc.CHUNK_BLOCKS, tc.CROSS_BLOCKS - b) for b in range(0, tc.CROSS_BLOCKS, wsc.CHUNK_BLOCKS))
    assert chunks == (8, 8, 8, 8, 2) and 17 % wsc.CHUNK_BLOCKS != 0              # the group seam lies inside the third chunk
    assert not np.array_equal(gid, np.sort(gid)) and np.array_equal(tc.labels_of(gid) == "a", gid == 0)
    assert tc.CROSS_BATCH == 7710 < tc.CROSS_G and (32 << 20) // (slots.size * 4) == tc.CROSS_BATCH
    rows = tc.cross_rows_checked()
    assert rows.size == 32 and {0, 4095, 4096, 7709, 7710, 8999} <= set(rows.tolist())
    pm = tc.cross_partner_mask(pc.query_marks(tc.CROSS_G))
    assert pm[:4096].sum() > 2048 and pm.sum() <= 4200 and pm[pc.query_marks(tc.CROSS_G)].all()
    X, _ = tc.cross_case("ties")
    q = pc.query_genes(tc.CROSS_G)
    assert X.dtype == np.int64 and X.shape == (tc.CROSS_G, 1050) and len({X[1::2, s].tobytes() for s in range(40)}) == 40
    cut, true = tc.truncated_counts(X, gid, q, np.arange(tc.CROSS_G), 12)
    assert ((cut != true).any(axis=-1).mean(axis=1) >= 0.25).all()
    assert set(tc.cross_loo_genes("ties").tolist()) <= set(tc.seam_genes(tc.CROSS_G, "ties").tolist()) and 36 <= tc.cross_loo_genes("ties").size <= tc.N_CROSS_LOO
    Xb, gb, pmb = tc.big_wide_case()
    assert Xb.shape == (65600, 265) and pc.padded(65600) == 66560 and wsc.blocks_of(tc.BIG_WIDE_LAYOUT)[1:] == (10, (8, 2))
    assert pmb[tc.BIG_WIDE_MARKS].all() and 194 <= pmb.sum() <= 200 and max(tc.BIG_WIDE_Q) == 65599 and (Xb[:20000, gb == 1].mean() - Xb[:20000, gb == 0].mean()) > 8000


def test_the_capacity_test_forces_refinement():
    """tp_select as wide_top_pairs_cases.select_passes models it, on the 44 850 pairs of the 9 000-gene case with ties: the whole list
    ends after one pass under any capacity (every pair is wanted), so the capacity test asks for the first 1 000 and 4 096 pairs; there the
    default capacity still ends after one pass and a capacity of n refines until exactly n keys are left -- through the digits of Gamma
    and of (i, j), since dozens of pairs share the |N| at the cut"""
    G = 9000
    o = tc.expected(G, "ties").top
    total = o.gene_i.size
    assert wt.select_passes(o, G, total, total) == (1, total)
    for n in tc.CAP_N:
        assert wt.default_capacity(n) > total > 4 * n
        wide, tight = wt.select_passes(o, G, n, wt.default_capacity(n)), wt.select_passes(o, G, n, n)
        assert wide[0] == 1 and wide[1] > n and tight[1] == n and tight[0] >= 3, (n, wide, tight)
        mag = np.abs(o.num)
        assert (mag == mag[n - 1]).sum() > 10 and mag[n - 1] == mag[n]           # the cut falls inside a run of equal |N| ...
        assert o.rank_num[n - 1] != o.rank_num[n] or (o.gene_i[n - 1], o.gene_j[n - 1]) != (o.gene_i[n], o.gene_j[n])


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_the_cross_case_holds_what_the_kernels_must_meet(kind):
    """the conditions of the cases above on `cross`, which has a matrix and label rows of its own.  Two of them cannot hold at 1 050
    samples and are asserted absent, so that nobody takes them for covered there: no two pairs share |N| and Gamma, and no shuffled
    row's maximum is attained twice -- those paths run at the sizes above."""
    e = tc.cross_expected(kind)
    o = e.top
    mag = np.abs(o.num)
    if kind == "ties":
        assert (o.counts[:, 1] > 0).sum() > 1000 and (o.counts[:, 3] > 0).sum() > 1000 and o.counts[:, 1::2].max() > 64
        assert all(r.counts[:, 1].any() and r.counts[:, 3].any() for r in e.rows_full)
    else:
        assert not o.counts[:, 1::2].any() and not any(r.counts[:, 1::2].any() for r in e.rows_full)
    assert o.counts.max() > 255 and len(np.unique(mag[:HEAD])) > 100               # counts past eight bits; a head of many |N|
    same_n = mag[1:] == mag[:-1]
    same_g = o.rank_num[1:] == o.rank_num[:-1]
    assert (same_n & ~same_g).sum() > 1000 and not (same_n & same_g).any()
    at_max = (e.null_abs == e.null_abs.max(axis=1)[:, None]).sum(axis=1)
    assert (at_max == 1).all() and e.pnull.n_multi == 0
    assert len(set(e.null.max_num.tolist())) > 10 and (e.pnull.max_num > 0).all() and e.null.n_reach[0, 2] == 1 and not e.null.n_reach[0, 3]
    for r, row in enumerate(e.rows_full):
        assert row.partner.size == tc.CROSS_G - 1 and e.pnull.max_num[0, r] == abs(int(row.num[0])) and e.pnull.arg_partner[0, r] == row.partner[0]
    loo = tc.cross_expected_loo(kind)
    assert loo.cut > 0 and 0 < loo.n_candidates < 780 and (loo.gene_i >= 0).all() and len({tuple(r) for r in loo.gene_i.tolist()}) > 1
    if kind == "ties":
        assert (loo.outcome == 0).any()                                          # a held-out sample tied on a pick


# ---- planted errors

def answers(X, gid, G, kind, rows=None, D_off=None):
    """what the six entry points would answer on (X, gid), in the shapes the diff_* functions read, from the restatements; rows: other
    label rows; D_off: a gene whose D is one too large (in the leave-one-out, whose folds form their own D from W: whose W is one too large
    in the first sample)"""
    genes, q, loo = tc.seam_genes(G, kind), tc.queries(G, kind), tc.loo_genes(G, kind)
    e = tc.expect(X, gid, genes, q, tc.row_seed(G, kind))
    if D_off is not None:
        e.W, e.D = e.W.copy(), e.D.copy()
        e.W[D_off, 0] += 1
        e.D[D_off] += 1
        e.top = tc.subset_oracle(X, gid, 2, 0, None, genes, e.D)
        e.rows_full = [tprc.row_oracle(X, gid, 2, 0, None, e.D, int(g)) for g in q]
    if rows is not None:
        e.null, e.pnull = tc.subset_null(X, rows, e.cuts, genes), tpnc.query_restate(X, rows, q, e.pcuts)
    e.loo = tc.subset_loo(X, gid, 2, 0, None, tc.KMAX, loo, e.W, e.D)
    return e


def differing(ans, e, loo, gene=1024):
    """per comparison of the GPU file, the fields in which the answers `ans` differ from the expectation; the chunk is that of `gene`"""
    lo, hi = tc.chunks(e.mask.size)[gene // tc.CHUNK]
    return {"shift": tc.diff_shift(ans.D, e), "pairs": tc.diff_pairs(tc.as_pairs(ans.top), e.top),
            "partners": tc.diff_partners(tc.as_partners(ans.rows_full), e.rows_full),
            "chunk": tc.diff_partners(tc.as_partners([tc.cut_row(r, lo, hi) for r in ans.rows_full]), [tc.cut_row(r, lo, hi) for r in e.rows_full]),
            "null": tc.diff_null(ans.null, e.null), "pnull": tc.diff_pnull(ans.pnull, e.pnull), "loo": tc.diff_loo(ans.loo, loo)}


def test_every_comparison_fails_on_planted_errors():
    G, kind = 9000, "ties"
    X, gid = tc.case(G, kind)
    e, loo = tc.expected(G, kind), tc.expected_loo(G, kind)
    right = differing(answers(X, gid, G, kind), e, loo)
    assert not any(right.values()), right                                        # the answers of the restatements themselves pass
    pick, out = int(loo.gene_i[0, 0]), int(np.setdiff1d(np.arange(G // 4), e.genes)[0])   # fold 0's first pick; a planted gene outside the set
    for g, hit in ((4096, ("shift", "pairs", "partners", "chunk", "null", "pnull")), (pick, ("shift", "pairs", "loo"))):   # a query; a pick
        assert g in e.genes and not np.array_equal(X[g], X[out])
        swapped = np.array(X)
        swapped[[g, out]] = swapped[[out, g]]
        bad = differing(answers(np.asfortranarray(swapped), gid, G, kind), e, loo)
        assert all(bad[k] for k in hit), ("two genes' rows swapped", g, out, bad)
    untied = np.asfortranarray(np.array(X) * G + np.arange(G)[:, None])          # eq dropped: every tie decided by the gene index
    bad = differing(answers(untied, gid, G, kind), e, loo)
    assert all(bad.values()), ("eq dropped", bad)
    rows = e.label_rows.copy()
    rows[16] = 1 - rows[16]                                                      # the last row, the one of the second launch group
    bad = differing(answers(X, gid, G, kind, rows=rows), e, loo)
    assert not any(bad.values())                                                 # a whole row exchanged: N changes its sign, |N| stays -- by definition
    at = [int(np.flatnonzero(e.label_rows[16] == v)[0]) for v in (1, 0)]
    rows = e.label_rows.copy()
    rows[16, at] = 1 - rows[16, at]                                              # so: one sample of either side exchanged
    bad = differing(answers(X, gid, G, kind, rows=rows), e, loo)
    assert bad["null"] and bad["pnull"] and not (bad["pairs"] or bad["partners"] or bad["shift"] or bad["loo"]), ("one label row's sides exchanged", bad)
    bad = differing(answers(X, (1 - gid).astype(gid.dtype), G, kind), e, loo)    # and the sides of the call itself
    assert bad["shift"] and bad["pairs"] and bad["partners"] and bad["chunk"] and bad["loo"], ("sides exchanged", bad)
    off = answers(X, gid, G, kind, D_off=pick)
    bad = differing(off, e, loo, pick)
    assert bad["shift"] and "rank_num" in bad["pairs"] and "rank_num" in bad["partners"] and "rank_num" in bad["chunk"] and bad["loo"], ("D off by one", bad)
    assert not bad["null"] and not bad["pnull"]                                  # (the nulls do not read D)
