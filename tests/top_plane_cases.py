"""Cases for the top-scoring family at 12, 15 and 16 position planes on ordinary data (tests/test_gpu_top_planes.py): reo_top_pairs,
reo_rank_shift, reo_top_pairs_null, reo_top_pairs_loo, reo_top_partners and reo_top_partners_null at the gene counts of
tests/plane_cases.py, on tie-free and on tie-rich matrices.  No fixtures, no GPU.

No G x G array exists at these sizes.  What is checked is (1) D of every gene, (2) every pair INSIDE A GENE SET of about 300 genes
(seam_mask) and (3) every cell of a few query rows across all G partners (queries).  The restatements are those of the family's own case
files, called on the sub-matrix of the gene set -- top_pairs_cases.side_counts, wide_top_pairs_cases.row_counts / restate_null /
Incremental, top_pairs_loo_cases.restate_candidates -- and on whole rows -- top_partners_cases.row_oracle,
top_partners_null_cases.query_restate.  The one quantity that a sub-matrix cannot give is the rank shift D (and its per-sample terms W),
which sums over ALL genes: it comes from one sort per sample (Int64: genes below = searchsorted left, genes above = G - searchsorted right),
or, for the Float64 case, from the band predicate abs(a - b) < 0.1 of a row against all genes, for the genes of the set only.
tests/test_top_plane_cases_cpu.py holds the subset forms to the whole-matrix functions on small cases.

cross_case and big_wide_case are the two cases of many genes and a wide sample axis together: 9 000 genes x 1 050 samples (34 blocks of 32
slots) and 65 600 genes x 265 samples (17 position planes, 10 blocks), with the masks, rows and lists that the query kernels are asked for.

The comparisons of the GPU file are the diff_* functions below: each returns the list of fields that differ (empty: equal), so that the
CPU file can show on planted errors that none of them is blind."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import masked_pairs_cases as mpc
import perm_null_cases as pnc
import plane_cases as pc
import top_pairs_cases as tpc
import top_pairs_loo_cases as lc
import top_pairs_null_cases as tnc
import top_partners_cases as tprc
import top_partners_null_cases as tpnc
import wide_sample_cases as wsc
import wide_top_pairs_cases as wt

KINDS = ("ranks", "ties", "ties_f64")
SEED = 0x5EED7A00
N_SEAM = 300              # genes of seam_mask: 44 850 pairs, all of them listed by one reo_top_pairs call
N_LOO = 120               # genes of the leave-one-out's mask
B_ROWS = 17               # label rows: a launch group of 16 and one row
KMAX = 5
CHUNK = 1024              # reo_top_partners lists at most 1 024 partners per row


def cases():
    """(G, kind): both kinds at DEEP_G, the kinds in turn at the boundary sizes and at PAD_G, and the Float64 band comparator once"""
    out = []
    for G in pc.PLANE_G + pc.PAD_G:
        out += [(G, kind) for kind in (("ranks", "ties") if G in pc.DEEP_G else (pc.boundary_kind(G),))]
    return out + [(9000, "ties_f64")]


def loo_cases():
    return [(G, kind) for G in pc.DEEP_G for kind in ("ties", "ranks")]


def tie_matrix(G, S, seed, second):
    """query_cases.tie_rich with a wider noise and a smaller effect: gene levels 0 .. 7, noise 0 .. 4, the first quarter of the genes 3 up
    and the second quarter 3 down in the samples `second`.  A value is shared by G / 12 genes and more, and few pairs are separated in
    every sample, so that the head of the order is not one plateau of |N|."""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(G, 1)) + rng.integers(0, 5, size=(G, S))
    X[: G // 4, second] += 3
    X[G // 4: G // 2, second] -= 3
    return X.astype(np.int64)


def matrix(G, kind, sizes, seed):
    """X (Fortran order) and gid for groups of `sizes`, interleaved.  `ranks`: tie-free Int64, every sample a permutation of 0 .. G - 1
    around gene levels, G / 8 genes planted up and as many down in group 1.  `ties`: tie_matrix, values -3 .. 14 with the effect in
    group 1 -- a value is shared by G / 12 genes and more.  `ties_f64`: Float64 rounded to two decimals."""
    if kind == "ranks":
        X, _, gid = mpc.rank_case(G, sizes, 0.0, seed, level=0.8, shift=2.0, planted=G // 8)
        X = np.rint(X / 10.0).astype(np.int64)
    elif kind == "ties":
        gid = mpc.interleaved(*sizes)
        X = tie_matrix(G, int(gid.size), seed, gid == 1)
    else:
        X, gid = pnc.case(G, sizes, "ties", seed, shift=2.0, planted=G // 8)
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X, gid


@functools.lru_cache(maxsize=None)
def case(G, kind):
    """X, gid of a case, built once and shared: read-only.  Side A is group 0, side B group 1 (a = 0, b = None)."""
    return matrix(G, kind, pc.sides(G), SEED + 4 * G + KINDS.index(kind))


def planted_genes(G, kind):
    """one gene planted up and one planted down in side B"""
    return (5, G // 4 + 5) if kind == "ties" else (5, G // 8 + 5)


def queries(G, kind):
    """0, 63, 64, one gene on each side of 4 096 and of 32 768 where they exist, G - 1, and two planted genes: sorted, int32"""
    seams = [g for g in (4095, 4096, 32767, 32768) if g < G - 1]
    return np.array(sorted({0, 63, 64, G - 1, *seams, *planted_genes(G, kind)}), dtype=np.int32)


@functools.lru_cache(maxsize=None)
def seam_genes(G, kind, n=N_SEAM):
    """the genes of seam_mask, sorted: the queries; both sides of 4 095 / 4 096, 8 191 / 8 192 and 32 767 / 32 768 where they exist; the
    last 40 genes (a ragged last tile, or the lone gene of the pad); random genes up to n"""
    fixed = set(queries(G, kind).tolist()) | set(range(G - 40, G))
    for seam in (4096, 8192, 32768):
        fixed |= {g for g in (seam - 2, seam - 1, seam, seam + 1) if g < G}
    rest = np.setdiff1d(np.arange(G), np.fromiter(fixed, dtype=np.int64))
    rng = np.random.default_rng(SEED + G)
    genes = np.sort(np.concatenate([np.fromiter(fixed, dtype=np.int64), rng.choice(rest, n - len(fixed), replace=False)]))
    genes.setflags(write=False)
    return genes


def mask_of(genes, G):
    m = np.zeros(G, dtype=bool)
    m[np.asarray(genes)] = True
    return m


def loo_genes(G, kind):
    """about N_LOO genes of seam_mask: the queries, the last 8 genes and every third of the others"""
    genes = seam_genes(G, kind)
    keep = set(queries(G, kind).tolist()) | set(range(G - 8, G))
    return np.array(sorted(keep | set(genes[::3][: N_LOO - len(keep)].tolist())), dtype=np.int64)


# ---- W and D over all genes

def rank_terms(X):
    """W[g, s] = (genes that g lies above) - (genes that g lies below) in sample s, G x S int64, for an integer matrix: one sort per sample
    (what searchsorted left and right on the sorted column give)"""
    X = np.asarray(X)
    assert X.dtype == np.int64
    G, S = X.shape
    W = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        _, inv, n = np.unique(X[:, s], return_inverse=True, return_counts=True)   # one sort: the genes at each value, values ascending
        upto = np.cumsum(n)
        W[:, s] = (upto - n)[inv] - (G - upto[inv])                               # below: the smaller values; above: G - (smaller or equal)
    return W


def band_terms(X, genes):
    """the rows `genes` of W for a Float64 matrix, len(genes) x S, by the exact predicate: tied when abs(a - b) < 0.1"""
    X = np.asarray(X)
    assert X.dtype == np.float64
    W = np.empty((len(genes), X.shape[1]), dtype=np.int64)
    for r, q in enumerate(genes):
        d = X[q][None, :] - X
        far = ~(np.abs(d) < 0.1)
        W[r] = ((d > 0) & far).sum(axis=0, dtype=np.int64) - ((d < 0) & far).sum(axis=0, dtype=np.int64)
    return W


def shift_of(W, in_a, in_b):
    """D = W(A) S_B - W(B) S_A"""
    return W[:, in_a].sum(axis=1) * int(in_b.sum()) - W[:, in_b].sum(axis=1) * int(in_a.sum())


def terms(X, genes=None):
    """W of every gene; for a Float64 matrix of the rows `genes` only, every other row 0 (those genes' D is never looked at)"""
    X = np.asarray(X)
    if X.dtype == np.int64:
        return rank_terms(X)
    W = np.zeros(X.shape, dtype=np.int64)
    W[np.asarray(genes)] = band_terms(X, genes)
    return W


# ---- subset forms

def subset_oracle(X, gid, ngroups, a, b, genes, D) -> tpc.Oracle:
    """top_pairs_cases.oracle with gene_mask = `genes` (sorted) without G x G arrays: the counts of the pairs inside the set from
    top_pairs_cases.side_counts on the sub-matrix, D (over all genes) from outside, the order of the definition.  N is genes x genes."""
    genes = np.asarray(genes, dtype=np.int64)
    assert (np.diff(genes) > 0).all()                                            # sorted: (i, j) inside the set orders as outside it
    gt_a, eq_a, gt_b, eq_b, s_a, s_b = tpc.side_counts(np.asarray(X)[genes], gid, ngroups, a, b)
    N = (2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a
    iu, ju = np.triu_indices(genes.size, 1)
    D = np.asarray(D, dtype=np.int64)
    num, gam = N[iu, ju], np.abs(D[genes[iu]] - D[genes[ju]])
    order = np.lexsort((ju, iu, -gam, -np.abs(num)))
    iu, ju = iu[order], ju[order]
    counts = np.stack([gt_a[iu, ju], eq_a[iu, ju], gt_b[iu, ju], eq_b[iu, ju]], axis=1).astype(np.int32)
    return tpc.Oracle(genes[iu].astype(np.int32), genes[ju].astype(np.int32), counts, num[order], gam[order], D, (s_a, s_b), N)


def subset_null(X, rows, cuts, genes, counts=None) -> tnc.Null:
    """top_pairs_null_cases.restate with gene_mask = `genes` (sorted): wide_top_pairs_cases.restate_null on the sub-matrix, the pair
    translated back.  |N| needs nothing from outside the set.  counts: wide_top_pairs_cases.row_counts of the sub-matrix, made before."""
    genes = np.asarray(genes, dtype=np.int64)
    sub = wt.restate_null(np.asarray(X)[genes], rows, cuts, counts)
    return tnc.Null(sub.max_num, genes[sub.arg_i].astype(np.int32), genes[sub.arg_j].astype(np.int32), sub.n_reach)


def subset_abs(X, rows, genes, counts=None):
    """|N| of the pairs i < j inside `genes` under every label row: rows x pairs int64"""
    rows = np.atleast_2d(np.asarray(rows))
    gt_a, eq_a, gt_b, eq_b = wt.row_counts(np.asarray(X)[np.asarray(genes)], rows) if counts is None else counts
    iu, ju = np.triu_indices(len(genes), 1)
    s_a, s_b = (rows == 1).sum(axis=1)[:, None], (rows == 0).sum(axis=1)[:, None]
    return np.abs((2 * gt_a[:, iu, ju] + eq_a[:, iu, ju] - s_a) * s_b - (2 * gt_b[:, iu, ju] + eq_b[:, iu, ju] - s_b) * s_a)


def cut_row(row: tprc.Row, lo, hi) -> tprc.Row:
    """top_partners_cases.row_oracle with partner_mask = the genes lo .. hi - 1, from the row over all partners: the order is total, so the
    masked row is the subsequence"""
    keep = (row.partner >= lo) & (row.partner < hi)
    return tprc.Row(row.partner[keep], row.counts[keep], row.num[keep], row.rank_num[keep])


def chunks(G):
    return [(lo, min(lo + CHUNK, G)) for lo in range(0, G, CHUNK)]


def subset_loo(X, gid, ngroups, a, b, kmax, genes, W, D) -> lc.Loo:
    """top_pairs_loo_cases.restate_candidates with gene_mask = `genes` (sorted): wide_top_pairs_cases.Incremental on the sub-matrix, whose
    per-sample terms w -- sums over ALL genes -- are given as the rows of W; the picks translated back"""
    genes = np.asarray(genes, dtype=np.int64)
    sub = np.asarray(X)[genes]
    inc = wt.Incremental(sub, gid, ngroups, a, b, w=np.ascontiguousarray(W[genes].T))
    full = subset_oracle(X, gid, ngroups, a, b, genes, D)
    local = full._replace(gene_i=np.searchsorted(genes, full.gene_i).astype(np.int32), gene_j=np.searchsorted(genes, full.gene_j).astype(np.int32))
    loo = lc.restate_candidates(sub, gid, ngroups, a, b, kmax, folds=inc.fold, full=local)
    back = lambda g: np.where(g >= 0, genes[np.maximum(g, 0)], -1).astype(np.int32)
    return loo._replace(gene_i=back(loo.gene_i), gene_j=back(loo.gene_j))


# ---- label rows and cuts

def label_rows(gid, seed, B=B_ROWS):
    """the observed labels, the inverted labels (top_pairs_null_cases.moved_rows) and B - 2 shuffles"""
    obs = tnc.observed_row(gid, 0, None)
    return np.concatenate([tnc.moved_rows(gid, seed)[:2], tnc.shuffled_rows(obs, B - 1, seed)[1:]])


ROW_SEED = {(4096, "ties"): 1, (9000, "ties"): 2, (65535, "ranks"): 1}        # seeds at which several pairs attain a shuffled row's maximum


def row_seed(G, kind):
    return SEED + G + 100000 * ROW_SEED.get((G, kind), 0)


# ---- the expectation of a case

class Expected(SimpleNamespace):
    """genes, q, mask, W, D, computed (the genes whose D is known), top (Oracle inside the mask), rows_full (one Row per query over all
    partners), label_rows, cuts, null (Null inside the mask), null_abs (rows x pairs), pcuts, pnull (PNull over all partners)"""


def expect(X, gid, genes, q, seed, B=B_ROWS) -> Expected:
    X = np.asarray(X)
    G = X.shape[0]
    in_a, in_b = tprc.side_masks(gid, 2, 0, None)
    e = Expected(genes=np.asarray(genes, dtype=np.int64), q=np.asarray(q, dtype=np.int32), mask=mask_of(genes, G))
    e.W = terms(X, e.genes)
    e.D = shift_of(e.W, in_a, in_b)
    e.computed = np.arange(G) if X.dtype == np.int64 else e.genes
    e.top = subset_oracle(X, gid, 2, 0, None, e.genes, e.D)
    pm = None if X.dtype == np.int64 else e.mask                                 # Float64: Gamma is known inside the set only
    e.partner_mask = pm
    e.rows_full = [tprc.row_oracle(X, gid, 2, 0, None, e.D, int(g), pm) for g in e.q]
    e.label_rows = label_rows(gid, seed, B)
    counts = wt.row_counts(X[e.genes], e.label_rows)
    e.null_abs = subset_abs(X, e.label_rows, e.genes, counts)
    top = int(e.null_abs[0].max())
    e.cuts = np.array([0, 1, top, top + 1], dtype=np.int64)
    e.null = subset_null(X, e.label_rows, e.cuts, e.genes, counts)
    if pm is None:                                                               # a row over all partners begins with the gene's observed maximum
        observed = np.array([abs(int(r.num[0])) for r in e.rows_full], dtype=np.int64)
    else:
        observed = tpnc.query_restate(X, e.label_rows[:1], e.q).max_num[0]
    e.pcuts = np.where(np.arange(e.q.size) % 2 == 0, observed, 1).astype(np.int64)   # the observed maximum, or 1
    e.pnull = tpnc.query_restate(X, e.label_rows, e.q, e.pcuts)
    return e


@functools.lru_cache(maxsize=None)
def expected(G, kind) -> Expected:
    """the expectation of a case, computed once and shared: read-only"""
    X, gid = case(G, kind)
    return expect(X, gid, seam_genes(G, kind), queries(G, kind), row_seed(G, kind))


@functools.lru_cache(maxsize=None)
def expected_loo(G, kind) -> lc.Loo:
    X, gid = case(G, kind)
    e = expected(G, kind)
    return subset_loo(X, gid, 2, 0, None, KMAX, loo_genes(G, kind), e.W, e.D)


# ---- many genes and a wide sample axis together

CROSS_G, CROSS_SIZES, CROSS_BLOCKS = 9000, (520, 530), 34   # 17 + 17 blocks of 32 slots: chunks of 8, 8, 8, 8, 2, a chunk seam inside each group
N_CROSS_LOO = 40                                            # genes of the leave-one-out's mask there: 1 050 folds


@functools.lru_cache(maxsize=None)
def cross_gid():
    """two groups of 520 and 530 samples under shuffled labels, numbered in order of first appearance: int32, read-only"""
    gid = wsc.first_appearance(np.random.default_rng(SEED + 1).permutation(np.repeat(np.arange(2), CROSS_SIZES)))
    gid.setflags(write=False)
    return gid


@functools.lru_cache(maxsize=None)
def cross_case(kind):
    """X, gid of the `cross` case, read-only.  `ties`: tie_matrix with the effect in group 1 plus wide_sample_cases.sample_pattern, so
    that every sample differs from its neighbours; `ranks`: the tie-free matrix of `matrix`, its columns dealt to the shuffled labels"""
    gid = cross_gid()
    G, S, seed = CROSS_G, int(gid.size), SEED + 7 + KINDS.index(kind)
    if kind == "ties":
        X = tie_matrix(G, S, seed, gid == 1) + wsc.sample_pattern(G, S)
    else:
        made, own = matrix(G, "ranks", tuple(int(n) for n in np.bincount(gid)), seed)
        X = np.empty_like(made)
        for g in (0, 1):
            X[:, gid == g] = made[:, own == g]
    X = np.asfortranarray(X.astype(np.int64))
    X.setflags(write=False)
    return X, gid


@functools.lru_cache(maxsize=None)
def cross_expected(kind) -> Expected:
    X, gid = cross_case(kind)
    return expect(X, gid, seam_genes(CROSS_G, kind), queries(CROSS_G, kind), SEED + CROSS_G + 1)


def cross_loo_genes(kind):
    """the queries and every eighth gene of seam_mask, N_CROSS_LOO in all"""
    genes = seam_genes(CROSS_G, kind)
    keep = set(queries(CROSS_G, kind).tolist())
    return np.array(sorted(keep | set(genes[3::8][: N_CROSS_LOO - len(keep)].tolist())), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def cross_expected_loo(kind) -> lc.Loo:
    X, gid = cross_case(kind)
    e = cross_expected(kind)
    return subset_loo(X, gid, 2, 0, None, KMAX, cross_loo_genes(kind), e.W, e.D)


def labels_of(gid):
    """string labels that the package's encode_groups numbers as gid: ids in order of first appearance"""
    assert np.array_equal(wsc.first_appearance(gid), gid)
    return np.array(["a", "b", "c"], dtype=object)[np.asarray(gid)]


def cross_partner_mask(marks, seed=SEED + 11):
    """the partner mask of the query kernels on `cross`: 55 % of the first tile of 4 096 table columns -- more than 2 048 listed partners,
    so that the counter planes above the first eleven are used --, 10 % of the other genes, and `marks`; fewer than 4 200 partners in
    all, the largest background that the tolerance of the exact tails is measured for"""
    rng = np.random.default_rng(seed)
    pm = rng.random(CROSS_G) < np.where(np.arange(CROSS_G) < 4096, 0.55, 0.10)
    pm[list(marks)] = True
    return pm


CROSS_BATCH = (32 << 20) // (CROSS_BLOCKS * 32 * 4)        # sc_batch_rows: 7 710 count rows of 1 088 slots fit 32 MiB, below 9 000


def cross_rows_checked(n=32, seed=SEED + 12):
    """the rows of the all-genes call that are compared: the first, the last, both sides of the batch seam and of 4 096, random ones"""
    fixed = {0, 4095, 4096, CROSS_BATCH - 1, CROSS_BATCH, CROSS_G - 1}
    rest = np.setdiff1d(np.arange(CROSS_G), np.fromiter(fixed, dtype=np.int64))
    more = np.random.default_rng(seed).choice(rest, n - len(fixed), replace=False)
    return np.array(sorted(fixed | set(more.tolist())), dtype=np.int32)


BIG_WIDE_G, BIG_WIDE_LAYOUT = 65600, "seam_in_group"       # 17 planes; S = 265 (130 + 135 shuffled), 10 blocks, chunks of 8 + 2
BIG_WIDE_Q = [65599, 0, 40000, 65535, 65536, 7]
BIG_WIDE_MARKS = [0, 4095, 4096, 65535, 65536, 65599]


@functools.lru_cache(maxsize=None)
def big_wide_case(seed=61):
    """X, gid, partner mask: the matrix of the sample tests' plane_case (tests/test_gpu_sample_tests.py) on the seam_in_group layout --
    Int64 gene levels below 30 000 with noise below 6 000, the first 20 000 genes 9 000 up in group 1 --, a mask of the marks and 194
    random partners"""
    gid = wsc.gid_of(BIG_WIDE_LAYOUT)
    G, S = BIG_WIDE_G, int(gid.size)
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, 30000, size=(G, 1)) + rng.integers(0, 6000, size=(G, S))).astype(np.int64)
    X[:20000, gid == 1] += 9000
    X = np.asfortranarray(X)
    X.setflags(write=False)
    pm = np.zeros(G, dtype=bool)
    pm[rng.choice(G, 194, replace=False)] = True
    pm[BIG_WIDE_MARKS] = True
    return X, gid, pm


def row_lists(genes, marks, G, seed, extra=70):
    """a CSR (genes, rowptr, partner) as tests/test_gpu_pair_support.py's big_case lists it: per gene the marks and `extra` random
    partners, shuffled, the gene itself left out"""
    rng = np.random.default_rng(seed)
    parts = []
    for i in genes:
        p = np.concatenate([np.asarray(marks), rng.choice(G, extra, replace=False)])
        parts.append(rng.permutation(p[p != i]))
    rowptr = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    return np.asarray(genes, dtype=np.int32), rowptr, np.concatenate(parts).astype(np.int32)


# ---- the comparisons of the GPU file: the fields that differ

def _ne(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(got, want)


def diff_shift(D, e: Expected):
    return ["D"] if _ne(np.asarray(D)[e.computed], e.D[e.computed]) else []


def diff_pairs(tp, o: tpc.Oracle, n=None):
    """a TopPairs against the first n pairs of an Oracle (None: its whole list)"""
    want = {"gene_i": o.gene_i, "gene_j": o.gene_j, "n_gt": o.counts[:, 0::2], "n_eq": o.counts[:, 1::2], "num": o.num, "rank_num": o.rank_num}
    bad = [f for f, w in want.items() if _ne(getattr(tp, f), w[:n])]
    return bad + (["side_sizes"] if tuple(int(v) for v in tp.side_sizes) != o.sizes else [])


CAP_N = (1000, 4096)      # list lengths of the capacity test: far fewer pairs than the 44 850 eligible ones, so that the select must refine


def diff_partners(tp, rows, m=CHUNK):
    """a TopPartners against the padded table of `rows`"""
    partner, counts, num, gam, found = tprc.table(rows, m)
    want = {"n_found": found, "partner": partner, "n_gt": counts[:, :, 0::2], "n_eq": counts[:, :, 1::2], "num": num, "rank_num": gam}
    return [f for f, w in want.items() if _ne(getattr(tp, f), w)]


def diff_null(got, want: tnc.Null):
    return [f for f in ("max_num", "arg_i", "arg_j", "n_reach") if _ne(getattr(got, f), getattr(want, f))]


def diff_pnull(got, want: tpnc.PNull):
    return [f for f in ("max_num", "arg_partner", "n_reach") if _ne(getattr(got, f), getattr(want, f))]


def diff_loo(got, want: lc.Loo):
    return [f for f in lc.FIELDS if _ne(getattr(got, f), getattr(want, f))] + \
        [f for f in ("cut", "n_candidates") if getattr(got, f) != getattr(want, f)]


# ---- what the library would answer from a restatement (the CPU file's stand-in for the device)

def as_pairs(o: tpc.Oracle):
    return SimpleNamespace(gene_i=o.gene_i, gene_j=o.gene_j, n_gt=o.counts[:, 0::2], n_eq=o.counts[:, 1::2], num=o.num, rank_num=o.rank_num,
                           side_sizes=o.sizes)


def as_partners(rows, m=CHUNK):
    partner, counts, num, gam, found = tprc.table(rows, m)
    return SimpleNamespace(partner=partner, n_gt=counts[:, :, 0::2], n_eq=counts[:, :, 1::2], num=num, rank_num=gam, n_found=found)


# ---- truncated ranks

def gt_counts(M, gid, rows_of, cols_of):
    """gt per group of the ordered pairs rows_of x cols_of of a matrix, len(rows_of) x len(cols_of) x 2 int64, per sample: Float64 tied
    inside the band 0.1, integers when equal -- the comparator of plane_cases.masked_counts_block without a mask"""
    M = np.asarray(M)
    assert M.dtype in (np.float64, np.int64), M.dtype
    rows_of, cols_of = np.asarray(rows_of, dtype=np.int64), np.asarray(cols_of, dtype=np.int64)
    gt = np.zeros((rows_of.size, cols_of.size, 2), dtype=np.int64)
    for s in range(M.shape[1]):
        a, b = M[rows_of, s][:, None], M[cols_of, s][None, :]
        tie = (np.abs(a - b) < 0.1) if M.dtype == np.float64 else (a == b)
        gt[:, :, int(gid[s])] += ~tie & (a > b)
    return gt


def truncated_counts(X, gid, rows_of, cols_of, bits, R=None):
    """gt per group of the pairs rows_of x cols_of when every sample's ranks (plane_cases.sample_ranks: the genes strictly below; R, when
    the caller has them) lose the bits from `bits` upwards, and the true gt: two len(rows_of) x len(cols_of) x 2 arrays.  bits = 18
    truncates nothing."""
    R = pc.sample_ranks(X) if R is None else R
    return gt_counts(R & ((1 << bits) - 1), gid, rows_of, cols_of), gt_counts(X, gid, rows_of, cols_of)
