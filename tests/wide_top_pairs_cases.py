"""Cases for the top-scoring-pair family (reo_top_pairs, reo_rank_shift, reo_top_pairs_null, reo_top_pairs_loo) on wide sample axes
(tests/test_gpu_wide_top_pairs.py, tests/test_wide_top_pairs_cases_cpu.py).  No fixtures, no GPU, no import of the package.

The cases of tests/top_pairs_cases.py stop at 64 samples: two blocks of 32 sample slots per side.  Here:

  ROWS        the layouts of tests/wide_sample_cases.py (10 to 21 blocks) with the sides named by group SIZE:
    row               layout           side A   side B   data                      what it reaches
    seam              seam_in_group    id 0     rest     float_ties, G = 130       5 + 5 blocks; padding in both sides; Float64 ties
    full_ties         full_blocks      id 0     rest     int_ties, G = 70          no padding slot; eq of a side above 64; 9-bit counts
    full_ranks        full_blocks      id 0     rest     ranks, G = 130, tie-free  the TIES = false form of k_top_pairs_null over 16 blocks
    three_33_31       three_groups     33       31       float_ties, G = 130       the 300-sample group (10 blocks) on neither side
    three_300_rest    three_groups     300      rest     the same matrix           side B a union of two groups; a side of 10 blocks
    padding_30_rest   mostly_padding   30       rest     float_ties, G = 130       side B a union of 16 groups, 15 of them of 1-3 samples
    padding_20_30     mostly_padding   20       30       the same matrix           15 tiny groups on neither side: live words of no bit
    contrast_300_260  contrast_groups  300      260      float_ties, G = 70        21 blocks; counts above 255; the 40-group on neither side
  deep_gamma  G = 66, Int64, sides of 6 016 and 4 600 samples interleaved (332 blocks): twelve genes lie below every other gene in side A
              and above every other gene in side B, so 12 x 54 = 648 pairs reach |N| = 2 S_A S_B and Gamma alone orders them -- and
              Gamma straddles 2^32 there (21 of the 648 lie above it): the part of Gamma that tp_pack puts into TpKey.hi differs
              between the leading pairs.  (At 6 016 / 5 500 the 50 leading pairs all share the high word 1.)
  limit       the same construction with six such genes (360 pairs) at sides of 32 768 and 32 767 samples: S = 65 535 = kTpMaxSamples,
              2 048 blocks, 2 S_A S_B = 2^31 - 65 536, Gamma up to 2^37.

`Incremental` restates a fold of the leave-one-out without the G x G x S walk per fold that top_pairs_loo_cases.fold_oracle makes: the
per-sample gt / eq bits of every pair and the per-sample rank contribution of every gene are made once; a fold subtracts its sample's.
`row_counts` restates the null's counts per label row by matrix products; at the limit the search's expectation is made from them too.
tests/test_wide_top_pairs_cases_cpu.py holds all of them to the definitions they shorten."""
from __future__ import annotations

import functools

import numpy as np

import float32_cases as fc
import masked_pairs_cases as mpc
import perm_null_cases as pnc
import top_pairs_cases as tpc
import top_pairs_loo_cases as lc
import top_pairs_null_cases as tnc
import wide_sample_cases as wc

K = 5          # picks per fold
N = 50         # pairs of a search
B_NULL = 33    # label rows of a null: two launch groups of 16 and one row

# row: (layout, size of side A's group or None for id 0, size of side B's group or None for the rest, kind of data, G, seed).  The seeds of
# the Float64 rows are the first at which pair 50 and pair 51 of the order share the first digit of the key that can differ, so that a
# candidate buffer of 50 records makes the pass loop refine (select_passes; asserted on the CPU): at most seeds the 50 largest |N| lie
# so far apart that one pass ends the selection at any capacity.
ROWS = {"seam": ("seam_in_group", None, None, "float", 130, 48),
        "full_ties": ("full_blocks", None, None, "int", wc.G_TABLE, wc.TABLE_SEED["full_blocks"]),
        "full_ranks": ("full_blocks", None, None, "ranks", 130, 43),
        "three_33_31": ("three_groups", 33, 31, "float", 130, 42),
        "three_300_rest": ("three_groups", 300, None, "float", 130, 42),
        "padding_30_rest": ("mostly_padding", 30, None, "float", 130, 41),
        "padding_20_30": ("mostly_padding", 20, 30, "float", 130, 41),
        "contrast_300_260": ("contrast_groups", 300, 260, "float", 70, 48)}
MASKED_ROW = "three_33_31"      # the row that also runs under a gene mask
LONG_ROW, LONG_N = "seam", 3000  # the row whose list is also read deep enough to cross many equal |N|

# name: (S_A, S_B, seed, separated genes) of the two cases built by separated_levels
DEEP = {"deep_gamma": (6016, 4600, 7, 12), "limit": (32768, 32767, 7, 6)}
G_DEEP = 66


def sides(name):
    """(a, b) of a row: group ids of the layout (they depend on its shuffle), b None for every other sample"""
    layout, sa, sb = ROWS[name][:3]
    return (0 if sa is None else wc.group_of_size(layout, sa)), (None if sb is None else wc.group_of_size(layout, sb))


def effect_group(name):
    """the group whose samples the data's effect leaves out: side A, except where the same matrix serves two rows"""
    shared = {"three_300_rest": 33, "padding_20_30": 30}
    return wc.group_of_size(ROWS[name][0], shared[name]) if name in shared else sides(name)[0]


def separated_levels(s_a, s_b, seed, m, G=G_DEEP):
    """Int64, sides interleaved.  Genes 0 .. m - 1 lie near -1000 in side A and near 1000 in side B: below every other gene in A, above
    every other gene in B, so the m (G - m) pairs with one of them reach |N| = 2 S_A S_B.  Every gene holds a level of 0 .. 7 plus noise
    per sample -- 0 .. 7 on the m genes, whose levels are drawn per side, 0 .. 5 on the others, which also carry an effect of their own
    out of -2 .. 2 in side B --: ties everywhere, rank shifts D that spread over the genes of either kind, and no further pair that is
    separated in every sample (the noise spans as much as two levels can differ, or the effects cannot turn the order round).
    Returns X (column-major) and gid."""
    rng = np.random.default_rng(seed)
    gid = mpc.interleaved(s_a, s_b)
    S = int(gid.size)
    in_b = gid == 1
    X = np.empty((G, S), dtype=np.int64)
    X[:m] = rng.integers(0, 8, size=(m, S))
    X[:m, ~in_b] += rng.integers(0, 8, size=(m, 1)) - 1000
    X[:m, in_b] += rng.integers(0, 8, size=(m, 1)) + 1000
    X[m:] = rng.integers(0, 8, size=(G - m, 1)) + rng.integers(0, 6, size=(G - m, S))
    X[m:, in_b] += rng.integers(-2, 3, size=(G - m, 1))
    assert X[m:].min() > -900 and X[m:].max() < 900 and X[:m, ~in_b].max() < -900 and X[:m, in_b].min() > 900
    return np.asfortranarray(X), gid


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, gid, ngroups, a, b) of a row or of deep_gamma / limit, built once and shared: read-only"""
    if name in DEEP:
        s_a, s_b, seed, m = DEEP[name]
        X, gid = separated_levels(s_a, s_b, seed, m)
        X.setflags(write=False)
        gid.setflags(write=False)
        return X, gid, 2, 0, None
    layout, _, _, kind, G, seed = ROWS[name]
    gid = wc.gid_of(layout)
    a, b = sides(name)
    k = effect_group(name)
    if kind == "float":
        X = wc.float_ties(layout, G, seed, k)
    elif kind == "int":
        X = wc.int_ties(layout, G, seed, k, pattern=False)
    else:
        X = wc.ranks(layout, G, seed, effect_group=k)
    return X, gid, int(gid.max()) + 1, a, b


def blocks(name):
    """blocks of 32 sample slots that the context of a case walks: every group padded to whole blocks"""
    gid = case(name)[1]
    return int(sum((int(n) + 31) // 32 for n in np.bincount(gid)))


def oracle_from_counts(gt_a, eq_a, gt_b, eq_b, s_a, s_b) -> tpc.Oracle:
    """top_pairs_cases.oracle behind its side_counts, no gene mask: N, D, Gamma and the order from the G x G counts of the two sides"""
    G = gt_a.shape[0]
    N = (2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a
    D = (gt_a.sum(axis=1) - gt_a.sum(axis=0)) * s_b - (gt_b.sum(axis=1) - gt_b.sum(axis=0)) * s_a
    iu, ju = np.triu_indices(G, 1)
    num, gam = N[iu, ju], np.abs(D[iu] - D[ju])
    order = np.lexsort((ju, iu, -gam, -np.abs(num)))
    iu, ju = iu[order], ju[order]
    counts = np.stack([gt_a[iu, ju], eq_a[iu, ju], gt_b[iu, ju], eq_b[iu, ju]], axis=1).astype(np.int32)
    return tpc.Oracle(iu.astype(np.int32), ju.astype(np.int32), counts, num[order], gam[order], D, (s_a, s_b), N)


@functools.lru_cache(maxsize=None)
def expected(name) -> tpc.Oracle:
    """the search's oracle of a case, computed once and shared: read-only.  top_pairs_cases.oracle itself, except at the limit, where its
    one Python step per sample takes seconds: there the counts come from row_counts under the observed label row (the products are
    shared with the null's expectation), and tests/test_wide_top_pairs_cases_cpu.py holds the result to top_pairs_cases.oracle field by
    field."""
    X, gid, ng, a, b = case(name)
    if name == "limit":
        gt_a, eq_a, gt_b, eq_b = (c[0] for c in _deep_counts(name))
        row = deep_rows(name)[0]
        return oracle_from_counts(gt_a, eq_a, gt_b, eq_b, int((row == 1).sum()), int((row == 0).sum()))
    return tpc.oracle(X, gid, ng, a, b)


def gene_mask(name):
    return tpc.half_mask(case(name)[0].shape[0], seed=6)


@functools.lru_cache(maxsize=None)
def expected_masked(name) -> tpc.Oracle:
    X, gid, ng, a, b = case(name)
    return tpc.oracle(X, gid, ng, a, b, gene_mask(name))


# ---- the null

@functools.lru_cache(maxsize=None)
def rows(name, B=B_NULL):
    """B label rows of a case: the observed one and seeded shuffles of it (top_pairs_null_cases.shuffled_rows), read-only"""
    _, gid, _, a, b = case(name)
    seed = 300 + (list(ROWS) + list(DEEP)).index(name)
    r = tnc.shuffled_rows(tnc.observed_row(gid, a, b), B, seed)
    r.setflags(write=False)
    return r


def cuts(name):
    """top_pairs_null_cases.cuts' rule: [0, 1, median |N|, observed max, 2 S_A S_B, 2 S_A S_B + 1], from the search's oracle"""
    e = expected(name)
    n = np.abs(e.num)
    full = 2 * e.sizes[0] * e.sizes[1]
    return np.array([0, 1, int(np.median(n)), int(n.max()), full, full + 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def expected_null(name) -> tnc.Null:
    """top_pairs_null_cases.restate over the B_NULL rows and the six cuts of a row, computed once and shared: read-only"""
    return tnc.restate(case(name)[0], rows(name), cuts(name))


@functools.lru_cache(maxsize=None)
def expected_null_masked(name) -> tnc.Null:
    return tnc.restate(case(name)[0], rows(name), cuts(name), gene_mask(name))


def row_counts(X, label_rows):
    """(gt_A, eq_A, gt_B, eq_B), each R x G x G int64 per ordered pair, under every label row at once: gene by gene the comparison of
    masked_pairs_cases.masked_counts (Float64 or integers: tied inside the band 0.1) as a G x S matrix, times the S x R indicators of the
    sides.  The products run in Float32, where sums of at most 2^24 ones are exact (asserted); no code shared with masked_counts."""
    X = np.asarray(X)
    assert X.dtype != np.float32 and X.shape[1] < (1 << 24)
    label_rows = np.atleast_2d(np.asarray(label_rows))
    X64 = X.astype(np.float64)
    G, R = X.shape[0], label_rows.shape[0]
    ind = np.concatenate([(label_rows == 1).T, (label_rows == 0).T], axis=1).astype(np.float32)   # S x 2 R
    gt, eq = np.empty((2 * R, G, G), dtype=np.int64), np.empty((2 * R, G, G), dtype=np.int64)
    for i in range(G):
        tie = np.abs(X64[i][None, :] - X64) < 0.1
        above = (X64[i][None, :] > X64) & ~tie
        gt[:, i, :] = np.rint(above.astype(np.float32) @ ind).astype(np.int64).T
        eq[:, i, :] = np.rint(tie.astype(np.float32) @ ind).astype(np.int64).T
    return gt[:R], eq[:R], gt[R:], eq[R:]


def restate_null(X, label_rows, cut_values, counts=None) -> tnc.Null:
    """top_pairs_null_cases.restate's outputs from row_counts (`counts`: made before): for the cases whose sample axis makes a walk per
    row slow"""
    label_rows = np.atleast_2d(np.asarray(label_rows))
    gt_a, eq_a, gt_b, eq_b = row_counts(X, label_rows) if counts is None else counts
    iu, ju = np.triu_indices(np.asarray(X).shape[0], 1)                          # (i, j) ascending: argmax finds the first among equals
    cut_values = np.asarray(cut_values, dtype=np.int64).reshape(-1)
    R = label_rows.shape[0]
    out = tnc.Null(np.full(R, -1, np.int64), np.full(R, -1, np.int32), np.full(R, -1, np.int32), np.zeros((R, cut_values.size), np.int64))
    for p in range(R):
        s_a, s_b = int((label_rows[p] == 1).sum()), int((label_rows[p] == 0).sum())
        n = np.abs((2 * gt_a[p] + eq_a[p] - s_a) * s_b - (2 * gt_b[p] + eq_b[p] - s_b) * s_a)[iu, ju]
        e = int(np.argmax(n))
        out.max_num[p], out.arg_i[p], out.arg_j[p] = n[e], iu[e], ju[e]
        out.n_reach[p] = (n[None, :] >= cut_values[:, None]).sum(axis=1)
    return out


def deep_rows(name):
    """the label rows of deep_gamma / limit: the observed one and two shuffles"""
    return rows(name, 3)


def deep_cuts(name):
    """the six cuts of `cuts`, 2 S_A S_B and 2 S_A S_B + 1 among them"""
    return cuts(name)


@functools.lru_cache(maxsize=None)
def _deep_counts(name):
    return row_counts(case(name)[0], deep_rows(name))


@functools.lru_cache(maxsize=None)
def expected_deep_null(name) -> tnc.Null:
    return restate_null(case(name)[0], deep_rows(name), deep_cuts(name), _deep_counts(name))


# ---- the leave-one-out

class Incremental:
    """The folds of top_pairs_loo_cases.fold_oracle without a walk over the samples per fold.  Made once: for every pair i < j and sample
    the bits gt (gene i above gene j, not tied) and eq (tied), under masked_pairs_cases.masked_counts' comparator for the element type
    (Float32 in Float32 arithmetic, everything else widened to Float64 with the band 0.1); from them w[g, s] = genes that g lies above -
    genes that g lies below in sample s, over ALL genes as the oracle's D sums them; and the sums of all three over the two sides.
    fold(s) subtracts the sample's bits and contribution on its side, shrinks that side by one, forms N(s), D(s) and Gamma(s) and orders
    the eligible pairs by lexsort as top_pairs_cases.oracle does.  w (S x G), when given, stands for the w of the matrix's own genes: the
    rows of X are then some genes of a larger matrix, and w sums over all of that one's (tests/top_plane_cases.py, subset_loo)."""

    def __init__(self, X, gid, ngroups, a, b, gene_mask=None, w=None):
        X = np.asarray(X)
        G, S = X.shape
        self.side = lc.sides_of(gid, ngroups, a, b)
        iu, ju = np.triu_indices(G, 1)
        gt, eq = np.empty((S, iu.size), dtype=bool), np.empty((S, iu.size), dtype=bool)   # sample-major: a fold reads one row
        X64 = X.astype(np.float64)
        if X.dtype == np.float32:
            for s in range(S):
                tie = fc.f32_ties(X[:, s])[iu, ju]
                eq[s], gt[s] = tie, ~tie & (X64[iu, s] > X64[ju, s])
        else:
            at = 0
            for i in range(G - 1):                                               # the pairs (i, i + 1 .. G - 1) are consecutive in triu order
                d = X64[i][None, :] - X64[i + 1:]
                tie = np.abs(d) < 0.1
                eq[:, at: at + G - 1 - i], gt[:, at: at + G - 1 - i] = tie.T, ((d > 0) & ~tie).T
                at += G - 1 - i
        if w is None:
            w = np.zeros((S, G), dtype=np.int64)
            at = 0
            for i in range(G - 1):
                d = gt[:, at: at + G - 1 - i].astype(np.int64) - (~gt[:, at: at + G - 1 - i] & ~eq[:, at: at + G - 1 - i])   # +1 i above j, -1 below, 0 tied
                w[:, i] += d.sum(axis=1)
                w[:, i + 1:] -= d
                at += G - 1 - i
        else:                                                                    # X is a sub-matrix of a larger one: w comes from all of its genes
            w = np.asarray(w, dtype=np.int64)
            assert w.shape == (S, G)
        in_a, in_b = self.side == 1, self.side == 0
        self.gt, self.eq, self.w = gt, eq, w
        self.s_a, self.s_b = int(in_a.sum()), int(in_b.sum())
        self.gt_a, self.eq_a, self.w_a = gt[in_a].sum(axis=0, dtype=np.int64), eq[in_a].sum(axis=0, dtype=np.int64), w[in_a].sum(axis=0)
        self.gt_b, self.eq_b, self.w_b = gt[in_b].sum(axis=0, dtype=np.int64), eq[in_b].sum(axis=0, dtype=np.int64), w[in_b].sum(axis=0)
        keep = np.ones(G, dtype=bool) if gene_mask is None else np.asarray(gene_mask, dtype=bool)
        self.sel = slice(None) if keep.all() else np.flatnonzero(keep[iu] & keep[ju])
        self.iu, self.ju = iu[self.sel].astype(np.int32), ju[self.sel].astype(np.int32)

    def fold(self, s) -> tpc.Oracle:
        """the order of fold s (counts and the G x G table are not made: top_pairs_loo_cases reads neither)"""
        out_a, out_b = int(self.side[s] == 1), int(self.side[s] == 0)
        assert out_a + out_b == 1, s                                             # a sample of neither side is no fold
        s_a, s_b = self.s_a - out_a, self.s_b - out_b
        g, e, w = self.gt[s][self.sel], self.eq[s][self.sel], self.w[s]         # (bool: 0 / 1 in the integer arithmetic below)
        gt_a, eq_a, gt_b, eq_b = self.gt_a[self.sel] - out_a * g, self.eq_a[self.sel] - out_a * e, self.gt_b[self.sel] - out_b * g, self.eq_b[self.sel] - out_b * e
        num = (2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a
        D = (self.w_a - out_a * w) * s_b - (self.w_b - out_b * w) * s_a
        gam = np.abs(D[self.iu] - D[self.ju])
        order = np.lexsort((self.ju, self.iu, -gam, -np.abs(num)))               # (the last key is the primary one)
        return tpc.Oracle(self.iu[order], self.ju[order], None, num[order], gam[order], D, (s_a, s_b), None)


@functools.lru_cache(maxsize=None)
def incremental(name, masked=False) -> Incremental:
    X, gid, ng, a, b = case(name)
    return Incremental(X, gid, ng, a, b, gene_mask(name) if masked else None)


@functools.lru_cache(maxsize=None)
def fold(name, s, masked=False) -> tpc.Oracle:
    return incremental(name, masked).fold(s)


@functools.lru_cache(maxsize=None)
def expected_loo(name, kmax=K, masked=False) -> lc.Loo:
    """the definition (top_pairs_loo_cases.restate: every fold from all eligible pairs) on the incremental folds: read-only"""
    X, gid, ng, a, b = case(name)
    return lc.restate(X, gid, ng, a, b, kmax, gene_mask(name) if masked else None, folds=lambda s: fold(name, s, masked))


@functools.lru_cache(maxsize=None)
def expected_loo_candidates(name, kmax=K, masked=False) -> lc.Loo:
    """the library's route (top_pairs_loo_cases.restate_candidates: the band of the cut) on the incremental folds: read-only"""
    X, gid, ng, a, b = case(name)
    full = expected_masked(name) if masked else expected(name)
    return lc.restate_candidates(X, gid, ng, a, b, kmax, gene_mask(name) if masked else None, folds=lambda s: fold(name, s, masked), full=full)


def seam_folds(name):
    """the folds that a restatement is held to the definition at: the first and the last sample of either side, and the samples on either
    side of a block seam -- the last real slot of a block and slot 0 of the next, where both are folds --, at the first such seam and
    at the last.  Returns the folds and the number of such seams."""
    _, gid, ng, a, b = case(name)
    side = lc.sides_of(gid, ng, a, b)
    m = pnc.slot_map(gid, ng)
    out = set()
    for v in (1, 0):
        at = np.flatnonzero(side == v)
        out.update((int(at[0]), int(at[-1])))
    seams = []
    for s in range(32, m.size, 32):
        last = m[s - 32: s][m[s - 32: s] >= 0][-1]                               # (every block holds a sample: groups fill theirs from slot 0)
        if side[last] != 2 and side[m[s]] != 2:
            seams.append((int(last), int(m[s])))
    for pair in seams[:1] + seams[-1:]:
        out.update(pair)
    return sorted(out), len(seams)


def picks_with(o: tpc.Oracle, gam, kmax):
    """the greedy picks of a fold's pairs when `gam` stands in for Gamma: (gene_i, gene_j) of the picks"""
    order = np.lexsort((o.gene_j, o.gene_i, -gam, -np.abs(o.num)))
    alt = o._replace(gene_i=o.gene_i[order], gene_j=o.gene_j[order])
    at = lc.greedy(alt, kmax)
    return alt.gene_i[at].tolist(), alt.gene_j[at].tolist()


# ---- the pass loop of the selection

def ones_below(bound):
    """tp_ones_below of csrc/top_pairs.h: all ones below the highest bit of a bound"""
    m = 0
    while m < bound:
        m = (m << 1) | 1
    return m


def select_passes(e: tpc.Oracle, G, n_want, capacity):
    """(histogram passes, candidates) of tp_select (csrc/top_pairs.h) over the oracle's pairs, restated on Python integers: the key is
    |N| << 80 | Gamma << 32 | 2^32 - 1 - (i G + j); ten digits of 12 bits from the top; a digit that the bounds 2 S_A S_B and
    max D - min D prove zero costs no pass; the loop ends once the keys at or above the chosen bin fit the capacity."""
    keys = [(abs(int(n)) << 80) | (int(g) << 32) | (0xFFFFFFFF - (int(i) * G + int(j))) for n, g, i, j in zip(e.num, e.rank_num, e.gene_i, e.gene_j)]
    mask = (ones_below(2 * e.sizes[0] * e.sizes[1]) << 80) | (ones_below(int(e.D.max() - e.D.min())) << 32) | 0xFFFFFFFF
    prefix, passes, live = 0, 0, keys
    for shift in range(108, -1, -12):
        if (mask >> shift) & 0xFFF == 0:
            prefix <<= 12
            continue
        passes += 1
        live = [k for k in live if (k >> (shift + 12)) >= prefix]                # at or above the prefix: counted by every later pass too
        above = sum(1 for k in live if (k >> (shift + 12)) > prefix)
        bins = np.bincount([(k >> shift) & 0xFFF for k in live if (k >> (shift + 12)) == prefix], minlength=4096)
        cum, digit = above, -1
        for d in range(4095, -1, -1):
            if cum + bins[d] >= n_want:
                digit = d
                break
            cum += int(bins[d])
        if digit < 0:
            return passes, cum                                                   # fewer than n_want eligible pairs: all of them
        prefix = (prefix << 12) | digit
        if cum + int(bins[digit]) <= capacity:
            return passes, cum + int(bins[digit])
    return passes, cum + 1


def default_capacity(n_want):
    """tp_capacity without REO_TOP_PAIRS_CAP: max(4 n_want, 2^18) candidate records"""
    return max(4 * n_want, 1 << 18)
