"""Cases for the leave-one-out cross-validation of the k-TSP selection (reo_top_pairs_loo): two numpy restatements on the cases of
tests/top_pairs_cases.py.  No fixtures, no GPU.

The definition (include/reo_hip.h): a fold is one sample s of side A or B; the fold's result is what the search gives when s is moved into a
group on neither side -- the fold relabels (s -> group 2, side A -> 0, side B -> 1, everything else -> 2), calls top_pairs_cases.oracle(X, g,
3, 0, 1), walks its order greedily (a pair is taken when neither gene is used, up to kmax pairs) and reads the held-out sample's outcome
from the values.  `restate` does exactly that; `restate_candidates` restates the library's route: the cut T from the full-data oracle,
then the same greedy walk over the pairs with full |N| >= T only.  That the two agree is the bound of csrc/top_pairs_loo.h."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import masked_pairs_cases as mpc
import top_pairs_cases as tpc


class Loo(NamedTuple):
    gene_i: np.ndarray     # S x kmax int32, -1 where there is no pick
    gene_j: np.ndarray
    num: np.ndarray        # S x kmax int64, N of the fold (signed)
    rank_num: np.ndarray   # S x kmax int64, Gamma of the fold
    outcome: np.ndarray    # S x kmax int8
    side: np.ndarray       # S int8: 1 = A, 0 = B, 2 = neither
    cut: int               # restate: 0; restate_candidates: T
    n_candidates: int      # restate: every eligible pair


def sides_of(gid, ngroups, a, b):
    """int8 per sample: 1 = side A, 0 = side B, 2 = neither"""
    gid = np.asarray(gid)
    return np.where(gid == a, 1, np.where((gid != a) if b is None else (gid == b), 0, 2)).astype(np.int8)


def fold_groups(side, s):
    """the group ids of fold s: side A -> 0, side B -> 1, the held-out sample and the samples of neither side -> 2"""
    g = np.where(side == 1, 0, np.where(side == 0, 1, 2)).astype(np.int32)
    g[s] = 2
    return g


def fold_oracle(X, side, s, gene_mask=None) -> tpc.Oracle:
    return tpc.oracle(X, fold_groups(side, s), 3, 0, 1, gene_mask)


def greedy(o: tpc.Oracle, kmax, allowed=None):
    """the indices into the oracle's order of the greedy disjoint walk; `allowed`: G x G bool, the pairs that may be taken"""
    used, out = set(), []
    for e, (i, j) in enumerate(zip(o.gene_i.tolist(), o.gene_j.tolist())):
        if len(out) >= kmax:
            break
        if i in used or j in used or (allowed is not None and not allowed[i, j]):
            continue
        used.update((i, j))
        out.append(e)
    return np.asarray(out, dtype=np.int64)


def outcome_of(X, i, j, s):
    """+1 gene i above gene j in sample s, 0 tied, -1 below, under the comparator of X's element type -- that of
    masked_pairs_cases.masked_counts: Float32 in Float32 arithmetic, everything else widened to Float64 with the band 0.1"""
    col = np.asarray(X)[:, s]
    x, y = col[i].astype(np.float64), col[j].astype(np.float64)
    tie = mpc.fc.f32_ties(col)[i, j] if col.dtype == np.float32 else np.abs(x - y) < 0.1
    return np.where(tie, 0, np.where(x > y, 1, -1)).astype(np.int8)


def _fill(X, side, kmax, folds, allowed, cut, n_cand) -> Loo:
    S = X.shape[1]
    gi, gj = np.full((S, kmax), -1, dtype=np.int32), np.full((S, kmax), -1, dtype=np.int32)
    num, gam, out = np.zeros((S, kmax), dtype=np.int64), np.zeros((S, kmax), dtype=np.int64), np.zeros((S, kmax), dtype=np.int8)
    for s in np.flatnonzero(side != 2):
        o = folds(int(s))
        at = greedy(o, kmax, allowed)
        k = at.size
        gi[s, :k], gj[s, :k], num[s, :k], gam[s, :k] = o.gene_i[at], o.gene_j[at], o.num[at], o.rank_num[at]
        out[s, :k] = outcome_of(X, o.gene_i[at], o.gene_j[at], s)
    return Loo(gi, gj, num, gam, out, side, cut, n_cand)


def restate(X, gid, ngroups, a, b, kmax, gene_mask=None, folds=None) -> Loo:
    """every fold from all eligible pairs: the definition"""
    side = sides_of(gid, ngroups, a, b)
    folds = folds or (lambda s: fold_oracle(X, side, s, gene_mask))
    G = X.shape[0] if gene_mask is None else int(np.asarray(gene_mask, dtype=bool).sum())
    return _fill(X, side, kmax, folds, None, 0, G * (G - 1) // 2)


def cut_of(full: tpc.Oracle, kmax):
    """T = max(v - 4 max(S_A, S_B), 0), v = |N| of the last of the 2 kmax greedy disjoint pairs of the full-data order; 0 without them"""
    at = greedy(full, 2 * kmax)
    if at.size < 2 * kmax:
        return 0
    return max(abs(int(full.num[at[-1]])) - 4 * max(full.sizes), 0)


def restate_candidates(X, gid, ngroups, a, b, kmax, gene_mask=None, folds=None, full=None) -> Loo:
    """the library's route: only the pairs with full-data |N| >= T may be taken"""
    side = sides_of(gid, ngroups, a, b)
    full = full or tpc.oracle(X, gid, ngroups, a, b, gene_mask)
    T = cut_of(full, kmax)
    keep = np.abs(full.num) >= T
    allowed = np.zeros((X.shape[0], X.shape[0]), dtype=bool)
    allowed[full.gene_i[keep], full.gene_j[keep]] = True
    folds = folds or (lambda s: fold_oracle(X, side, s, gene_mask))
    return _fill(X, side, kmax, folds, allowed, T, int(keep.sum()))


CASES = ["float300", "count_i64", "count_i32", "count_f32", "three_0_2", "three_1_rest", "separated", "level"]


@functools.lru_cache(maxsize=None)
def fold(name, s) -> tpc.Oracle:
    """the oracle of fold s of a named case, computed once and shared: treat as read-only"""
    if name == "count_i32":                                                      # (the same cells and the same rule as Int64)
        return fold("count_i64", s)
    X, gid, ng, a, b = tpc.case(name)
    return fold_oracle(X, sides_of(gid, ng, a, b), s)


@functools.lru_cache(maxsize=None)
def expected(name, kmax) -> Loo:
    """the definition on a named case, computed once and shared: treat as read-only"""
    X, gid, ng, a, b = tpc.case(name)
    return restate(X, gid, ng, a, b, kmax, folds=lambda s: fold(name, s))


@functools.lru_cache(maxsize=None)
def expected_candidates(name, kmax) -> Loo:
    X, gid, ng, a, b = tpc.case(name)
    return restate_candidates(X, gid, ng, a, b, kmax, folds=lambda s: fold(name, s), full=tpc.expected(name))


FIELDS = ("gene_i", "gene_j", "num", "rank_num", "outcome", "side")


def same(x, y):
    """field by field, no tolerance: x, y a Loo or a TopPairsLoo"""
    return all(np.array_equal(getattr(x, f), getattr(y, f)) and getattr(x, f).dtype == getattr(y, f).dtype for f in FIELDS)


def gamma_decides_otherwise(name, kmax):
    """in how many folds of a named case the picks differ from those of the order "|N(s)|, then the FULL-data Gamma": there the fold's own
    rank shifts decide a pick, and decide it otherwise than the full data's would"""
    full, exp, folds = tpc.expected(name), expected(name, kmax), 0
    for s in np.flatnonzero(exp.side != 2):
        o = fold(name, int(s))
        gam = np.abs(full.D[o.gene_i] - full.D[o.gene_j])
        order = np.lexsort((o.gene_j, o.gene_i, -gam, -np.abs(o.num)))
        alt = o._replace(gene_i=o.gene_i[order], gene_j=o.gene_j[order])
        at = greedy(alt, kmax)
        folds += not (np.array_equal(alt.gene_i[at], exp.gene_i[s]) and np.array_equal(alt.gene_j[at], exp.gene_j[s]))
    return folds


def moved_fold(X, gid, genes, s, kmax):
    """fold s of a top_pairs_cases.moved_case (two groups, tie-free) from moved_oracle on the training columns, with a list deep enough to
    hold kmax disjoint pairs: (gene_i, gene_j, N, Gamma, outcome) of the picks"""
    cols = np.delete(np.arange(X.shape[1]), s)
    oi, oj, _, on, og, _ = tpc.moved_oracle(np.asfortranarray(X[:, cols]), gid[cols], genes, 8 * kmax)
    used, at = set(), []
    for e, (i, j) in enumerate(zip(oi.tolist(), oj.tolist())):
        if len(at) < kmax and i not in used and j not in used:
            used.update((i, j)); at.append(e)
    assert len(at) == kmax                                                       # deep enough
    return oi[at], oj[at], on[at], og[at], outcome_of(X, oi[at], oj[at], s)


def moved_expected(X, gid, genes, kmax):
    """the definition on a moved_case, every fold, plus the full-data cut.  The ranks and the comparisons of the pairs with a moved gene are
    made once for all folds (they do not depend on the labels); a fold sums them over its training columns.  moved_fold restates single
    folds through moved_oracle; the tests compare the two."""
    G, S = X.shape
    side = sides_of(gid, 2, 0, None)
    r = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        r[np.argsort(X[:, s], kind="stable"), s] = np.arange(G)
    w = 2 * r - G + 1
    pi, pj = [], []
    for g in genes:
        others = np.delete(np.arange(G), g)
        pi.append(np.minimum(others, g)); pj.append(np.maximum(others, g))
    pairs = np.unique(np.stack([np.concatenate(pi), np.concatenate(pj)], axis=1), axis=0)
    i, j = pairs[:, 0], pairs[:, 1]
    gt = X[i] > X[j]                                                             # tie-free: nothing is tied

    in_a, in_b = gid == 0, gid == 1
    w_a, w_b = w[:, in_a].sum(axis=1), w[:, in_b].sum(axis=1)
    gt_a, gt_b = gt[:, in_a].sum(axis=1, dtype=np.int64), gt[:, in_b].sum(axis=1, dtype=np.int64)
    head = 2048                                                                  # pairs of the order's head that are sorted: the walk must end inside

    def ordered(s):
        """the head of the order without column s (None: of the full data): every pair in front of the head's last one, sorted"""
        out_a, out_b = (s is not None and in_a[s]), (s is not None and in_b[s])
        s_a, s_b = int(in_a.sum()) - out_a, int(in_b.sum()) - out_b
        D = (w_a - (w[:, s] if out_a else 0)) * s_b - (w_b - (w[:, s] if out_b else 0)) * s_a
        num = (2 * (gt_a - (gt[:, s] if out_a else 0)) - s_a) * s_b - (2 * (gt_b - (gt[:, s] if out_b else 0)) - s_b) * s_a
        gam, mag = np.abs(D[i] - D[j]), np.abs(num)
        cut = np.partition(mag, mag.size - head)[mag.size - head]               # ties at the cut: those with the largest Gamma only
        at_cut = np.flatnonzero(mag == cut)
        if at_cut.size > head:
            g_cut = np.partition(gam[at_cut], at_cut.size - head)[at_cut.size - head]
            at_cut = at_cut[gam[at_cut] >= g_cut]
        sel = np.concatenate([np.flatnonzero(mag > cut), at_cut])
        order = sel[np.lexsort((j[sel], i[sel], -gam[sel], -mag[sel]))]
        return tpc.Oracle(i[order].astype(np.int32), j[order].astype(np.int32), None, num[order], gam[order], D, (s_a, s_b), None)

    gi, gj = np.full((S, kmax), -1, dtype=np.int32), np.full((S, kmax), -1, dtype=np.int32)
    num, gam, out = np.zeros((S, kmax), dtype=np.int64), np.zeros((S, kmax), dtype=np.int64), np.zeros((S, kmax), dtype=np.int8)
    for s in range(S):
        o = ordered(s)
        at = greedy(o, kmax)
        assert at.size == kmax and np.abs(o.num[at]).min() > 0                   # (no pair of fixed genes, which are not listed, can come first)
        gi[s], gj[s], num[s], gam[s] = o.gene_i[at], o.gene_j[at], o.num[at], o.rank_num[at]
        out[s] = outcome_of(X, o.gene_i[at], o.gene_j[at], s)
    full = ordered(None)
    at = greedy(full, 2 * kmax)
    assert at.size == 2 * kmax
    return Loo(gi, gj, num, gam, out, side, max(abs(int(full.num[at[-1]])) - 4 * max(full.sizes), 0), -1)
