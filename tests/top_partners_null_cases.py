"""Cases for the label-permutation null of a gene's best partner score (reo_top_partners_null): numpy restatements of its definition.  No
fixtures, no GPU.

The definition (include/reo_hip.h, "Label-permutation null of a gene's best partner score"): label rows as in top_pairs_null_cases.  Per
label row b and query row r with gene q, over the eligible partners p (p != q, inside partner_mask): |N_b(q, p)| from
top_pairs_null_cases.abs_num -- the diagonal excluded, the mask applied --, then the maximum, the FIRST partner that attains it (argmax over
p ascending) and the number of partners with |N| >= cuts[r].  No eligible partner: -1, -1 and 0.

  restate        from the G x G |N| of top_pairs_null_cases.abs_num, row by row
  from_counts    the same from the R x G x G counts of wide_top_pairs_cases.row_counts (the wide sample axes)
  query_restate  per query in O(G S), without G x G arrays (the plane-chain cases of top_pairs_cases.moved_case, and matrices of many genes)
  overall        identity I1: per label row the maximum over the query rows and the smallest (min(q, p), max(q, p)) that attains it"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import top_pairs_cases as tpc
import top_pairs_null_cases as tnc

NAMES = tnc.NAMES
B_MAX = tnc.B_MAX


class PNull(NamedTuple):
    max_num: np.ndarray      # int64, B x Q
    arg_partner: np.ndarray  # int32, B x Q
    n_reach: np.ndarray      # int32, B x Q (B x 0 without cuts)
    n_multi: int             # cells whose maximum more than one partner attains


def from_abs(n, genes, cuts=None, partner_mask=None):
    """one label row: (max, first partner, reach, cells with several partners at the maximum) per query from the G x G |N|"""
    G = n.shape[0]
    keep = np.ones(G, dtype=bool) if partner_mask is None else np.asarray(partner_mask, dtype=bool)
    Q = len(genes)
    mx, arg, reach, multi = np.full(Q, -1, np.int64), np.full(Q, -1, np.int32), np.zeros(Q, np.int32), 0
    for r, q in enumerate(genes):
        ok = keep.copy()
        ok[q] = False                                                            # the diagonal is no partner
        p = np.flatnonzero(ok)
        if p.size == 0:
            continue
        v = n[q, p]
        e = int(np.argmax(v))                                                    # p ascending: the first among equals
        mx[r], arg[r] = v[e], p[e]
        multi += int((v == v[e]).sum() > 1)
        if cuts is not None:
            reach[r] = int((v >= cuts[r]).sum())
    return mx, arg, reach, multi


def _stack(per_row, with_cuts) -> PNull:
    mx, arg, reach = (np.stack([t[k] for t in per_row]) for k in range(3))
    return PNull(mx, arg, reach if with_cuts else reach[:, :0], sum(t[3] for t in per_row))


def restate(X, rows, genes, cuts=None, partner_mask=None) -> PNull:
    rows = np.atleast_2d(np.asarray(rows))
    genes = np.asarray(genes).reshape(-1)
    return _stack([from_abs(tnc.abs_num(X, rows[b])[0], genes, cuts, partner_mask) for b in range(rows.shape[0])], cuts is not None)


def from_counts(counts, rows, genes, cuts=None, partner_mask=None) -> PNull:
    """`counts`: wide_top_pairs_cases.row_counts(X, rows)"""
    rows = np.atleast_2d(np.asarray(rows))
    gt_a, eq_a, gt_b, eq_b = counts
    out = []
    for b in range(rows.shape[0]):
        s_a, s_b = int((rows[b] == 1).sum()), int((rows[b] == 0).sum())
        n = np.abs((2 * gt_a[b] + eq_a[b] - s_a) * s_b - (2 * gt_b[b] + eq_b[b] - s_b) * s_a)
        out.append(from_abs(n, np.asarray(genes).reshape(-1), cuts, partner_mask))
    return _stack(out, cuts is not None)


def query_restate(X, rows, genes, cuts=None, partner_mask=None) -> PNull:
    """per (label row, query) in O(G S), without G x G arrays: the comparator of top_partners_cases.row_oracle (a float32 matrix in Float32
    arithmetic, everything else widened to Float64; tied inside the band 0.1) on row q against every gene"""
    X = np.asarray(X)
    rows = np.atleast_2d(np.asarray(rows))
    G = X.shape[0]
    B, Q = rows.shape[0], len(genes)
    keep = np.ones(G, dtype=bool) if partner_mask is None else np.asarray(partner_mask, dtype=bool)
    assert cuts is None or np.min(cuts) >= 0
    sides = [(rows[b] == 1, rows[b] == 0) for b in range(B)]
    mx, arg, reach, multi = np.full((B, Q), -1, np.int64), np.full((B, Q), -1, np.int32), np.zeros((B, Q), np.int32), 0
    X64 = X.astype(np.float64)
    for r, q in enumerate(genes):
        if X.dtype == np.float32:
            with np.errstate(invalid="ignore"):
                tie = np.abs(X[q][None, :] - X).astype(np.float64) < 0.1         # Float32 arithmetic
        else:
            tie = np.abs(X64[q][None, :] - X64) < 0.1
        gt = (~tie) & (X64[q][None, :] > X64)                                    # G x S: q above p
        ok = keep.copy()
        ok[q] = False                                                            # the diagonal is no partner
        if not ok.any():
            continue
        for b, (in_a, in_b) in enumerate(sides):
            s_a, s_b = int(in_a.sum()), int(in_b.sum())
            w_a = 2 * gt[:, in_a].sum(axis=1).astype(np.int64) + tie[:, in_a].sum(axis=1) - s_a
            w_b = 2 * gt[:, in_b].sum(axis=1).astype(np.int64) + tie[:, in_b].sum(axis=1) - s_b
            n = np.where(ok, np.abs(w_a * s_b - w_b * s_a), -1)                  # (a cut is not negative: an ineligible gene reaches none)
            e = int(np.argmax(n))                                                # p ascending: the first among equals
            mx[b, r], arg[b, r] = n[e], e
            multi += int((n == n[e]).sum() > 1)
            if cuts is not None:
                reach[b, r] = int((n >= cuts[r]).sum())
    return PNull(mx, arg, reach if cuts is not None else reach[:, :0], multi)


moved_restate = query_restate    # top_pairs_cases.moved_case is tie-free: nothing is tied there


def overall(max_num, arg_partner, genes):
    """I1: (max, i, j) per label row over the query rows; -1, -1, -1 where no row has a partner"""
    B = max_num.shape[0]
    out = []
    for b in range(B):
        top = int(max_num[b].max()) if max_num.shape[1] else -1
        if top < 0:
            out.append((-1, -1, -1))
            continue
        pairs = [(min(int(q), int(p)), max(int(q), int(p))) for q, p, m in zip(genes, arg_partner[b], max_num[b]) if m == top]
        out.append((top,) + min(pairs))
    return out


SEAM_QUERIES = (0, 63, 64, -1, 5, 5, 64)     # -1 stands for G - 1: seven rows (a padded row tile), repeats, both sides of a column tile seam


def seam_queries(G):
    return np.array([G - 1 if q < 0 else q for q in SEAM_QUERIES], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def cuts(name):
    """one cut per gene, from the observed row: 0, 1, the median |N| of the gene's row, the gene's observed maximum, 2 S_A S_B + 1 -- by
    gene index modulo 5"""
    X = tpc.case(name)[0]
    n, (s_a, s_b) = tnc.abs_num(X, tnc.rows(name)[0])
    G = n.shape[0]
    off = n.astype(np.int64).copy()
    np.fill_diagonal(off, -1)
    med = np.array([int(np.median(np.delete(n[g], g))) for g in range(G)])
    pick = np.stack([np.zeros(G, np.int64), np.ones(G, np.int64), med, off.max(axis=1), np.full(G, 2 * s_a * s_b + 1)], axis=1)
    c = pick[np.arange(G), np.arange(G) % 5].astype(np.int64)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name) -> PNull:
    """the restatement over the B_MAX rows of a named case, all genes as queries, with the cuts of `cuts`: computed once and shared,
    read-only.  Any list of queries is a selection of its columns: every row is decided on its own."""
    X = tpc.case(name)[0]
    return restate(X, tnc.rows(name), np.arange(X.shape[0]), cuts(name))


def select(exp: PNull, B, genes=None, with_cuts=True) -> PNull:
    cols = slice(None) if genes is None else np.asarray(genes)
    return PNull(exp.max_num[:B, cols], exp.arg_partner[:B, cols], exp.n_reach[:B, cols] if with_cuts else exp.n_reach[:B, :0], exp.n_multi)
