"""Cases for the top partners of a gene (reo_top_partners): two numpy restatements of a row of its answer.  No fixtures, no GPU.

The definition (include/reo_hip.h, "Top partners"): sides, counts, N, D and Gamma of top_pairs_cases.  For a query gene q and a partner
p != q inside partner_mask: the counts are those of "q above p", N_qp signed, Gamma_qp = |D_q - D_p| with D over ALL genes; the row is
ordered |N| descending, Gamma descending, p ascending.

  row_oracle   a row straight from the values, O(G S): the comparator of masked_pairs_cases.masked_counts (a float32 matrix in Float32
               arithmetic, everything else widened to Float64 with the band 0.1) on row q against every gene; D comes from outside.
  from_pairs   the same row as the subsequence of a top_pairs_cases.Oracle over the pairs that contain q, re-oriented to "q above p":
               where q is the larger gene gt becomes S_side - gt - eq and N changes its sign.
tests/test_top_partners_cpu.py holds the two to each other on every case of top_pairs_cases.EQUALITY."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class Row(NamedTuple):
    partner: np.ndarray    # int32, every eligible partner in the row's order
    counts: np.ndarray     # partners x 4: gt_A, eq_A, gt_B, eq_B of "q above p", int32
    num: np.ndarray        # N (signed, q against p), int64
    rank_num: np.ndarray   # Gamma, int64


def side_masks(gid, ngroups, a, b):
    gid = np.asarray(gid)
    in_a = gid == a
    in_b = (gid != a) & (gid >= 0) & (gid < ngroups) if b is None else gid == b
    return in_a, in_b


def row_oracle(X, gid, ngroups, a, b, D, q, partner_mask=None) -> Row:
    X = np.asarray(X)
    G = X.shape[0]
    in_a, in_b = side_masks(gid, ngroups, a, b)
    s_a, s_b = int(in_a.sum()), int(in_b.sum())
    if X.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            d = np.abs(X[q][None, :] - X)                                        # Float32 arithmetic, as float32_cases.f32_ties
        assert d.dtype == np.float32
        tie = d.astype(np.float64) < 0.1
    else:
        tie = np.abs(X[q].astype(np.float64)[None, :] - X.astype(np.float64)) < 0.1
    gt = (~tie) & (X[q].astype(np.float64)[None, :] > X.astype(np.float64))
    gt_a, eq_a = gt[:, in_a].sum(axis=1).astype(np.int64), tie[:, in_a].sum(axis=1).astype(np.int64)
    gt_b, eq_b = gt[:, in_b].sum(axis=1).astype(np.int64), tie[:, in_b].sum(axis=1).astype(np.int64)
    num = (2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a
    D = np.asarray(D, dtype=np.int64)
    gam = np.abs(D[q] - D)
    keep = np.ones(G, dtype=bool) if partner_mask is None else np.asarray(partner_mask, dtype=bool).copy()
    keep[q] = False
    p = np.flatnonzero(keep)
    order = p[np.lexsort((p, -gam[p], -np.abs(num[p])))]                         # (the last key is the primary one)
    counts = np.stack([gt_a[order], eq_a[order], gt_b[order], eq_b[order]], axis=1).astype(np.int32)
    return Row(order.astype(np.int32), counts, num[order], gam[order])


def from_pairs(oracle, q, partner_mask=None) -> Row:
    """`oracle`: a top_pairs_cases.Oracle over ALL pairs (no gene mask); the partner mask filters the partners only"""
    s_a, s_b = oracle.sizes
    has = (oracle.gene_i == q) | (oracle.gene_j == q)
    gi, gj, c, num, gam = oracle.gene_i[has], oracle.gene_j[has], oracle.counts[has].astype(np.int64), oracle.num[has], oracle.rank_num[has]
    flip = gj == q                                                               # q is the larger gene: the oracle holds "p above q"
    p = np.where(flip, gi, gj)
    counts = c.copy()
    counts[flip, 0] = s_a - c[flip, 0] - c[flip, 1]
    counts[flip, 2] = s_b - c[flip, 2] - c[flip, 3]
    num = np.where(flip, -num, num)
    if partner_mask is not None:
        keep = np.asarray(partner_mask, dtype=bool)[p]
        p, counts, num, gam = p[keep], counts[keep], num[keep], gam[keep]
    return Row(p.astype(np.int32), counts.astype(np.int32), num.astype(np.int64), gam.astype(np.int64))


def same(x: Row, y: Row) -> bool:
    return all(np.array_equal(u, v) for u, v in zip(x, y))


def table(rows, m):
    """(partner, counts, num, rank_num, n_found) of a list of Rows as the library pads them: Q x m, -1 / 0 beyond n_found"""
    Q = len(rows)
    partner = np.full((Q, m), -1, dtype=np.int32)
    counts = np.zeros((Q, m, 4), dtype=np.int32)
    num, gam = np.zeros((Q, m), dtype=np.int64), np.zeros((Q, m), dtype=np.int64)
    found = np.zeros(Q, dtype=np.int32)
    for r, row in enumerate(rows):
        n = min(m, row.partner.size)
        found[r] = n
        partner[r, :n], counts[r, :n], num[r, :n], gam[r, :n] = row.partner[:n], row.counts[:n], row.num[:n], row.rank_num[:n]
    return partner, counts, num, gam, found


def check_table(tp, rows, m):
    """assert field by field that a TopPartners equals the padded table of `rows`"""
    partner, counts, num, gam, found = table(rows, m)
    assert tp.partner.shape == (len(rows), m) and tp.partner.dtype == np.int32
    assert np.array_equal(tp.n_found, found), (tp.n_found, found)
    assert np.array_equal(tp.partner, partner)
    assert np.array_equal(tp.n_gt, counts[:, :, 0::2]) and tp.n_gt.dtype == np.int32
    assert np.array_equal(tp.n_eq, counts[:, :, 1::2]) and tp.n_eq.dtype == np.int32
    assert np.array_equal(tp.num, num) and tp.num.dtype == np.int64
    assert np.array_equal(tp.rank_num, gam) and tp.rank_num.dtype == np.int64
