"""Cases for the label-permutation null of the best pair score (reo_top_pairs_null): a numpy restatement of its definition and the seeded
row generators.  No fixtures, no GPU.

The definition (include/reo_hip.h, "Label-permutation null of the best score"): a label row holds 1 on side A, 0 on side B and 2 on the
samples that take no part.  Per row, the counts of top_pairs_cases.side_counts on the RELABELLED groups gid_p -- 0 where the row is 1, 1
where it is 0, 2 where it is 2 --, N = w(A) S_B - w(B) S_A, and over the pairs i < j inside gene_mask: max |N|, the first (i, j) that
attains it, and the number of pairs with |N| >= each cut.  No eligible pair: -1, -1, -1 and 0."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import top_pairs_cases as tpc

B_MAX = 33                                                                       # rows of the shared expectation; its tests use the first B
NAMES = ["float300", "count_i64", "count_f32", "rank130", "three_0_2", "three_1_rest", "level", "separated"]


class Null(NamedTuple):
    max_num: np.ndarray    # int64, B
    arg_i: np.ndarray      # int32, B
    arg_j: np.ndarray      # int32, B
    n_reach: np.ndarray    # int64, B x len(cuts)


def observed_row(gid, a, b):
    """the label row of the observed groups: uint8, 1 = group a, 0 = group b (None: every other sample), 2 = neither"""
    gid = np.asarray(gid)
    return np.where(gid == a, 1, 0 if b is None else np.where(gid == b, 0, 2)).astype(np.uint8)


def relabel(row):
    """gid_p of a label row: side A is group 0, side B group 1, the rest group 2"""
    row = np.asarray(row)
    return np.where(row == 1, 0, np.where(row == 0, 1, 2)).astype(np.int32)


def abs_num(X, row):
    """|N| of every ordered pair under a label row, G x G int64, and the sides' sizes"""
    gt_a, eq_a, gt_b, eq_b, s_a, s_b = tpc.side_counts(X, relabel(row), 3, 0, 1)
    return np.abs((2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a), (s_a, s_b)


def restate(X, rows, cuts=(), gene_mask=None) -> Null:
    rows = np.atleast_2d(np.asarray(rows))
    G = np.asarray(X).shape[0]
    iu, ju = np.triu_indices(G, 1)                                               # (i, j) ascending: argmax finds the first among equals
    if gene_mask is not None:
        keep = np.asarray(gene_mask, dtype=bool)
        sel = keep[iu] & keep[ju]
        iu, ju = iu[sel], ju[sel]
    cuts = np.asarray(cuts, dtype=np.int64).reshape(-1)
    B = rows.shape[0]
    out = Null(np.full(B, -1, np.int64), np.full(B, -1, np.int32), np.full(B, -1, np.int32), np.zeros((B, cuts.size), np.int64))
    for p in range(B):
        if iu.size == 0:
            continue
        n = abs_num(X, rows[p])[0][iu, ju]
        e = int(np.argmax(n))
        out.max_num[p], out.arg_i[p], out.arg_j[p] = n[e], iu[e], ju[e]
        out.n_reach[p] = (n[None, :] >= cuts[:, None]).sum(axis=1)
    return out


def shuffled_rows(obs, B, seed):
    """B label rows: row 0 the observed one, the others seeded shuffles of it among the samples that take part (the 2s stay)"""
    obs = np.asarray(obs, dtype=np.uint8)
    rng = np.random.default_rng(seed)
    part = np.flatnonzero(obs != 2)
    rows = np.tile(obs, (B, 1))
    for p in range(1, B):
        rows[p, part] = rng.permutation(obs[part])
    return rows


@functools.lru_cache(maxsize=None)
def rows(name):
    """the B_MAX label rows of a named case of top_pairs_cases, built once and shared: treat as read-only"""
    _, gid, _, a, b = tpc.case(name)
    r = shuffled_rows(observed_row(gid, a, b), B_MAX, 100 + NAMES.index(name))
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def cuts(name):
    """[0, 1, median |N|, observed max, 2 S_A S_B, 2 S_A S_B + 1] of a named case, from the observed row"""
    X = tpc.case(name)[0]
    n, (s_a, s_b) = abs_num(X, rows(name)[0])
    n = n[np.triu_indices(n.shape[0], 1)]
    return np.array([0, 1, int(np.median(n)), int(n.max()), 2 * s_a * s_b, 2 * s_a * s_b + 1], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def expected(name) -> Null:
    """the restatement over the B_MAX rows and the six cuts of a named case, computed once and shared: treat as read-only"""
    return restate(tpc.case(name)[0], rows(name), cuts(name))


def first(null: Null, B) -> Null:
    return Null(null.max_num[:B], null.arg_i[:B], null.arg_j[:B], null.n_reach[:B])


def moved_rows(gid, seed):
    """three rows for top_pairs_cases.moved_case (two groups): observed, inverted as far as the sizes allow it (the first min(S_A, S_B)
    samples of either side change places by hand; the sizes are kept), and one shuffle"""
    obs = observed_row(gid, 0, None)
    inv = obs.copy()
    ia, ib = np.flatnonzero(obs == 1), np.flatnonzero(obs == 0)
    m = min(ia.size, ib.size)
    inv[ia[:m]], inv[ib[:m]] = 0, 1
    return np.stack([obs, inv, shuffled_rows(obs, 2, seed)[1]])


def moved_expected(X, row, genes):
    """(max |N|, i, j) under a label row for a moved_case without G x G arrays: on that data only pairs with a moved gene can have N != 0
    under any labelling, so the maximum is theirs -- asserted positive, and equal to what top_pairs_cases.moved_oracle gives for the
    relabelled groups -- and the pair is the smallest (i, j) among those that attain it."""
    G = X.shape[0]
    a, b = row == 1, row == 0
    s_a, s_b = int(a.sum()), int(b.sum())
    best = (-1, -1, -1)
    for g in genes:
        others = np.delete(np.arange(G), g)
        i, j = np.minimum(others, g), np.maximum(others, g)
        gt = X[i] > X[j]                                                         # tie-free: nothing is tied
        n = np.abs((2 * gt[:, a].sum(axis=1).astype(np.int64) - s_a) * s_b - (2 * gt[:, b].sum(axis=1).astype(np.int64) - s_b) * s_a)
        for e in np.flatnonzero(n == n.max()):
            cand = (int(n[e]), int(i[e]), int(j[e]))
            if cand[0] > best[0] or (cand[0] == best[0] and cand[1:] < best[1:]):
                best = cand
    assert best[0] > 0 and best[0] == abs(int(tpc.moved_oracle(X, relabel(row), genes, 1)[3][0]))
    return best
