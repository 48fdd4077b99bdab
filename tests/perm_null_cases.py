"""Cases for the label-permutation null (reo_perm_null, reo_perm_codes): a numpy restatement of its definition, of the word packing, and the
seeded case generators.  No fixtures, no GPU.

The definition (include/reo_hip.h, "Label-permutation null"): a permutation is a row of S bytes, 1 = side A.  For every i < j, over the
samples of side A: gt_A = those with x_i > x_j and not tied, eq_A = those tied; likewise side B.  a = gt_A + tie_wins(seed, i, j, 0, eq_A),
b = gt_B + tie_wins(seed, i, j, 1, eq_B); ic = 3 if a >= m1, else 1 if n1 - a >= m1, else 2; `it` likewise from b, n2, m2;
code(i, j) = 3 (ic - 1) + (it - 1), code(j, i) = 8 - code(i, j), 255 on the diagonal."""
from __future__ import annotations

import numpy as np

import masked_pairs_cases as mpc
from oracle import reo_numpy as rn


def permuted_codes(X, row, thr, seed):
    """The class table of one permutation (G x G uint8, 255 on the diagonal), restated from the definition: sides by `row`, coins keyed by
    side 0 / 1, thresholds thr = (m1, m2)."""
    X = np.asarray(X)
    row = np.asarray(row).astype(np.int64)
    side = 1 - row                                               # 0 = A, 1 = B: the coin's key
    n_gt, n_eq, n_av = mpc.masked_counts(X, np.ones(X.shape, dtype=bool), side.astype(np.int32), 2)
    G = X.shape[0]
    up = n_gt.astype(np.int64)
    for i, j, s in np.argwhere(n_eq > 0):
        if i < j:
            up[i, j, s] += rn.tie_wins(seed, int(i), int(j), int(s), int(n_eq[i, j, s]))
    n1, n2 = int(row.sum()), int(row.size - row.sum())
    a, b = up[:, :, 0], up[:, :, 1]
    ic = np.where(a >= thr[0], 3, np.where(n1 - a >= thr[0], 1, 2))
    it = np.where(b >= thr[1], 3, np.where(n2 - b >= thr[1], 1, 2))
    c = (3 * (ic - 1) + (it - 1)).astype(np.int64)
    upper = np.triu(np.ones((G, G), dtype=bool), 1)
    code = np.where(upper, c, 0) + np.where(upper.T, 8 - c.T, 0)
    code[np.arange(G), np.arange(G)] = 255
    return code.astype(np.uint8)


def relabelled(X, row):
    """The relabelled two-group problem of one permutation: group ids 1 - row.  The library wants its group ids numbered in order of first
    appearance, so the columns are put side A first (a stable sort; a class table does not depend on the order of the columns inside a
    side: counts are sums over the side's samples and the coins are keyed by pair, side and tie count).  Returns X2, gid2."""
    gid = (1 - np.asarray(row)).astype(np.int32)
    order = np.argsort(gid, kind="stable")
    return np.asfortranarray(np.asarray(X)[:, order]), gid[order]


def slot_map(gid, ngroups):
    """sc_slot_map of csrc/sample_counts.h: the caller's column of every sample slot, groups padded to whole blocks of 32, -1 for padding"""
    gid = np.asarray(gid)
    out = []
    for g in range(ngroups):
        cols = np.flatnonzero(gid == g)
        pad = (-cols.size) % 32
        out += cols.tolist() + [-1] * pad
    return np.asarray(out, dtype=np.int32)


def pack_words(rows, gid, ngroups):
    """(A-words [B][blocks], live words [blocks]) of label rows under the slot map of `gid`: bit s of block b = slot 32 b + s"""
    m = slot_map(gid, ngroups)
    nblk = m.size // 32
    rows = np.asarray(rows)
    live = np.zeros(nblk, dtype=np.uint32)
    aw = np.zeros((rows.shape[0], nblk), dtype=np.uint32)
    for t, col in enumerate(m):
        if col < 0:
            continue
        live[t // 32] |= np.uint32(1 << (t % 32))
        aw[rows[:, col] == 1, t // 32] |= np.uint32(1 << (t % 32))
    return aw, live


def case(G, sizes, kind, seed, dtype=np.float64, **kw):
    """X (Fortran order), gid: `ties` = Float64 rounded to two decimals (ties inside the 0.1 band on both sides), `ranks` = every sample a
    permutation (tie-free), `counts` = small counts with equality ties in `dtype`; further keywords go to the generator"""
    if kind == "ranks":
        X, _, gid = mpc.rank_case(G, sizes, 0.0, seed, **kw)
    elif kind == "counts":
        X, _, gid = mpc.count_case(G, sizes, 0.0, seed, dtype=dtype)
    else:
        X, _, gid = mpc.float_case(G, sizes, 0.0, seed, **kw)
        X = X.astype(dtype)
    return np.asfortranarray(X), gid


def shuffled_rows(gid, k, n_perm, seed):
    """n_perm label rows with the ones of gid == k shuffled (plain numpy; repeats and the observed row may occur)"""
    rng = np.random.default_rng(seed)
    obs = (np.asarray(gid) == k).astype(np.uint8)
    return np.stack([rng.permutation(obs) for _ in range(n_perm)])
