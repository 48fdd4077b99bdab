"""Cases for the top-scoring-pair search (reo_top_pairs, reo_rank_shift): a numpy restatement of its definition and the seeded case
generators.  No fixtures, no GPU.

The definition (include/reo_hip.h, "Top-scoring pairs"): side A = the samples of group a, side B = those of group b or, for b None, every
other sample.  Per ordered pair and side, gt = samples with x_i above x_j and not tied, eq = tied samples -- under the comparator of the
matrix's element type, masked_pairs_cases.masked_counts with an all-ones mask --, w = gt - lt = 2 gt + eq - S_side.
N_ij = w(A) S_B - w(B) S_A;  W_i(side) = sum_j (gt_ij - gt_ji), D_i = W_i(A) S_B - W_i(B) S_A, Gamma_ij = |D_i - D_j|.
The order over i < j, both inside gene_mask: |N| descending, Gamma descending, i ascending, j ascending."""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import masked_pairs_cases as mpc


class Oracle(NamedTuple):
    gene_i: np.ndarray     # every eligible pair, in the order of the definition
    gene_j: np.ndarray
    counts: np.ndarray     # pairs x 4: gt_A, eq_A, gt_B, eq_B
    num: np.ndarray        # N (signed), int64
    rank_num: np.ndarray   # Gamma, int64
    D: np.ndarray          # G, int64
    sizes: tuple           # (S_A, S_B)
    N: np.ndarray          # G x G, int64 (for the antisymmetry check)


def side_counts(X, gid, ngroups, a, b):
    """(gt_A, eq_A, gt_B, eq_B, S_A, S_B): G x G int64 per ordered pair"""
    gid = np.asarray(gid)
    n_gt, n_eq, _ = mpc.masked_counts(X, np.ones(np.asarray(X).shape, dtype=bool), gid, ngroups)
    n_gt, n_eq = n_gt.astype(np.int64), n_eq.astype(np.int64)
    rest = [g for g in range(ngroups) if g != a] if b is None else [b]
    s_a, s_b = int((gid == a).sum()), int(np.isin(gid, rest).sum())
    return n_gt[:, :, a], n_eq[:, :, a], n_gt[:, :, rest].sum(axis=2), n_eq[:, :, rest].sum(axis=2), s_a, s_b


def oracle(X, gid, ngroups, a=0, b=None, gene_mask=None) -> Oracle:
    gt_a, eq_a, gt_b, eq_b, s_a, s_b = side_counts(X, gid, ngroups, a, b)
    G = gt_a.shape[0]
    N = (2 * gt_a + eq_a - s_a) * s_b - (2 * gt_b + eq_b - s_b) * s_a
    w_a, w_b = gt_a.sum(axis=1) - gt_a.sum(axis=0), gt_b.sum(axis=1) - gt_b.sum(axis=0)   # (the diagonal is tied: it adds to neither)
    D = w_a * s_b - w_b * s_a
    iu, ju = np.triu_indices(G, 1)
    if gene_mask is not None:
        keep = np.asarray(gene_mask, dtype=bool)
        sel = keep[iu] & keep[ju]
        iu, ju = iu[sel], ju[sel]
    num, gam = N[iu, ju], np.abs(D[iu] - D[ju])
    order = np.lexsort((ju, iu, -gam, -np.abs(num)))                             # (the last key is the primary one)
    iu, ju = iu[order], ju[order]
    counts = np.stack([gt_a[iu, ju], eq_a[iu, ju], gt_b[iu, ju], eq_b[iu, ju]], axis=1).astype(np.int32)
    return Oracle(iu.astype(np.int32), ju.astype(np.int32), counts, num[order], gam[order], D, (s_a, s_b), N)


def separated_case(seed=15):
    """G = 200, groups 33 / 31 interleaved, tie-free Float64: genes 0 .. 59 lie below every other gene in group 0 and above every other gene
    in group 1, so 60 x 140 = 8 400 pairs reach |N| = 2 S_A S_B and Gamma alone orders them."""
    rng = np.random.default_rng(seed)
    gid = mpc.interleaved(33, 31)
    G, S, m = 200, int(gid.size), 60
    X = np.empty((G, S), dtype=np.float64)
    for s in range(S):
        low, high = rng.permutation(m), rng.permutation(G - m)
        if gid[s] == 0:
            X[:m, s], X[m:, s] = low, m + high
        else:
            X[:m, s], X[m:, s] = (G - m) + low, high
    return X * 10.0, gid


def level_case():
    """Int64, X[g, s] = g // 10, G = 100, 12 / 12: every key is (0, 0)"""
    gid = mpc.interleaved(12, 12)
    X = np.tile((np.arange(100, dtype=np.int64) // 10)[:, None], (1, int(gid.size)))
    return X, gid


def _two(case):
    X, _, gid = case
    return X, gid


# name -> (X, gid, ngroups, a, b); the matrix in the dtype it goes to the library in
def _build(name):
    if name == "float300":
        X, gid = _two(mpc.float_case(300, (33, 31), 0.0, 11, shift=2.0, planted=20))
        return X, gid, 2, 0, None
    if name in ("count_i64", "count_i32", "count_f32"):
        X, gid = _two(mpc.count_case(200, (40, 24), 0.0, 12))
        return X.astype({"count_i64": np.int64, "count_i32": np.int32, "count_f32": np.float32}[name]), gid, 2, 0, None
    if name == "rank130":
        X, gid = _two(mpc.rank_case(130, (1, 20), 0.0, 13))
        return X, gid, 2, 0, None
    if name in ("three_1_rest", "three_0_2"):
        X, gid = _two(mpc.float_case(150, (20, 33, 12), 0.0, 14, shift=2.0, planted=10))
        return (X, gid, 3, 1, None) if name == "three_1_rest" else (X, gid, 3, 0, 2)
    if name == "separated":
        X, gid = separated_case()
        return X, gid, 2, 0, None
    if name == "level":
        X, gid = level_case()
        return X, gid, 2, 0, None
    raise KeyError(name)


EQUALITY = ["float300", "count_i64", "count_i32", "count_f32", "rank130", "three_1_rest", "three_0_2", "separated", "level"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(X, gid, ngroups, a, b) of a named case, built once and shared: treat as read-only"""
    X, gid, ng, a, b = _build(name)
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X, gid, ng, a, b


@functools.lru_cache(maxsize=None)
def expected(name) -> Oracle:
    """the oracle of a named case, computed once and shared: treat as read-only"""
    X, gid, ng, a, b = case(name)
    if name == "count_i32":                                                      # (Int32 goes up widened to Int64: the same cells, the same rule)
        return expected("count_i64")
    return oracle(X, gid, ng, a, b)


def moved_case(G, seed, moved=6, sizes=(5, 4)):
    """A case for gene counts whose full oracle would be too large (the 15- and 16-plane chains: G above 4 095 and above 32 767), tie-free
    Float64.  Every gene g holds 10 g in every sample -- the same order everywhere, N = 0 between any two of them -- except `moved` genes,
    which sit at a place of their own in every sample: near the bottom in group 0 and near the top in group 1, or the other way round.
    Only pairs with a moved gene can have N != 0, and the oracle counts exactly those.  Returns X, gid, the moved genes."""
    rng = np.random.default_rng(seed)
    gid = mpc.interleaved(*sizes)
    S = int(gid.size)
    X = np.tile(10.0 * np.arange(G, dtype=np.float64)[:, None], (1, S))
    genes = np.sort(rng.choice(np.arange(64, G - 64), size=moved, replace=False))
    genes[0], genes[-1] = 63, G - 1                                              # a tile's last column and the last gene among them
    for q, g in enumerate(genes):
        low = rng.integers(0, G // 8, size=S)
        high = rng.integers(G - G // 8, G, size=S)
        place = np.where((gid == 0) == (q % 2 == 0), low, high)
        X[g, :] = 10.0 * place + 1.0 + q                                         # between two fixed genes, and never on another moved gene
    return np.asfortranarray(X), gid, genes


def moved_oracle(X, gid, genes, n):
    """(gene_i, gene_j, counts, N, Gamma) of the first n pairs and D of every gene for a moved_case, exact: D from the ranks (tie-free:
    above - below = 2 r - G + 1), the counts of the pairs with a moved gene from the values, every other pair at N = 0."""
    G, S = X.shape
    a, b = gid == 0, gid == 1
    s_a, s_b = int(a.sum()), int(b.sum())
    r = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        r[np.argsort(X[:, s], kind="stable"), s] = np.arange(G)
    w = 2 * r - G + 1
    D = w[:, a].sum(axis=1) * s_b - w[:, b].sum(axis=1) * s_a
    fixed = np.ones(G, dtype=bool)
    fixed[genes] = False
    assert (np.diff(X[fixed], axis=0) > 0).all()                                 # the fixed genes keep one order: N = 0 among them
    pi, pj = [], []
    for g in genes:
        others = np.delete(np.arange(G), g)
        pi.append(np.minimum(others, g)); pj.append(np.maximum(others, g))
    pairs = np.unique(np.stack([np.concatenate(pi), np.concatenate(pj)], axis=1), axis=0)
    i, j = pairs[:, 0], pairs[:, 1]
    gt = X[i] > X[j]                                                             # tie-free: nothing is tied
    gt_a, gt_b = gt[:, a].sum(axis=1).astype(np.int64), gt[:, b].sum(axis=1).astype(np.int64)
    num = (2 * gt_a - s_a) * s_b - (2 * gt_b - s_b) * s_a
    gam = np.abs(D[i] - D[j])
    order = np.lexsort((j, i, -gam, -np.abs(num)))[:n]
    assert np.abs(num[order]).min() > 0                                          # the first n all have N != 0: no pair of fixed genes among them
    z = np.zeros(n, dtype=np.int64)
    counts = np.stack([gt_a[order], z, gt_b[order], z], axis=1).astype(np.int32)
    return i[order].astype(np.int32), j[order].astype(np.int32), counts, num[order], gam[order], D


def half_mask(G, seed=5):
    return np.random.default_rng(seed).random(G) < 0.5


def key_lines(exp: Oracle, G):
    """the oracle's pairs as the text the driver's select mode reads: |N| Gamma i j per line, in (i, j) order -- not in the answer's"""
    o = np.lexsort((exp.gene_j, exp.gene_i))
    return "".join(f"{abs(int(n))} {int(g)} {int(i)} {int(j)}\n" for n, g, i, j in zip(exp.num[o], exp.rank_num[o], exp.gene_i[o], exp.gene_j[o]))
