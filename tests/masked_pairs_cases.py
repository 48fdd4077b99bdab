"""Cases for the masked build (reo_build_pairs_masked): a numpy restatement of its definition and the seeded case generators.  No
fixtures, no GPU.

The definition (include/reo_hip.h, "Missing values"): for every i < j and group g, over the samples of g in which both genes are valid,
n_g = their number, gt_g = those with x_i > x_j and not tied, eq_g = those tied -- under the comparator of the matrix's element type --,
nre_g = gt_g + tie_wins(seed, i, j, g, eq_g).  For comparison k: a = nre_k, n1 = n_k, b and n2 the sums over the other groups;
ic = 2 if n1 < min_complete[0], else 3 if a >= m(n1), else 1 if n1 - a >= m(n1), else 2 with m(n) = threshold(n, pval_reo); `it` likewise.
code(i, j) = 3 (ic - 1) + (it - 1), code(j, i) = 8 - code(i, j), 255 on the diagonal.

Vectorised per sample like oracle.reo_numpy.pair_counts; the coins are looped over the pairs with eq_g > 0 only."""
from __future__ import annotations

import functools

import numpy as np

import float32_cases as fc
from oracle import reo_numpy as rn


def masked_counts(X, V, gid, ngroups):
    """(n_gt, n_eq, n_avail) per ORDERED pair and group, G x G x ngroups int32.  A float32 matrix is compared in Float32 arithmetic
    (float32_cases.f32_ties), everything else after widening to Float64 (band 0.1; for integers: equality)."""
    X = np.asarray(X)
    V = np.asarray(V) != 0
    G, S = X.shape
    assert V.shape == X.shape
    n_gt = np.zeros((G, G, ngroups), dtype=np.int32)
    n_eq = np.zeros((G, G, ngroups), dtype=np.int32)
    n_av = np.zeros((G, G, ngroups), dtype=np.int32)
    f32 = X.dtype == np.float32
    X64 = X.astype(np.float64)
    for s in range(S):
        tie = fc.f32_ties(X[:, s]) if f32 else np.abs(X64[:, None, s] - X64[None, :, s]) < 0.1
        gt = (~tie) & (X64[:, None, s] > X64[None, :, s])
        v = V[:, None, s] & V[None, :, s]
        n_gt[:, :, gid[s]] += gt & v
        n_eq[:, :, gid[s]] += tie & v
        n_av[:, :, gid[s]] += v
    return n_gt, n_eq, n_av


@functools.lru_cache(maxsize=None)
def threshold_table(n_max: int, pval_reo: float) -> np.ndarray:
    """m(0 .. n_max) by oracle.reo_numpy.threshold, fallback branch included."""
    return np.array([rn.threshold(n, pval_reo) for n in range(n_max + 1)], dtype=np.int64)


def default_min_complete(sizes, k, pval_reo):
    """per side min(side size, n*), n* the smallest n with min(1, 2 * 0.5^n) < pval_reo"""
    n = 1
    while not min(1.0, 2.0 * 0.5 ** n) < pval_reo:
        n += 1
    s1 = int(sizes[k])
    return (min(s1, n), min(int(sizes.sum()) - s1, n))


def side_classes(a, n, m, min_complete):
    """the side rule, elementwise; also which pairs are unstable for being short and which for lacking a majority"""
    mn = m[n]
    short = n < min_complete
    cls = np.where(short, 2, np.where(a >= mn, 3, np.where(n - a >= mn, 1, 2)))
    return cls, short, (cls == 2) & ~short


def masked_codes(counts, k, pval_reo, min_complete, seed, detail=False):
    """The class table (G x G uint8, 255 on the diagonal) from masked_counts' output.  detail=True: also a dict with the boolean upper-
    triangle matrices short_c, short_t, nomaj_c, nomaj_t (why a side is class 2)."""
    n_gt, n_eq, n_av = counts
    G, _, ng = n_gt.shape
    up = n_gt.astype(np.int64)
    for i, j, g in np.argwhere(n_eq > 0):
        if i < j:
            up[i, j, g] += rn.tie_wins(seed, int(i), int(j), int(g), int(n_eq[i, j, g]))
    n = n_av.astype(np.int64)
    a, n1 = up[:, :, k], n[:, :, k]
    b, n2 = up.sum(axis=2) - a, n.sum(axis=2) - n1
    m = threshold_table(int(max(n1.max(), n2.max())), float(pval_reo))
    ic, short_c, nomaj_c = side_classes(a, n1, m, min_complete[0])
    it, short_t, nomaj_t = side_classes(b, n2, m, min_complete[1])
    c = (3 * (ic - 1) + (it - 1)).astype(np.int64)
    upper = np.triu(np.ones((G, G), dtype=bool), 1)
    code = np.where(upper, c, 0) + np.where(upper.T, 8 - c.T, 0)
    code[np.arange(G), np.arange(G)] = 255
    code = code.astype(np.uint8)
    if not detail:
        return code
    return code, {"short_c": short_c & upper, "short_t": short_t & upper, "nomaj_c": nomaj_c & upper, "nomaj_t": nomaj_t & upper}


def interleaved(n0: int, n1: int) -> np.ndarray:
    """labels of two groups of n0 and n1 samples, the columns interleaved as far as the smaller group reaches; group 0 comes first"""
    out, left = [], [n0, n1]
    while left[0] or left[1]:
        for g in (0, 1):
            if left[g]:
                out.append(g)
                left[g] -= 1
    return np.asarray(out, dtype=np.int32)


def random_mask(rng, G, S, frac):
    return rng.random((G, S)) >= frac


def float_case(G, sizes, frac, seed, shift=0.0, planted=0, decimals=2):
    """Float64 rounded to `decimals`: ties inside the 0.1 band are plentiful.  Planted effects: genes 4 .. 4 + planted - 1 are shifted up by
    `shift` in group 1, the next `planted` genes down.  Returns X, V, gid."""
    rng = np.random.default_rng(seed)
    gid = interleaved(*sizes) if len(sizes) == 2 else np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    S = int(gid.size)
    X = np.round(rng.normal(0.0, 1.0, size=(G, S)) + 0.8 * rng.normal(0.0, 1.0, size=(G, 1)), decimals)
    if planted:
        X[4: 4 + planted, gid == 1] += shift
        X[4 + planted: 4 + 2 * planted, gid == 1] -= shift
    return X, random_mask(rng, G, S, frac), gid


def special_rows(V, gid, rng):
    """the four special genes of the first GPU case, written into V in place: gene 0 never observed in group 0, gene 1 complete, gene 2
    observed in exactly 5 samples of group 0, gene 3 with the whole first 32-slot block of group 0 invalid"""
    ctrl = np.flatnonzero(gid == 0)
    V[0, ctrl] = False
    V[1, :] = True
    V[2, ctrl] = False
    V[2, rng.choice(ctrl, size=5, replace=False)] = True
    V[3, ctrl[:32]] = False
    V[3, ctrl[32:]] = True
    return V


def count_case(G, sizes, frac, seed, dtype=np.int64):
    """small counts with many equal values (ties by equality); as float32 the same cells"""
    rng = np.random.default_rng(seed)
    gid = interleaved(*sizes)
    S = int(gid.size)
    X = rng.poisson(rng.gamma(2.0, 2.0, size=(G, 1)), size=(G, S)).astype(dtype)
    return X, random_mask(rng, G, S, frac), gid


def rank_case(G, sizes, frac, seed, level=0.0, shift=0.0, planted=0):
    """tie-free: every sample a permutation of 0, 10, 20, ... (Float64).  level > 0: the permutations are the ranks of unit noise around
    gene levels of that spread, with the planted effects of float_case, so that stable and reversed pairs occur (level = 0: pure noise)"""
    rng = np.random.default_rng(seed)
    gid = interleaved(*sizes)
    S = int(gid.size)
    if level > 0.0:
        v = rng.normal(0.0, 1.0, size=(G, S)) + level * rng.normal(0.0, 1.0, size=(G, 1))
        v[4: 4 + planted, gid == 1] += shift
        v[4 + planted: 4 + 2 * planted, gid == 1] -= shift
        X = np.empty((G, S), dtype=np.float64)
        np.put_along_axis(X, np.argsort(v, axis=0, kind="stable"), 10.0 * np.arange(G, dtype=np.float64)[:, None], axis=0)
    else:
        X = np.stack([rng.permutation(G) for _ in range(S)], axis=1).astype(np.float64) * 10.0
    return X, random_mask(rng, G, S, frac), gid


FIRST_SEED = 0x5EED0B01


def first_case():
    """Float64, two groups 37 / 43 interleaved, G = 72, 25 % missing at random, six genes planted up and six down (the oracle's iteration
    on the restated table runs four passes and ends with nine DEGs), the four special genes.  X, V, gid, seed."""
    X, V, gid = float_case(72, (37, 43), 0.25, FIRST_SEED, shift=2.0, planted=6)
    special_rows(V, gid, np.random.default_rng(7))
    return X, V, gid, FIRST_SEED
