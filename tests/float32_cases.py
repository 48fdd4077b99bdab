"""Cases for Float32 expression matrices (reo_set_matrix_f32): seeded generators and the numpy restatement of the reference's
comparator evaluated in Float32.  No fixtures, no GPU.

is_greater(x::Float32, y::Float32) (src/RankCompV3.jl:71-77) forms abs(x - y) in Float32 and compares it with the Float64 literal
0.1.  Float32(0.1) = 0.100000001490116... is not below 0.1, so a pair whose exact difference lies in [0.09999999776, 0.1) and
rounds up to Float32(0.1) is "not tied" in Float32 and "tied" after widening to Float64.  Wherever x - y is exact in Float32 the
two arithmetics agree.
"""
from __future__ import annotations

import numpy as np


def f32_ties(x: np.ndarray) -> np.ndarray:
    """Tie matrix of one sample in Float32 arithmetic: [i, j] = (double)fabsf(x_i - x_j) < 0.1.  The cast is explicit, so numpy's
    scalar promotion rules play no part."""
    x = np.asarray(x)
    assert x.dtype == np.float32
    with np.errstate(invalid="ignore"):   # Inf - Inf = NaN: not tied
        d = np.abs(x[:, None] - x[None, :])
    assert d.dtype == np.float32
    return d.astype(np.float64) < 0.1


def f64_ties(x: np.ndarray) -> np.ndarray:
    """The same sample widened: the comparator in Float64 arithmetic (what oracle.pair_counts evaluates)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.abs(x[:, None] - x[None, :]) < 0.1


def f32_pair_counts(X: np.ndarray, gid, ngroups: int):
    """Deterministic (n_gt, n_eq) per ORDERED pair and group, G x G x ngroups, of a float32 matrix compared in Float32 arithmetic:
    np.abs(X[:, None, s] - X[None, :, s]).astype(np.float64) < 0.1 on the float32 array, else x_i > x_j (:72-76 without the coin).
    The Float32 twin of oracle.reo_numpy.pair_counts."""
    X = np.asarray(X)
    assert X.dtype == np.float32 and X.ndim == 2
    G, S = X.shape
    n_gt = np.zeros((G, G, ngroups), dtype=np.int32)
    n_eq = np.zeros((G, G, ngroups), dtype=np.int32)
    for s in range(S):
        tie = f32_ties(X[:, s])
        gt = (~tie) & (X[:, None, s] > X[None, :, s])
        n_gt[:, :, gid[s]] += gt
        n_eq[:, :, gid[s]] += tie
    return n_gt, n_eq


def disagreements(X: np.ndarray):
    """(comparisons (i < j, sample) on which the Float32 and the Float64 comparator disagree about "tied", how many of those are
    Float32 "not tied" where Float64 says "tied", comparisons in all).  Greater-than cannot differ where the ties agree: widening
    keeps the order."""
    X = np.asarray(X)
    G, S = X.shape
    upper = np.triu(np.ones((G, G), dtype=bool), 1)
    n = one_way = 0
    for s in range(S):
        t32, t64 = f32_ties(X[:, s]), f64_ties(X[:, s])
        diff = (t32 != t64) & upper
        n += int(diff.sum())
        one_way += int((diff & ~t32 & t64).sum())
    return n, one_way, G * (G - 1) // 2 * S


def _flip_pair(rng):
    """One pair (x, y) of float32 numbers that Float32 calls not tied and Float64 tied, or None: y uniform in (-0.09, 0.09), x starts
    at float32(y + 0.1) and walks by nextafter (at most 6 steps) until the Float64 difference is < 0.1 while the Float32 one is >= 0.1."""
    y = np.float32(rng.uniform(-0.09, 0.09))
    x = np.float32(np.float64(y) + 0.1)
    for _ in range(7):
        d64 = np.float64(x) - np.float64(y)
        d32 = np.float64(np.float32(x - y))
        if d64 < 0.1 and d32 >= 0.1:
            return x, y
        x = np.nextafter(x, np.float32(-np.inf if d64 >= 0.1 else np.inf))
    return None


def planted(G: int, S: int, per_column: int, seed: int) -> np.ndarray:
    """float32 G x S: a normal(0, 1) background in which every column has `per_column` planted pairs (2 per_column distinct genes) on
    which the two arithmetics disagree.  About a fifth of the draws hit; a column draws until it has its pairs."""
    assert 2 * per_column <= G
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((G, S)).astype(np.float32)
    for s in range(S):
        genes = rng.permutation(G)[: 2 * per_column]
        k = 0
        while k < per_column:
            p = _flip_pair(rng)
            if p is None:
                continue
            X[genes[2 * k], s], X[genes[2 * k + 1], s] = p
            k += 1
    return X


def exact_grid(G: int, S: int, seed: int, n_inf: int = 6) -> np.ndarray:
    """float32 G x S of values k / 64, |k| < 2^17, plus a few +-Inf: every difference is exact in Float32 and in Float64, so the two
    arithmetics agree on every pair.  Ties (|dk| <= 6) are plentiful: half of the values come from a narrow range."""
    rng = np.random.default_rng(seed)
    wide = rng.integers(-(1 << 17) + 1, 1 << 17, size=(G, S))
    narrow = rng.integers(-max(8, 2 * G), max(8, 2 * G) + 1, size=(G, S)).clip(-(1 << 17) + 1, (1 << 17) - 1)
    k = np.where(rng.random((G, S)) < 0.5, narrow, wide)
    X = (k / 64.0).astype(np.float32)
    assert np.array_equal(X.astype(np.float64) * 64.0, k)
    for q in range(min(n_inf, G * S)):
        X[int(rng.integers(0, G)), int(rng.integers(0, S))] = np.float32(np.inf if q % 2 else -np.inf)
    return X


def f32_build_codes(X, gid, ngroups, k, thr, seed, tie_wins):
    """REO class codes of comparison k (src/RankCompV3.jl:363-392; 0..8 per ordered pair, 255 on the diagonal) from the Float32 counts:
    the counts of f32_pair_counts, the keyed tie coins (`tie_wins`, the oracle's), the rule of :376-377,385-386 -- assembled as
    oracle.reo_numpy.build_codes assembles them."""
    n_gt, n_eq = f32_pair_counts(X, gid, ngroups)
    G = n_gt.shape[0]
    sizes = np.bincount(gid, minlength=ngroups)
    s1, s2 = int(sizes[k]), int(sizes.sum() - sizes[k])
    code = np.full((G, G), 255, dtype=np.uint8)
    for i in range(G):
        for j in range(i + 1, G):
            nre = [int(n_gt[i, j, g]) + (tie_wins(seed, i, j, g, int(n_eq[i, j, g])) if n_eq[i, j, g] else 0) for g in range(ngroups)]
            a, b = nre[k], sum(nre) - nre[k]
            ic = 3 if a >= thr[0] else (1 if s1 - a >= thr[0] else 2)
            it = 3 if b >= thr[1] else (1 if s2 - b >= thr[1] else 2)
            c = 3 * (ic - 1) + (it - 1)
            code[i, j] = c
            code[j, i] = 8 - c
    return code
