"""The generators and small helpers that the GPU tests of the query entry points share (tests/test_gpu_sample_counts.py,
test_gpu_sample_tests.py, test_gpu_pair_support.py).  No fixtures, no import of the package; a helper whose body differs in one of those
files is defined there."""
import numpy as np


def halves(S, ngroups=2):
    return np.array([f"g{min(s * ngroups // S, ngroups - 1)}" for s in range(S)], dtype=object)


def tie_rich(G, S, seed, second):
    """small integers with gene levels and an effect in the samples `second` (bool over the samples): every one of the nine classes occurs
    (asserted where it matters); greater, tied and smaller all occur"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(G, 1)) + rng.integers(0, 3, size=(G, S))
    X[: G // 4, second] += 4
    X[G // 4: G // 2, second] -= 4
    return X.astype(np.int64)


def code_rows(ctx, genes):
    return {int(i): ctx.get_codes(int(i), int(i) + 1, 0, ctx.G)[0] for i in set(np.asarray(genes).reshape(-1).tolist())}


def band_matrix(G, S, seed):
    """Float64 with many pairs near the 0.1 band, and planted pairs a hair inside and outside it"""
    rng = np.random.default_rng(seed)
    X = rng.normal(0.0, 0.4, size=(G, S)) + (np.arange(G)[:, None] % 5) * 0.3
    X[G // 3:, S // 2:] += 0.35
    for s in range(S):
        for k, d in enumerate((0.1 - 1e-12, 0.1 + 1e-12, float(np.nextafter(0.1, 0.0)), 0.1, float(np.nextafter(0.1, 1.0)))):
            X[2 * k + 1, s] = X[2 * k, s] + (d if s % 2 else -d)
    return np.asfortranarray(X)


def planted_ranks(G, S, seed, n_up=30, n_dn=30):
    """tie-free Int64, every sample a permutation of 0 .. G - 1: stable gene levels with a little noise, the first n_up genes far up and the
    next n_dn far down in the second half of the samples"""
    rng = np.random.default_rng(seed)
    v = 10.0 * rng.permutation(G)[:, None] + rng.integers(-12, 13, size=(G, S))
    v[:n_up, S // 2:] += 1200.0
    v[n_up:n_up + n_dn, S // 2:] -= 1200.0
    order = np.argsort(v, axis=0, kind="stable")
    X = np.empty((G, S), dtype=np.int64)
    np.put_along_axis(X, order, np.broadcast_to(np.arange(G, dtype=np.int64)[:, None], (G, S)), axis=0)
    return X
