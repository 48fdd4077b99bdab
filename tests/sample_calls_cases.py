"""Cases for the sample calls (reo_sample_calls): the expected value everywhere is the host route that the package already has --
SampleTests.calls(pval_deg, padj_deg) and (SampleTests.padj() <= padj_deg).sum(0) -- and the comparison is an equality, not a tolerance:
both sides evaluate p * (n / r).  The data makers are those of tests/test_gpu_sample_tests.py, copied here so that that file stays as it
is.  No fixtures, no GPU."""
from __future__ import annotations

import numpy as np

THRESHOLDS = (0.0, 0.05, 0.2, 1.0)
TODAY = {"k", "result", "labels", "iters_run", "trace"}
FIELDS = ("genes", "calls", "cut", "n_up", "n_down")


def interleaved_33_37():
    labels = np.array(["a" if (s % 2 == 0 and s < 66) else "b" for s in range(70)], dtype=object)
    assert (labels == "a").sum() == 33 and (labels == "b").sum() == 37
    return labels


def tie_rich(G, S, seed, second):
    """small integers with gene levels and an effect in the samples `second` (bool over the samples): ties in every sample, stable pairs of
    both directions in the control group"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(G, 1)) + rng.integers(0, 3, size=(G, S))
    X[: G // 4, second] += 4
    X[G // 4: G // 2, second] -= 4
    X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)                  # every sample its own pattern: a swapped column shows
    return X.astype(np.int64)


def open_ctx(pkg, X, labels, pval_reo=0.1, seed=11, k=0, treat=None):
    ctx = pkg.Context(device=0, seed=seed)
    gid, lev = pkg.encode_groups(labels)
    ctx.set_groups(gid, len(lev))
    ctx.compute_thresholds(pval_reo)
    ctx.set_matrix(X)
    if treat is None:
        ctx.build_pairs(k)
    else:
        ctx.build_contrast(k, treat)
    return ctx


def expected(st, pval_deg, padj_deg):
    """(calls, cut, n_up, n_down) of the host route from a SampleTests"""
    calls = st.calls(pval_deg, padj_deg)
    cut = (st.padj() <= padj_deg).sum(axis=0).astype(np.int32)
    return calls, cut, (calls == 1).sum(axis=0).astype(np.int32), (calls == -1).sum(axis=0).astype(np.int32)


def same(got, st, pval_deg, padj_deg, tag=None):
    """a SampleCalls against the host route on the same tails, byte for byte; returns the expected calls and cuts"""
    calls, cut, n_up, n_down = expected(st, pval_deg, padj_deg)
    assert np.array_equal(got.genes, st.genes), tag
    assert got.calls.dtype == np.int8 and got.calls.shape == calls.shape, (tag, got.calls.shape, calls.shape)
    assert np.ascontiguousarray(got.calls).tobytes() == calls.tobytes(), (tag, pval_deg, padj_deg, np.argwhere(got.calls != calls)[:5].tolist())
    for name, exp in (("cut", cut), ("n_up", n_up), ("n_down", n_down)):
        g = getattr(got, name)
        assert g.dtype == np.int32 and np.array_equal(g, exp), (tag, name, pval_deg, padj_deg, g[:8].tolist(), exp[:8].tolist())
    return calls, cut


def bitwise(a, b):
    for f in FIELDS:
        x, y = np.ascontiguousarray(getattr(a, f)), np.ascontiguousarray(getattr(b, f))
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
