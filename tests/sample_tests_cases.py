"""Cases for the sample tests (reo_sample_tests): the exact hypergeometric tails in Python integers, the tolerance that the library's
arithmetic is held to, and the expected integers from the numpy restatement of tests/sample_counts_cases.py.  No fixtures, no GPU.

The 2 x 2 table of one (gene, sample) cell is [[a, b], [u, d]] (include/reo_hip.h): N = a + b + u + d, K = a + u, n = u + d,
X ~ Hypergeometric(N, K, n), p_up = P(X >= u), p_down = P(X <= u).  The weights C(K, x) C(N - K, n - x) are formed as Python integers by
the exact integer ratio recurrence from math.comb at the lower end of the support, and a tail is an integer sum over C(N, n): rounded
once, where it becomes a float.

Tolerance.  MEASURED_REL_ERR is the largest relative error of csrc/sample_tests.h, built for the host by g++ against glibc's exp, over
the tables of tests/sample_tests_driver.cpp (degenerate tables and the seeded grid), per background size |J| <= 12, 70, 300, 4 200; a
tail whose exact value lies below 2^-900 is not measured (it must lie below 2^-890 instead).  The tests assert 4 x that figure: the
margin covers another libm's exp and the device's.  The error is that of the log-factorial table: its entries near N carry half an ulp
of log N!, and nine of them make up log pmf(u)."""
from __future__ import annotations

import math

import numpy as np

import sample_counts_cases as scc

MASK_ABOVE, MASK_BELOW = 0x1C0, 0x007

# the largest relative error measured on the CPU (tests/test_sample_tests_cpu.py prints the figures it finds), by background size
MEASURED_REL_ERR = {12: 7.2e-15, 70: 1.4e-13, 300: 5.6e-13, 4200: 1.12e-11}   # measured: 7.11e-15, 1.38e-13, 5.56e-13, 1.120e-11
MARGIN = 4.0
UNDERFLOW_EXACT_LOG2, UNDERFLOW_RESULT = -900, 2.0 ** -890


def tolerance(background: int) -> float:
    """the asserted bound for tables whose background |J| = a + b is at most `background`: 4 x the measured error of the smallest
    measured size that covers it"""
    for size in sorted(MEASURED_REL_ERR):
        if background <= size:
            return MARGIN * MEASURED_REL_ERR[size]
    raise ValueError(f"no measured tolerance for a background of {background}")


def exact_tails(a: int, b: int, u: int, d: int):
    """(up, down, total): integers with p_up = up / total and p_down = down / total, exactly.  n = 0: (1, 1, 1)."""
    a, b, u, d = int(a), int(b), int(u), int(d)
    N, K, n = a + b + u + d, a + u, u + d
    if n == 0:
        return 1, 1, 1
    M = N - K
    lo, hi = max(0, n - M), min(n, K)
    assert lo <= u <= hi
    total = math.comb(N, n)                                                    # Vandermonde: the weights sum to C(N, n)
    wu = w = math.comb(K, u) * math.comb(M, n - u)
    if hi - u <= u - lo:                                                       # the side with fewer terms is summed, the other follows
        up = w
        for x in range(u, hi):
            w, r = divmod(w * (K - x) * (n - x), (x + 1) * (M - n + x + 1))
            assert r == 0
            up += w
        down = total - up + wu
    else:
        down = w
        for x in range(u, lo, -1):
            w, r = divmod(w * x * (M - n + x), (K - x + 1) * (n - x + 1))
            assert r == 0
            down += w
        up = total - down + wu
    assert 0 < up <= total and 0 < down <= total
    return up, down, total


def rel_err(got: float, num: int, den: int) -> float:
    """|got - num / den| / (num / den) without forming the quotient first (num > 0)"""
    p, q = float(got).as_integer_ratio()
    return abs(p * den - num * q) / (num * q)


def below_two_to(num: int, den: int, log2: int) -> bool:
    """num / den < 2^log2 (log2 < 0), in integers"""
    return (num << -log2) < den


def judge(got: float, num: int, den: int):
    """("underflow", ok) for an exact value below 2^-900 -- the result must lie below 2^-890 -- else ("value", relative error)"""
    if below_two_to(num, den, UNDERFLOW_EXACT_LOG2):
        return "underflow", bool(0.0 <= got < UNDERFLOW_RESULT)
    return "value", rel_err(got, num, den)


def check_tails(p_up, p_down, a, b, u, d, tol, tag=None) -> float:
    """asserts both tails of every cell against the exact ones under `tol`; p_up, p_down, u, d: equal shapes, a, b: broadcastable.
    Equal tables are judged once.  Returns the largest relative error met."""
    p_up, p_down, u, d = (np.asarray(v) for v in (p_up, p_down, u, d))
    a, b = np.broadcast_to(np.asarray(a), u.shape), np.broadcast_to(np.asarray(b), u.shape)
    worst, seen = 0.0, {}
    for idx in np.ndindex(u.shape):
        key = (int(a[idx]), int(b[idx]), int(u[idx]), int(d[idx]))
        got = (float(p_up[idx]), float(p_down[idx]))
        if key in seen:
            assert seen[key] == got, (tag, key)                                # the same table, the same bits
            continue
        seen[key] = got
        up, down, total = exact_tails(*key)
        for name, g, num in (("p_up", got[0], up), ("p_down", got[1], down)):
            kind, v = judge(g, num, total)
            if kind == "underflow":
                assert v, (tag, name, key, g)
            else:
                assert v <= tol, (tag, name, key, g, v, tol)
                worst = max(worst, v)
    return worst


def expected_integers(X, codes_of_row, genes, partner_mask, st=None):
    """what reo_sample_tests reports besides the tails, from the restatement of the comparators and the two class masks:
    dict(n_above_ctrl, n_below_ctrl, rev_up, rev_down, tied, u, d), int32 / int64 arrays"""
    genes = np.asarray(genes, dtype=np.int64).reshape(-1)
    gt, eq = st if st is not None else scc.states(X, genes)
    out = {}
    sel = {}
    for name, mask in (("A", MASK_ABOVE), ("B", MASK_BELOW)):
        s = np.stack([scc.selection(codes_of_row(int(i)), mask, partner_mask) for i in genes])
        assert not s[np.arange(genes.size), genes].any()
        sel[name] = scc.counts_of(gt, eq, s)
    (na, gta, eqa), (nb, gtb, eqb) = sel["A"], sel["B"]
    out["n_above_ctrl"], out["n_below_ctrl"] = na, nb
    out["rev_up"] = gtb
    out["rev_down"] = (na[:, None] - gta - eqa).astype(np.int32)
    out["tied"] = (eqa + eqb).astype(np.int32)
    out["u"] = gta.astype(np.int64) + gtb
    out["d"] = (na + nb).astype(np.int64)[:, None] - out["u"] - out["tied"]
    return out
