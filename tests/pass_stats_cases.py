"""Cases for the six statistics of a pass (pval, padj, delta1, delta2, se, z1): an exact restatement of McCullagh's test on the 3 x 3
table of nine tallies (the reference's :225-259) and of the end of a pass (:409-416: trimmed standard deviation, normal p-value,
Benjamini-Hochberg) in mpmath at 50 digits, the tolerances that the library's arithmetic is held to, and the inputs.  No fixtures, no GPU.

The final columns 0, 1 and 11..14 of identify_degs are a function of the last pass's nine tallies per gene (columns 2..10), which other
tests pin bit for bit: so the reference here starts from tallies and needs neither the oracle nor the iteration.

Tolerance.  MEASURED_REL_ERR holds the largest error of a plain float64 restatement of the same formulas (closed_form_f64, pass_f64:
numpy, math.erfc, glibc's log) against the exact values, by quantity and bucket; tests/test_pass_stats_cpu.py measures it afresh, prints
it and asserts that it stays inside what is recorded.  The GPU tests assert MARGIN = 4 x these figures: the margin covers another libm's
and the device's log / erfc / sqrt.  How each quantity is judged (judge_*):
  p, padj, se     relative error; an exact p below 2^-1000 is not measured: the result must lie in [0, 2^-990) instead;
  delta2          relative error where |delta2| > 1e-3, else the absolute error (against 1);
  delta1          |got - exact| / (|t1| + |t2|), the two log terms of :248-249, which may cancel;
  z1              the same with the scale divided by the exact se.
Buckets: kappa = a d / |det N| (<= 10, <= 1e3, <= 1e6, above) for everything that comes out of the 2 x 2 system, and |z| (<= 2, <= 8,
<= 20, <= 38.4) for a p-value, whose error grows like z^2 times that of z."""
from __future__ import annotations

import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()                                                         # a context of its own: nobody else's precision changes
MP.dps = 50

KAPPA_BUCKETS = (10.0, 1e3, 1e6, math.inf)
Z_BUCKETS = (2.0, 8.0, 20.0, 38.4)
MARGIN = 4.0
UNDERFLOW_EXACT, UNDERFLOW_RESULT = MP.mpf(2) ** -1000, 2.0 ** -990
DELTA2_ABS_BELOW = 1e-3

# The largest errors measured on the CPU (tests/test_pass_stats_cpu.py prints what it finds and asserts that it stays inside these).
# "table": closed_form_f64 over tables(1) and over the tallies of the whole runs, keyed (quantity, kappa bucket) and, for the test's own
# p-value, (p, kappa bucket, |z| bucket); nothing falls into the bucket above 1e6 (kappa < 2.63e5 while a row sums to 262 142 at most).
# "pass": pass_f64 over the whole runs, p and padj keyed by |z| bucket, and the trimmed standard deviation, which the library does not
# return.  "pass_blocks": the same with the slice's moments per block and Chan's combination (pass_blocks_f64).
MEASURED_REL_ERR = {
    "table": {
        ("delta1", 10.0): 1.17e-14, ("delta1", 1e3): 9.2e-15, ("delta1", 1e6): 4.1e-14,     # measured: 1.16e-14, 9.14e-15, 4.02e-14
        ("z1", 10.0): 1.17e-14, ("z1", 1e3): 9.2e-15, ("z1", 1e6): 4.1e-14,                 # measured: 1.16e-14, 9.14e-15, 4.03e-14
        ("delta2", 10.0): 1.9e-13, ("delta2", 1e3): 1.21e-13, ("delta2", 1e6): 1.5e-13,     # measured: 1.85e-13, 1.20e-13, 1.47e-13
        ("se", 10.0): 3.6e-16, ("se", 1e3): 3.3e-16, ("se", 1e6): 2.7e-16,                  # measured: 3.54e-16, 3.25e-16, 2.61e-16
        ("p", 10.0, 2.0): 8.0e-15, ("p", 10.0, 8.0): 1.2e-13, ("p", 10.0, 20.0): 3.3e-13, ("p", 10.0, 38.4): 8.3e-13,   # 7.98e-15, 1.19e-13, 3.24e-13, 8.26e-13
        ("p", 1e3, 2.0): 1.35e-14, ("p", 1e3, 8.0): 4.1e-14, ("p", 1e3, 20.0): 2.4e-13, ("p", 1e3, 38.4): 3.6e-13,      # 1.32e-14, 4.00e-14, 2.38e-13, 3.56e-13
        ("p", 1e6, 2.0): 1.8e-14, ("p", 1e6, 8.0): 1.1e-13, ("p", 1e6, 20.0): 2.85e-13, ("p", 1e6, 38.4): 6.0e-13,      # 1.76e-14, 1.09e-13, 2.80e-13, 5.99e-13
    },
    "pass": {
        ("p", 2.0): 1.95e-14, ("p", 8.0): 2.7e-14, ("p", 20.0): 1.4e-13, ("p", 38.4): 2.25e-13,            # measured: 1.92e-14, 2.69e-14, 1.38e-13, 2.24e-13
        ("padj", 2.0): 1.15e-14, ("padj", 8.0): 2.7e-14, ("padj", 20.0): 1.4e-13, ("padj", 38.4): 2.25e-13,    # 1.14e-14, 2.69e-14, 1.38e-13, 2.24e-13
        ("se",): 1.8e-16,                                                                                   # 1.78e-16
    },
    "pass_blocks": {
        ("p", 2.0): 1.95e-14, ("p", 8.0): 2.7e-14, ("p", 20.0): 9.1e-14, ("p", 38.4): 1.5e-13,             # measured: 1.92e-14, 2.69e-14, 9.00e-14, 1.45e-13
        ("padj", 2.0): 1.1e-14, ("padj", 8.0): 2.7e-14, ("padj", 20.0): 9.1e-14, ("padj", 38.4): 1.5e-13,  # 1.07e-14, 2.69e-14, 9.01e-14, 1.45e-13
        ("se",): 1.8e-16,                                                                                   # 1.78e-16
    },
}


def bucket(value: float, edges) -> float:
    for e in edges:
        if value <= e:
            return e
    raise ValueError(f"{value} lies above every bucket of {edges}")


# ------------------------------------------------------------------------------------------------------------ the exact reference

class Exact:
    """what exact_mccullagh returns: mp numbers delta1, delta2, se, z1, scale = |t1| + |t2|, kappa, and p = erfc(|z1| / sqrt 2), which is
    evaluated when it is first asked for; singular: the (1, 0, 0, 0, 0) of :243"""
    __slots__ = ("_p", "delta1", "delta2", "se", "z1", "scale", "kappa", "singular")

    def __init__(self, delta1, delta2, se, z1, scale, kappa, singular):
        self._p, self.delta1, self.delta2, self.se, self.z1, self.scale, self.kappa, self.singular = None, delta1, delta2, se, z1, scale, kappa, singular

    @property
    def p(self):
        if self._p is None:
            self._p = MP.mpf(1) if self.singular else MP.erfc(abs(self.z1) / SQRT2)   # :255
        return self._p


SQRT2, ZERO = MP.sqrt(2), MP.mpf(0)


def system_of(cont9):
    """(a, b, d, R1, R2, det) as Python integers (:230-240 for k = 3)"""
    n11, n12, n13, n21, n22, n23, n31, n32, n33 = (int(v) for v in cont9)
    a, b, d = n12 + n13 + n21 + n31, n13 + n31, n13 + n23 + n31 + n32
    return a, b, d, n12 + n13, n13 + n23, a * d - b * b


def exact_mccullagh(cont9) -> Exact:
    """:225-259 for a 3 x 3 table.  N = [[a b][b d]], omega2 = inv(N) (a, d) = (m1, m2) / det with m1 = d (a - b), m2 = a (d - b).
    Everything rational stays in Python integers and becomes an mp number by one division: nu = 1 / (a w1 + d w2) = det / (a m1 + d m2),
    the weights a w1 nu = a m1 / (a m1 + d m2) and d w2 nu, the arguments (2 R + 1) / (2 (n - R) + 1) of the logarithms, and
    (0.5 + w . R) / (0.5 + w . (n - R)) = (det + 2 (m1 R1 + m2 R2)) / (det + 2 (m1 (a - R1) + m2 (d - R2))).
    A zero pivot (det = 0 with b = 0) is the reference's own singular branch; the other integer-singular tables (a = b = d > 0) are
    refused: they follow the float elimination of the oracle by design and have their own tests."""
    a, b, d, R1, R2, det = system_of(cont9)
    f = MP.mpf
    if det == 0:
        if b != 0:
            raise ValueError(f"integer-singular table with b = {b} > 0: not this module's business")
        return Exact(ZERO, ZERO, ZERO, ZERO, ZERO, ZERO, True)
    m1, m2 = d * (a - b), a * (d - b)
    s = a * m1 + d * m2
    nu = f(det) / s                                                            # :247
    t1 = f(a * m1) / s * MP.log(f(2 * R1 + 1) / (2 * (a - R1) + 1)) if m1 else ZERO   # :248-249
    t2 = f(d * m2) / s * MP.log(f(2 * R2 + 1) / (2 * (d - R2) + 1)) if m2 else ZERO
    d1 = t1 + t2
    d2 = MP.log(f(det + 2 * (m1 * R1 + m2 * R2)) / (det + 2 * (m1 * (a - R1) + m2 * (d - R2))))   # :250
    se = MP.sqrt(nu * (4 + (d1 * d1 + d2 * d2) / 2))                           # :251-253: (v1 + v2) / 2 with v = 4 (1 + delta^2 / 4) nu
    return Exact(d1, d2, se, d1 / se, abs(t1) + abs(t2), f(a * d) / abs(det), False)


def exact_mccullagh_general(mat):
    """:225-259 for any k x k table, with the inverse of N solved at 50 digits: (p, delta1, delta2, se, z1).  Only to tie the closed form
    above to the reference's known answer (a 4 x 4 table) and to the general formula on 3 x 3 tables."""
    mat = [[int(v) for v in row] for row in mat]
    k, m = len(mat), len(mat) - 1
    N = MP.zeros(m, m)
    for i in range(m):
        for j in range(i, m):
            N[i, j] = N[j, i] = sum(mat[x][y] + mat[y][x] for x in range(i + 1) for y in range(j + 1, k))
    R = [sum(mat[x][y] for x in range(i + 1) for y in range(i + 1, k)) for i in range(m)]
    n = MP.matrix([N[i, i] for i in range(m)])
    w2 = MP.lu_solve(N, n)
    nu = 1 / sum(n[i] * w2[i] for i in range(m))
    d1 = sum(n[i] * w2[i] * nu * MP.log((R[i] + MP.mpf(0.5)) / (n[i] - R[i] + 0.5)) for i in range(m))
    d2 = MP.log((0.5 + sum(w2[i] * R[i] for i in range(m))) / (0.5 + sum(w2[i] * (n[i] - R[i]) for i in range(m))))
    se = MP.sqrt((4 * (1 + d1 * d1 / 4) * nu + 4 * (1 + d2 * d2 / 4) * nu) / 2)
    z1 = d1 / se
    return MP.erfc(abs(z1) / SQRT2), d1, d2, se, z1


def slice_bounds(G: int):
    """round(Int, G * 0.05), round(Int, G * 0.95): 1-based, inclusive, half to even on the Float64 product (:411)"""
    return int(np.rint(G * 0.05)), int(np.rint(G * 0.95))


def exact_bh(p):
    """:413 on mp numbers: ascending order, p G / r, reverse cumulative minimum, clamp to 1"""
    G = len(p)
    order = sorted(range(G), key=lambda i: p[i])
    out, run = [None] * G, None
    for r in range(G, 0, -1):
        v = p[order[r - 1]] * G / r
        run = v if run is None or v < run else run
        out[order[r - 1]] = run if run < 1 else MP.mpf(1)
    return out


def exact_trimmed_std(values):
    """:409-411 on mp numbers: the n - 1 standard deviation of sort(values)[a : b]"""
    G = len(values)
    a, b = slice_bounds(G)
    assert 1 <= a <= b <= G
    sl = sorted(values)[a - 1: b]
    mean = MP.fsum(sl) / len(sl)
    return MP.sqrt(MP.fsum((v - mean) ** 2 for v in sl) / (len(sl) - 1))


def exact_pass(cont, rows=None):
    """:409-416 from the tallies [G, 9]: dict(delta1, se, p, padj) of mp numbers (se: one number).  `rows`: the exact_mccullagh of every
    gene, if the caller has them.  erfc is evaluated once per distinct |delta1|."""
    rows = rows if rows is not None else exact_rows(cont)
    d1 = [r.delta1 for r in rows]
    se = exact_trimmed_std(d1)
    assert se > 0
    scale, memo, p = 1 / (se * SQRT2), {}, []
    for v in d1:
        v = abs(v)
        if v not in memo:
            memo[v] = MP.erfc(v * scale)
        p.append(memo[v])
    return {"delta1": d1, "se": se, "p": p, "padj": exact_bh(p)}


def exact_rows(cont):
    """exact_mccullagh of every row, equal rows evaluated once"""
    memo, out = {}, []
    for row in np.asarray(cont).astype(np.int64).tolist():
        key = tuple(row)
        if key not in memo:
            memo[key] = exact_mccullagh(key)
        out.append(memo[key])
    return out


# ------------------------------------------------------------------------------------------------------------------------ judging

def _mp(x: float):
    return MP.mpf(float(x))


def judge_p(got: float, exact):
    """("underflow", ok) for an exact value below 2^-1000 -- the result must lie in [0, 2^-990) -- else ("value", relative error)"""
    if exact < UNDERFLOW_EXACT:
        return "underflow", bool(0.0 <= got < UNDERFLOW_RESULT)
    return "value", float(abs(_mp(got) - exact) / exact)


def judge_rel(got: float, exact) -> float:
    return float(abs(_mp(got) - exact) / abs(exact))


def judge_delta2(got: float, exact) -> float:
    err = abs(_mp(got) - exact)
    return float(err / abs(exact)) if abs(exact) > DELTA2_ABS_BELOW else float(err)


def judge_scaled(got: float, exact, scale) -> float:
    """delta1: scale = |t1| + |t2|; z1: that over the exact se.  Both log terms exactly zero: the result must be zero."""
    if scale == 0:
        return 0.0 if got == 0.0 else math.inf
    return float(abs(_mp(got) - exact) / scale)


def judge_table_row(got5, ex: Exact, with_p: bool = True) -> dict:
    """errors of one (p, delta1, delta2, se, z1) row against exact_mccullagh, by quantity; p: ("underflow", ok) or ("value", err)"""
    return {"p": judge_p(got5[0], ex.p) if with_p else None, "delta1": judge_scaled(got5[1], ex.delta1, ex.scale), "delta2": judge_delta2(got5[2], ex.delta2),
            "se": judge_rel(got5[3], ex.se), "z1": judge_scaled(got5[4], ex.z1, ex.scale / ex.se)}


class Worst:
    """the largest figure per key, for printing and recording"""

    def __init__(self):
        self.v = {}

    def add(self, key, err: float):
        self.v[key] = max(self.v.get(key, 0.0), err)

    def show(self) -> str:
        return "{" + ", ".join(f"{k!r}: {v:.2e}" for k, v in sorted(self.v.items(), key=lambda kv: repr(kv[0]))) + "}"


def measure_table(out5, cont, rows=None, worst=None, tol=None, tag=None, with_p=True):
    """judges rows of (p, delta1, delta2, se, z1) against exact_mccullagh of `cont`: the largest error by ("se", kappa bucket) ...
    ("p", kappa bucket, |z| bucket).  With `tol` (a function of the key) every figure is asserted on the spot; the underflow class is
    asserted by its bound always.  Singular rows must be (1, 0, 0, 0, 0) exactly.  with_p = False: the first column is not the test's own
    p-value (a pass overwrites it, :415) and is left alone.  Returns (Worst, number of underflow rows)."""
    rows = rows if rows is not None else exact_rows(cont)
    worst = worst if worst is not None else Worst()
    under = 0
    for i, ex in enumerate(rows):
        got = [float(v) for v in out5[i]]
        if ex.singular:
            assert got[1 - with_p:] == [1.0, 0.0, 0.0, 0.0, 0.0][1 - with_p:], (tag, i, got)
            continue
        kb = bucket(float(ex.kappa), KAPPA_BUCKETS)
        j = judge_table_row(got, ex, with_p)
        kind, v = j.pop("p") or ("skip", None)
        if kind == "skip":
            pass
        elif kind == "underflow":
            assert v, (tag, "p", i, list(cont[i]), got[0])
            under += 1
        else:
            j[("p", bucket(abs(float(ex.z1)), Z_BUCKETS))] = v
        for name, err in j.items():
            key = (name, kb) if isinstance(name, str) else (name[0], kb, name[1])
            if tol is not None:
                assert err <= tol(key), (tag, key, i, list(cont[i]), got, err, tol(key))
            worst.add(key, err)
    return worst, under


def measure_pass(p, padj, cont, ex_pass, worst=None, tol=None, tag=None):
    """judges the p and padj columns of a pass against exact_pass: the largest relative error by ("p" | "padj", |z| bucket) with
    z = delta1 / se exact.  Returns (Worst, number of underflow genes)."""
    worst = worst if worst is not None else Worst()
    under, se = 0, ex_pass["se"]
    for i in range(len(ex_pass["p"])):
        z = abs(ex_pass["delta1"][i]) / se
        is_under = ex_pass["p"][i] < UNDERFLOW_EXACT
        under += is_under
        zb = None if is_under else bucket(float(z), Z_BUCKETS)
        for name, got, exact in (("p", float(p[i]), ex_pass["p"][i]), ("padj", float(padj[i]), ex_pass["padj"][i])):
            kind, v = judge_p(got, exact)
            if kind == "underflow":
                assert v, (tag, name, i, list(cont[i]), got)
                continue
            key = (name, zb if zb is not None else Z_BUCKETS[-1])              # (padj of an underflowing p that a larger p determines)
            if tol is not None:
                assert v <= tol(key), (tag, key, i, list(cont[i]), got, v, tol(key))
            worst.add(key, v)
    return worst, under


def tolerance(kind: str):
    """the asserted bound as a function of the key: MARGIN x the recorded figure"""
    table = MEASURED_REL_ERR[kind]

    def tol(key):
        if key not in table:
            raise ValueError(f"no measured figure for {kind} {key}")
        return MARGIN * table[key]
    return tol


# ------------------------------------------------------------------------------------------------- plain float64 restatements

def closed_form_f64(cont) -> np.ndarray:
    """the closed form in ordinary double arithmetic, [n, 5] = (p, delta1, delta2, se, z1); singular rows (1, 0, 0, 0, 0).  Only to
    measure what double arithmetic delivers: it is not the code under test."""
    cont = np.asarray(cont).astype(np.int64).reshape(-1, 9)
    out = np.zeros((cont.shape[0], 5))
    for i, row in enumerate(cont.tolist()):
        a, b, d, R1, R2, det = system_of(row)
        if det == 0:
            out[i, 0] = 1.0
            continue
        fa, fd, r1, r2 = float(a), float(d), float(R1), float(R2)
        w1, w2 = float(d * (a - b)) / float(det), float(a * (d - b)) / float(det)
        nu = 1.0 / (fa * w1 + fd * w2)
        d1 = (fa * w1 * nu) * math.log((r1 + 0.5) / (fa - r1 + 0.5)) + (fd * w2 * nu) * math.log((r2 + 0.5) / (fd - r2 + 0.5))
        d2 = math.log((0.5 + (w1 * r1 + w2 * r2)) / (0.5 + (w1 * (fa - r1) + w2 * (fd - r2))))
        se = math.sqrt((4.0 * (1.0 + 0.25 * d1 * d1) * nu + 4.0 * (1.0 + 0.25 * d2 * d2) * nu) * 0.5)
        z1 = d1 / se
        out[i] = (min(1.0, math.erfc(abs(z1) * math.sqrt(0.5))), d1, d2, se, z1)
    return out


def bh_f64(p: np.ndarray) -> np.ndarray:
    G = len(p)
    order = np.argsort(p, kind="stable")
    adj = np.minimum.accumulate((p[order] * (G / np.arange(1, G + 1)))[::-1])[::-1]
    out = np.empty(G)
    out[order] = np.minimum(adj, 1.0)
    return out


def pass_f64(delta1: np.ndarray):
    """the end of a pass in ordinary double arithmetic: sort, two-pass standard deviation of the slice, math.erfc, BH -> (se, p, padj)"""
    G = len(delta1)
    a, b = slice_bounds(G)
    sl = np.sort(delta1)[a - 1: b]
    mean = sl.sum() / len(sl)
    se = math.sqrt(((sl - mean) ** 2).sum() / (len(sl) - 1))
    p = np.array([min(1.0, math.erfc(abs(v) / se * math.sqrt(0.5))) for v in delta1.tolist()])
    return se, p, bh_f64(p)


def pass_blocks_f64(delta1: np.ndarray, chunk: int = 1024, block: int = 16):
    """the same with the slice's moments formed the way the library forms them: the genes in chunks of 1 024 by index, every chunk
    sorted, (count, mean, M2) of the slice's members among every 16 consecutive elements of a sorted chunk, and the blocks combined by
    Chan's rule (mean = sum n_b mean_b / n, M2 = sum [M2_b + n_b (mean_b - mean)^2]; numpy's pairwise sums stand for the device's
    butterflies) -> (se, p, padj)"""
    G = len(delta1)
    a, b = slice_bounds(G)
    rank = np.empty(G, dtype=np.int64)
    rank[np.argsort(delta1, kind="stable")] = np.arange(G)
    nb, mb, qb = [], [], []
    for c0 in range(0, G, chunk):
        idx = c0 + np.argsort(delta1[c0: c0 + chunk], kind="stable")
        for e0 in range(0, len(idx), block):
            g = idx[e0: e0 + block]
            x = delta1[g][(rank[g] >= a - 1) & (rank[g] <= b - 1)]
            m = x.sum() / len(x) if len(x) else 0.0
            nb.append(float(len(x))); mb.append(m); qb.append(((x - m) * (x - m)).sum())
    nb, mb, qb = np.array(nb), np.array(mb), np.array(qb)
    n = nb.sum()
    mean = (nb * mb).sum() / n
    se = math.sqrt((qb + nb * (mb - mean) * (mb - mean)).sum() / (n - 1.0))
    p = np.array([min(1.0, math.erfc(abs(v) / se * math.sqrt(0.5))) for v in delta1.tolist()])
    return se, p, bh_f64(p)


# ----------------------------------------------------------------------------------------------------------------- the inputs

TALLY_SUM_MAX = 262142                                                         # a gene's tallies sum to nref - 1 <= 262 143 - 1


def _fit(rows: np.ndarray) -> np.ndarray:
    """scales rows whose sum exceeds TALLY_SUM_MAX down to it (integer division of every cell)"""
    rows = rows.astype(np.int64)
    s = rows.sum(axis=1)
    over = s > TALLY_SUM_MAX
    rows[over] = rows[over] * TALLY_SUM_MAX // s[over, None]
    return rows


def _z_of(row) -> float:
    return abs(float(closed_form_f64([row])[0, 4]))


def tables(seed: int) -> np.ndarray:
    """about 3 000 tally rows [n, 9] int32 for Context.mccullagh, every row's sum <= 262 142, none integer-singular:
    six magnitudes with a quarter of the cells zeroed; R1 = 0, R1 = a, R2 = 0, R2 = d; near-singular rows (n13, n31 large, n12, n21,
    n23 small: kappa to 2.6e5, the most that a sum of 262 142 allows, so the bucket above 1e6 stays empty); rows whose |z1| steps through 1 ... several hundred (p crosses the subnormal range and
    underflows).  Some rows are repeated: equal rows must give equal bits."""
    rng = np.random.default_rng(seed)
    rows = []
    for mag in (3, 40, 400, 5000, 60000, 262000):                              # 6 x 300
        r = rng.integers(0, mag + 1, size=(300, 9))
        r[rng.random(r.shape) < 0.25] = 0
        rows.append(_fit(r))
    edge = rng.integers(0, 300, size=(400, 9))                                 # R1 = n12 + n13, a - R1 = n21 + n31, R2 = n13 + n23, d - R2 = n31 + n32
    edge[0:100, [1, 2]] = 0                                                    # R1 = 0 (then n13 = 0: R2 = n23)
    edge[100:200, [3, 6]] = 0                                                  # R1 = a
    edge[200:300, [2, 5]] = 0                                                  # R2 = 0
    edge[300:400, [6, 7]] = 0                                                  # R2 = d
    rows.append(edge)
    near = rng.integers(0, 50, size=(700, 9))                                  # near-singular: a, d barely above b
    near[:, 2] = rng.integers(1000, 100001, size=700)
    near[:, 6] = rng.integers(1000, 100001, size=700)
    near[:, [1, 3, 5]] = rng.integers(0, 3, size=(700, 3))
    near[:, 7] = rng.integers(0, 3, size=700) + (near[:, [1, 3, 5]].sum(axis=1) == 0)   # (never all four zero: that is a = b = d)
    near[400:450, 2] = rng.integers(100000, 131000, size=50)                   # the largest b the sum allows: kappa to 2.6e5, which is
    near[400:450, 6] = rng.integers(100000, 131000, size=50)                   # its ceiling (det >= b when it is not zero)
    near[400:450, [0, 4, 8]] = 0
    near[450:700, [1, 3, 5, 7]] = rng.integers(0, 2000, size=(250, 4))         # the buckets in between
    rows.append(_fit(near))
    steps = []                                                                 # |z1| through the tail: one-sided tables of growing size
    for target in (1, 5, 10, 20, 30, 37, 38, 39, 45, 100, 200):
        for shape in range(12):
            lo, hi = 1, 100000
            while lo < hi:                                                     # the smallest m whose |z1| reaches the target (|z1| grows with m)
                m = (lo + hi) // 2
                if _z_of(_step_row(m, shape)) >= target:
                    hi = m
                else:
                    lo = m + 1
            for m in (lo - 1, lo, lo + 1):
                if m >= 1:
                    steps.append(_step_row(m, shape))
    rows.append(_fit(np.array(steps)))
    cont = np.concatenate(rows)
    cont = np.concatenate([cont, cont[rng.integers(0, cont.shape[0], size=100)]])   # repeats
    keep = np.array([system_of(r)[5] != 0 for r in cont.tolist()])
    cont = cont[keep]
    assert (cont >= 0).all() and cont.sum(axis=1).max() <= TALLY_SUM_MAX
    return cont.astype(np.int32)


def _step_row(m: int, shape: int):
    """a one-sided table of size m: the gene lies above m partners in one group and below (nearly) none, `shape` varies the rest"""
    k = shape % 4
    up = shape % 2 == 0
    big, small = (1, 5) if up else (3, 7)                                      # n12, n23 (R1, R2 large) or n21, n32
    row = [shape, 0, 0, 0, 7 * shape, 0, 0, 0, 3]
    row[big], row[small] = m, m // (1 + k) + 1
    row[2 if up else 6] = m // 3 if shape >= 6 else 0
    row[3 if up else 1] = k
    return row


def _groups(S: int):
    return np.array(["group1"] * (S // 2) + ["group2"] * (S - S // 2), dtype=object)


def _planted(G: int, S: int, noise: float, seed: int, noisy: float, shifted: float, guards: int, mirrors: int):
    rng = np.random.default_rng(seed)
    level = rng.permutation(G).astype(np.float64)
    X = level[:, None] + rng.normal(0.0, noise * G, size=(G, S)) * (rng.random(G) < noisy)[:, None]
    k = int(round(shifted * G))
    mid = np.argsort(np.abs(level - (G - 1) / 2), kind="stable")[:guards + mirrors]   # the genes at the middle levels
    genes = rng.choice(np.setdiff1d(np.arange(G), mid), size=k, replace=False)
    sign = rng.choice([-1.0, 1.0], size=k)
    assert max((sign > 0).sum(), (sign < 0).sum()) < 0.05 * G - 1
    X[genes, S // 2:] += (np.linspace(0.01, 1.0, k) ** 2 * G * sign)[:, None]
    h = S // 2
    for j, g in enumerate(mid):                                                # guards and mirrors alternate by level when there are both
        first = (j % 2 == 0 and j < 2 * guards) or j >= 2 * mirrors
        X[g, :] = level[g]
        if first:
            X[g, :h] = np.where(np.arange(h) % 2 == 0, -G - j, 2 * G + j)
        else:
            X[g, h:] = np.where(np.arange(S - h) % 2 == 0, -G - j, 2 * G + j)
    return np.asfortranarray(X), _groups(S)


def planted(G: int, S: int, noise: float, seed: int):
    """(X [G, S] Float64, group): distinct base levels (a permutation of 0 .. G-1), Gaussian noise of noise * G, and 4 % of the genes
    shifted in the second group by linspace(0.01, 1, k)^2 * G with a random sign: fewer than 5 % per side, so that they lie outside
    the trimmed slice.
    Two guard genes keep the integer-singular corner a = b = d > 0 out of the cases (it follows the oracle's float elimination by design
    and has its own tests): with this little noise many genes have reversed partners (n13, n31: the shifted genes that cross them) and
    no half-stable one, which IS that corner.  A guard alternates between a level below and a level above every gene in the first group
    and keeps its base level, a middle one, in the second: unstable there, stable here against every gene, so every table gets n21 or
    n23 >= 1 and a reversed pair no longer makes it singular.  The guards' own delta1 is near zero (as many genes above as below): they
    stay in the reference set."""
    return _planted(G, S, noise, seed, 1.0, 0.04, 2, 0)


def underflow(G: int, S: int, seed: int):
    """a variant whose trimmed slice holds zeros and near-zeros only, so that its standard deviation is tiny (0.1) and the p-values of
    the shifted genes pass through the subnormal range and underflow.  2 % of the genes are shifted, and 2.5 % of G guards (unstable
    in the first group, see `planted`) sit at the middle levels interleaved with as many mirrors (unstable in the SECOND group): a gene
    has H of each above it, or below it, which makes n12 = n21 (or n23 = n32) large and balanced.  An ordinary gene that no shifted
    gene crosses has a zero pivot and delta1 = 0 exactly; one that c shifted genes cross has delta1 = log((H + c + 0.5) / (H + 0.5)),
    about c / H.  These small values, and those of the half of the genes that get noise of 0.004 G (an unstable pair more on one side
    than on the other, over H), are the spread of the slice.  A slice of exact zeros alone would not do: its standard deviation is 0,
    the quantile windows of the light passes need two distinct values, and once the shifted genes have left the reference set nothing
    that they crossed is left.  With so small a spread every crossed gene would be called at padj 0.05 and the reference set would
    collapse within two passes: this case runs with padj_deg = 1e-40, so that the shifted genes alone are DEGs."""
    return _planted(G, S, 0.004, seed, 0.5, 0.02, int(round(0.025 * G)), int(round(0.025 * G)))


# Whole runs through identify_degs: name -> (generator, its arguments, padj_deg); Float64, all-ones reference set, RUN's other arguments,
# once with n_iter = 1 (a sorting pass only) and once with 6 passes.  The shapes are the smallest at which each seam of the kernels exists.
# The seeds are ones at which a light pass completes among the 6 (tests/test_gpu_pass_stats.py asserts it): with so little noise delta1
# takes few distinct values, and at many seeds every light pass hands its work back to the sorting path, as it is designed to.
RUN = {"pval_reo": 0.01, "pval_deg": 1.0, "n_conv": 0, "seed": 7}
N_ITERS = (1, 6)
SEAM_G = 29000   # the smallest multiple of 1 000 at which `planted`, S = 12, noise 0.0005, has more than 1 024 genes below 1e-6 after 6 passes
WHOLE_RUNS = {
    "tail_0005": (planted, (1200, 40, 0.0005, 1287), 0.05),                    # the tail: p to 1e-69
    "tail_002": (planted, (1200, 40, 0.002, 1241), 0.05),
    "half_1230": (planted, (1230, 16, 0.0005, 1248), 0.05),                    # 0.05 G = 61.5 and 62.5: the slice starts at 62 and 62
    "half_1250": (planted, (1250, 16, 0.0005, 1266), 0.05),
    "chunk_1024": (planted, (1024, 16, 0.0005, 1040), 0.05),                   # one full sort chunk,
    "chunk_1025": (planted, (1025, 16, 0.0005, 1041), 0.05),                   # a last chunk of one gene and 1 023 of padding,
    "chunk_2049": (planted, (2049, 16, 0.0005, 2066), 0.05),                   # the merge over three chunks
    "seam": (planted, (SEAM_G, 12, 0.0005, SEAM_G + 13), 0.05),                # the first 1 024-rank BH block seam inside the tail, and
                                                                                # a padj in front of it that comes from behind it
    "underflow": (underflow, (2000, 16, 5), 1e-40),                            # subnormal and zero p-values; only they are DEGs
}

