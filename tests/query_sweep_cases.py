"""The seeded differential sweep of the query family (tests/test_gpu_query_sweep.py runs it, tests/test_query_sweep_cpu.py holds it to its
purpose): 24 cases from one seed, each a dict with the matrix, the sample labels and every argument of every call made on it, plus the
`order` the calls are made in.  The generator is numpy only: no fixtures, no GPU, no import of the package; the expectations (Expect) call
the restatements of the entry points' own test files and the oracle package.  A case is addressed by its number (sweep()[no], or case(no)
alone), so a failure is replayed alone.

What is drawn per case: G (33 .. 700, the square of a uniform number so that most cases stay small; one time in four a seam: 63, 64, 65, 255,
256, 257, 511, 513), 2 to 5 groups with sizes from {1, 2, 5, 31, 32, 33, 63, 64, 65, 97} and small numbers (S <= 260), contiguous or
interleaved labels, the element type (six kinds in rotation), how the matrix is handed over (column-major, row-major, scipy.sparse), the
table (build_pairs(k) or, from three groups on, half of the time build_contrast), pval_reo, the sides (a, b) of the searches, an unsorted
query list with repeats that holds gene 0 and gene G - 1, masks (none, 70 % random, one that excludes queried genes, one with 0 to 2 genes),
sizes m, n, kmax (sometimes above what is eligible), class masks, 3 to 9 relabellings per null or permutation call, and the order.

The tiny cases (TINY: G = 2 and G = 3) leave out identify_degs and perm_null -- reo_identify_degs refuses G < 10 (include/reo_hip.h: the
trimmed standard deviation's slice), and a permutation's pass is the same pass -- and with them every run with a NULL partner mask, which
stands for the reference set of the last identify_degs.  A case whose
table is a contrast leaves out perm_null: reo_perm_null wants the resident table of a comparison built by reo_build_pairs.

Cost.  The restatements under tests/ count every sample of every pair once per call, and the leave-one-out definition runs one full search
per fold.  Counts(X) holds the per-sample outcomes of a case as bits, packed along the samples, and answers masked_pairs_cases.masked_counts
(all-ones mask) and sample_counts_cases.states from them; fast(counts) puts the two in place of the originals while a restatement runs, so
that top_pairs_cases.oracle, top_pairs_null_cases.restate, top_pairs_loo_cases.restate and perm_null_cases.permuted_codes are called as
they are.  tests/test_query_sweep_cpu.py holds Counts to the originals.  The leave-one-out gene mask is thinned until folds x eligible
pairs <= LOO_PAIR_FOLDS: its restatement sorts every fold's pairs."""
from __future__ import annotations

import contextlib
import functools

import numpy as np

import float32_cases as fc
import masked_pairs_cases as mpc
import perm_null_cases as pnc
import sample_counts_cases as scc
import top_pairs_null_cases as tpnc
from query_cases import band_matrix

SWEEP_SEED, SWEEP_CASES = 20261021, 24
TINY = {5: 2, 17: 3}                                                             # case number -> G
SEAM_G = (63, 64, 65, 255, 256, 257, 511, 513)
SEAM_SIZES = (1, 2, 5, 31, 32, 33, 63, 64, 65, 97)
S_MAX = 260
KINDS = ("float64_band", "ranks", "int64_ties", "int32_ties", "float32_band", "level")
FORMS = ("colmajor", "rowmajor", "sparse")
LOO_PAIR_FOLDS = 1_500_000
QUERIES = ("codes", "pair_list", "sample_counts", "pair_support", "sample_tests", "sample_calls", "rank_shift", "top_pairs", "top_partners",
           "top_pairs_null", "top_pairs_loo", "perm_codes", "perm_null")
CALLS = QUERIES + ("identify_degs",)
PVAL_DEG, PADJ_DEG = 1.0, 0.05                                                   # identify_degs, as tests/test_gpu_parity.py
CALLS_PVAL, CALLS_PADJ = 0.2, 0.9                                                # sample_calls and perm_null: wide, so that calls occur


# ---- the per-sample outcomes of a case, as bits

_POP = np.array([bin(v).count("1") for v in range(256)], dtype=np.uint8)


class Counts:
    """gt and tie of every ordered pair in every sample under the comparator of masked_pairs_cases.masked_counts (Float32 in Float32
    arithmetic, everything else widened to Float64 with the band 0.1), one bit per sample.  group(ind) sums them over a set of samples: from
    scratch by a popcount table, or from a set already summed that differs in at most two samples."""

    def __init__(self, X):
        X = np.asarray(X)
        self.X = X
        G, S = X.shape
        self.G, self.S = G, S
        nb = (S + 7) // 8
        self.gt = np.zeros((G, G, nb), dtype=np.uint8)
        self.eq = np.zeros((G, G, nb), dtype=np.uint8)
        f32 = X.dtype == np.float32
        X64 = X.astype(np.float64)
        for s in range(S):
            tie = fc.f32_ties(X[:, s]) if f32 else np.abs(X64[:, None, s] - X64[None, :, s]) < 0.1
            gt = (~tie) & (X64[:, None, s] > X64[None, :, s])
            self.gt[:, :, s >> 3] |= gt.astype(np.uint8) << (7 - (s & 7))
            self.eq[:, :, s >> 3] |= tie.astype(np.uint8) << (7 - (s & 7))
        self.summed = []

    def plane(self, bits, s):
        return ((bits[:, :, s >> 3] >> (7 - (s & 7))) & 1).astype(np.int32)

    def group(self, ind):
        ind = np.asarray(ind, dtype=bool)
        for have, gt, eq in self.summed:
            d = np.flatnonzero(have != ind)
            if d.size <= 2:
                gt, eq = gt.copy(), eq.copy()
                for s in d:
                    sign = 1 if ind[s] else -1
                    gt += sign * self.plane(self.gt, int(s))
                    eq += sign * self.plane(self.eq, int(s))
                return gt, eq
        m = np.packbits(ind)
        gt = _POP[self.gt & m].sum(axis=2, dtype=np.int32)
        eq = _POP[self.eq & m].sum(axis=2, dtype=np.int32)
        self.summed.append((ind.copy(), gt, eq))
        return gt, eq

    def masked_counts(self, X, V, gid, ngroups):
        """masked_pairs_cases.masked_counts for this matrix under an all-ones mask"""
        assert np.asarray(X).shape == self.X.shape and np.asarray(X).dtype == self.X.dtype and np.asarray(V).all()
        gid = np.asarray(gid)
        G = self.G
        n_gt, n_eq, n_av = (np.zeros((G, G, ngroups), dtype=np.int32) for _ in range(3))
        for g in range(ngroups):
            n_gt[:, :, g], n_eq[:, :, g] = self.group(gid == g)
            n_av[:, :, g] = int((gid == g).sum())
        return n_gt, n_eq, n_av

    def states(self, X, genes):
        """sample_counts_cases.states for this matrix (no infinities in the sweep): queries x genes x samples, bool"""
        assert np.asarray(X).shape == self.X.shape
        genes = np.asarray(genes, dtype=np.int64).reshape(-1)
        gt = np.unpackbits(self.gt[genes], axis=2, count=self.S).astype(bool)
        eq = np.unpackbits(self.eq[genes], axis=2, count=self.S).astype(bool)
        return gt, eq


@contextlib.contextmanager
def fast(c: Counts):
    """while it is open, masked_pairs_cases.masked_counts and sample_counts_cases.states answer from a matrix's Counts"""
    keep = mpc.masked_counts, scc.states
    mpc.masked_counts, scc.states = c.masked_counts, c.states
    try:
        yield c
    finally:
        mpc.masked_counts, scc.states = keep


# ---- the draws

def draw_groups(rng, interleave):
    """(sizes, gid): 2 to 5 groups, S <= S_MAX, at least two groups of two or more samples (the leave-one-out call needs them); labels
    contiguous or interleaved, numbered in order of first appearance"""
    ng = int(rng.integers(2, 6))
    sizes = [int(rng.choice(SEAM_SIZES)) if rng.random() < 0.6 else int(rng.integers(2, 20)) for _ in range(ng)]
    if rng.random() < 0.4:
        sizes[int(rng.integers(0, ng))] = int(rng.choice([32, 64]))                 # whole blocks next to partly filled ones
    while sum(sizes) > S_MAX:
        sizes[int(np.argmax(sizes))] = int(rng.integers(2, 20))
    while sum(n >= 2 for n in sizes) < 2:
        sizes[int(np.argmin(sizes))] = int(rng.integers(2, 20))
    lab = np.repeat(np.arange(ng), sizes)
    if interleave:
        lab = lab[rng.permutation(lab.size)]
    first = {}
    for v in lab.tolist():
        first.setdefault(v, len(first))
    gid = np.array([first[v] for v in lab.tolist()], dtype=np.int32)
    return np.bincount(gid, minlength=ng).tolist(), gid


def draw_matrix(rng, kind, G, gid):
    """the matrix of a kind, G x S, in the dtype it goes to the library in.  Every kind has an effect in the second half of the samples or in
    a group, so that stable, reversed and unstable pairs occur."""
    S = gid.size
    seed = int(rng.integers(0, 2 ** 31))
    second = gid != 0
    if kind == "float64_band":
        X = np.array(band_matrix(max(G, 10), S, seed)[:G])
        X[: G // 4, second] += 1.0
        return X
    if kind == "ranks":                                                           # (query_cases.planted_ranks with the effect in a group)
        r = np.random.default_rng(seed)
        v = 10.0 * r.permutation(G)[:, None] + r.integers(-12, 13, size=(G, S))
        v[: G // 6, second] += 10.0 * G
        v[G // 6: G // 3, second] -= 10.0 * G
        X = np.empty((G, S), dtype=np.int64)
        np.put_along_axis(X, np.argsort(v, axis=0, kind="stable"), np.broadcast_to(np.arange(G, dtype=np.int64)[:, None], (G, S)), axis=0)
        return X
    if kind in ("int64_ties", "int32_ties"):
        r = np.random.default_rng(seed)
        X = r.integers(0, 8, size=(G, 1)) + r.integers(0, 3, size=(G, S))
        X[: G // 4, second] += 4
        X[G // 4: G // 2, second] -= 4
        X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)              # every sample its own pattern: a swapped column shows
        return X.astype(np.int64 if kind == "int64_ties" else np.int32)
    if kind == "float32_band":
        X = fc.planted(G, S, min(3, G // 2), seed)
        X[: G // 4, second] += np.float32(1.5)
        X[G // 4: G // 2, second] -= np.float32(1.5)
        return X
    assert kind == "level", kind
    r = np.random.default_rng(seed)
    X = r.integers(0, 6, size=(G, 1)) + r.integers(0, 2, size=(G, S))
    X[: G // 4, second] += 3
    X[G // 4: G // 2, second] -= 3
    lo = G // 2
    X[lo: lo + max(G // 5, 1)] = X[lo]                                           # a block of identical rows: whole runs of keys tie
    return X.astype(np.int64)


def draw_queries(rng, G):
    """2 to 40 genes, unsorted, with repeats, gene 0 and gene G - 1 among them; mostly no multiple of 8"""
    n = int(rng.integers(2, 41))
    if n % 8 == 0 and rng.random() < 0.8:
        n -= 1
    q = rng.integers(0, G, size=n)
    if n > 3:
        q[int(rng.integers(0, n))] = q[int(rng.integers(0, n))]                  # (most lists repeat a gene anyway)
    at = rng.choice(n, size=2, replace=False)
    q[at[0]], q[at[1]] = 0, G - 1
    if n > 3:
        free = np.delete(np.arange(n), at)
        q[free[0]] = q[free[-1]]                                                 # a repeat for certain
    return q.astype(np.int32)


def draw_mask(rng, G, queries):
    """None, 70 % random, one that excludes some of the queried genes, or 0 to 2 genes set"""
    kind = int(rng.integers(0, 4))
    if kind == 0:
        return None
    if kind == 1:
        return rng.random(G) < 0.7
    if kind == 2:
        m = rng.random(G) < 0.8
        m[np.unique(queries)[::2]] = False
        return m
    m = np.zeros(G, dtype=bool)
    m[rng.integers(0, G, size=int(rng.integers(0, 3)))] = True
    return m


def all_ones(G, mask):
    return np.ones(G, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)


def draw_sides(rng, sizes):
    """(a, b) of the searches: both sides of two or more samples; with three or more groups b is a group two times in three, which leaves
    a group on neither side"""
    ng = len(sizes)
    big = [g for g in range(ng) if sizes[g] >= 2]
    a = int(rng.choice(big))
    if ng >= 3 and rng.random() < 0.67:
        b = int(rng.choice([g for g in big if g != a]))
        return a, b
    return a, None


def draw_order(rng, calls):
    """a permutation of the calls with two of them made once more later in the sequence"""
    order = [calls[i] for i in rng.permutation(len(calls))]
    for name in rng.choice(order, size=min(2, len(order)), replace=False).tolist():
        at = order.index(name)
        order.insert(int(rng.integers(at + 1, len(order) + 1)), name)
    return tuple(order)


TABLE_QUERIES = ("pair_list", "sample_counts", "sample_tests", "sample_calls")      # the calls that take a NULL partner mask


def null_mask_runs(order):
    """how many calls of an order find a reference set standing -- one of the last identify_degs, not yet taken away by a perm_null -- and
    so run with the NULL partner mask too"""
    standing, n = False, 0
    for name in order:
        standing = True if name == "identify_degs" else False if name == "perm_null" else standing
        n += standing and name in TABLE_QUERIES
    return n


def random_case(no):
    rng = np.random.default_rng([SWEEP_SEED, no])
    kind = KINDS[(no + no // 6) % 6]
    interleave = bool(no % 2)                                                     # half and half
    sizes, gid = draw_groups(rng, interleave)
    ng, S = len(sizes), int(gid.size)
    if no in TINY:
        G = TINY[no]
    elif rng.random() < 0.25:
        G = int(rng.choice(SEAM_G))
    else:
        G = 33 + int(667 * rng.random() ** 2)
    X = draw_matrix(rng, kind, G, gid)
    form = FORMS[int(rng.integers(0, 3))]
    pval_reo = float(rng.choice([0.01, 0.05, 0.1]))
    if ng >= 3 and rng.random() < 0.5 and kind != "float32_band":   # (composed_rows counts in Float64)
        ctrl, treat = (int(v) for v in rng.choice(ng, size=2, replace=False))
        table = ("contrast", ctrl, treat)
    else:
        table = ("pairs", int(rng.integers(0, ng)))
    a, b = draw_sides(rng, sizes)
    side = tpnc.observed_row(gid, a, b)
    s_a, s_b = int((side == 1).sum()), int((side == 0).sum())
    queries = draw_queries(rng, G)
    cs = dict(no=no, G=G, S=S, sizes=sizes, gid=gid, ngroups=ng, interleaved=interleave, kind=kind, form=form, pval_reo=pval_reo, table=table,
              a=a, b=b, queries=queries, ctx_seed=SWEEP_SEED + no // 3, matrix_first=bool(rng.integers(0, 2)))
    cs["X"] = X
    cs["Xo"] = np.asfortranarray(X.astype(np.int64) if X.dtype == np.int32 else X)   # what the restatements read: Int32 widened
    cs["tag"] = f"case {no}: G={G} S={S} sizes={sizes}{' interleaved' if interleave else ''} {kind}/{form} {table} a={a} b={b}"
    # partner masks of the table queries (explicit: a bool array; the NULL mask runs besides, after an identify_degs)
    for name in ("pair_list", "sample_counts", "sample_tests", "sample_calls"):
        cs[name + "_mask"] = all_ones(G, draw_mask(rng, G, queries))
    cs["pair_list_classes"] = int(rng.integers(1, 0x200))
    cs["sample_counts_classes"] = int(rng.integers(1, 0x200))
    cs["top_partners_mask"] = draw_mask(rng, G, queries)
    cs["top_pairs_mask"] = draw_mask(rng, G, queries)
    cs["null_mask"] = draw_mask(rng, G, queries)
    loo_mask = draw_mask(rng, G, queries)
    n_el = G if loo_mask is None else int(loo_mask.sum())
    cap = LOO_PAIR_FOLDS // (s_a + s_b)
    if n_el * (n_el - 1) // 2 > cap:
        n_keep = max(int((2 * cap) ** 0.5), 2)
        el = np.arange(G) if loo_mask is None else np.flatnonzero(loo_mask)
        loo_mask = np.zeros(G, dtype=bool)
        loo_mask[rng.choice(el, size=n_keep, replace=False)] = True
    cs["loo_mask"] = loo_mask
    eligible = lambda m: G if m is None else int(np.asarray(m).sum())            # noqa: E731
    e = eligible(cs["top_partners_mask"])
    cs["m"] = int(rng.integers(1, 13)) if rng.random() < 0.6 else min(e + int(rng.integers(0, 4)), 1024) or 1
    e = eligible(cs["top_pairs_mask"])
    pairs = e * (e - 1) // 2
    cs["n"] = int(rng.integers(1, 200)) if rng.random() < 0.6 else max(pairs + int(rng.integers(0, 5)), 1)
    cs["n_all"] = G * (G - 1) // 2                                               # top_pairs without a mask, every pair: for from_pairs
    cs["kmax"] = int(rng.integers(1, 9)) if rng.random() < 0.6 else min(eligible(cs["loo_mask"]) // 2 + int(rng.integers(1, 4)), 64)
    cs["null_rows"] = tpnc.shuffled_rows(side, int(rng.integers(3, 10)), int(rng.integers(0, 2 ** 31)))
    cs["null_cuts"] = np.array([0, 1, s_a * s_b, 2 * s_a * s_b, 2 * s_a * s_b + 1], dtype=np.int64)
    k = table[1]
    cs["perm_k"] = k
    cs["perm_rows"] = pnc.shuffled_rows(gid, k, int(rng.integers(3, 10)), int(rng.integers(0, 2 ** 31)))
    cs["perm_ref"] = all_ones(G, draw_mask(rng, G, queries))
    cs["ref0"] = rng.random(G) < 0.5
    cs["n_iter"] = int(rng.integers(1, 6))
    calls = [c for c in CALLS if not (c in ("identify_degs", "perm_null") and G < 10) and not (c == "perm_null" and table[0] == "contrast")]
    cs["order"] = draw_order(rng, calls)
    return cs


@functools.lru_cache(maxsize=None)
def case(no):
    """case `no` alone: treat as read-only"""
    cs = random_case(no)
    for v in cs.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs


def sweep():
    """the SWEEP_CASES cases"""
    return tuple(case(no) for no in range(SWEEP_CASES))


def handed_over(cs):
    """the matrix as the case hands it to set_matrix: column-major, row-major, or a scipy.sparse CSC matrix"""
    if cs["form"] == "rowmajor":
        return np.ascontiguousarray(cs["X"])
    if cs["form"] == "sparse":
        import scipy.sparse
        return scipy.sparse.csc_matrix(np.asarray(cs["X"]))
    return np.asfortranarray(cs["X"])


# ---- what every call must return, from the restatements under tests/ and the oracle package alone

def thresholds(cs):
    """2 x ngroups, as Context.get_thresholds: row 0 the threshold of a group's size, row 1 that of all the other samples"""
    import oracle as orc
    n = np.asarray(cs["sizes"])
    return np.array([[orc.threshold(int(v), cs["pval_reo"]) for v in n], [orc.threshold(int(cs["S"] - v), cs["pval_reo"]) for v in n]], dtype=np.int32)


def side_sizes(cs):
    side = tpnc.observed_row(cs["gid"], cs["a"], cs["b"])
    return int((side == 1).sum()), int((side == 0).sum())


class Expect:
    """the expectations of one case, each computed once on first use: treat as read-only"""

    def __init__(self, cs):
        self.cs = case(cs) if isinstance(cs, int) else cs                       # (a dict: a case with a planted change)
        self.thr = thresholds(self.cs)

    @functools.cached_property
    def cnt(self) -> Counts:
        return Counts(self.cs["Xo"])

    @functools.cached_property
    def codes(self):
        """the class table (255 on the diagonal): oracle.build_codes; a Float32 matrix through masked_pairs_cases.masked_codes on the
        Float32 counts (oracle.build_codes compares in Float64); a contrast by test_gpu_contrasts.composed_rows"""
        import oracle as orc
        cs = self.cs
        Xo, gid, ng, G, seed, table = cs["Xo"], cs["gid"], cs["ngroups"], cs["G"], cs["ctx_seed"], cs["table"]
        if table[0] == "pairs":
            k = table[1]
            if Xo.dtype == np.float32:
                with fast(self.cnt):
                    cnt = mpc.masked_counts(Xo, np.ones(Xo.shape, dtype=bool), gid, ng)
                return mpc.masked_codes(cnt, k, cs["pval_reo"], mpc.default_min_complete(np.asarray(cs["sizes"]), k, cs["pval_reo"]), seed)
            return orc.build_codes(Xo.astype(np.float64), gid, ng, k, (int(self.thr[0, k]), int(self.thr[1, k])), seed)
        from test_gpu_contrasts import composed_rows
        _, ctrl, treat = table
        out, off = composed_rows(orc, Xo, gid, ng, self.thr, seed, 0, G, [(ctrl, treat)])
        return np.where(off, out[ctrl, treat], 255).astype(np.uint8)

    def row(self, i):
        return self.codes[int(i)]

    @functools.cached_property
    def states(self):
        return self.cnt.states(self.cs["Xo"], self.cs["queries"])

    def pair_list(self, mask):
        from test_gpu_pair_list import expected
        return expected(self.row, self.cs["queries"], self.cs["pair_list_classes"], mask)

    def sample_counts(self, mask):
        return scc.expected_counts(self.cs["Xo"], self.row, self.cs["queries"], self.cs["sample_counts_classes"], mask, self.states)

    def pair_support(self, csr):
        from test_gpu_pair_support import expected
        with fast(self.cnt):
            return expected(self.cs["Xo"], self.cs["gid"], self.cs["ngroups"], *csr)

    def sample_tests(self, mask):
        import sample_tests_cases as stc
        return stc.expected_integers(self.cs["Xo"], self.row, self.cs["queries"], mask, self.states)

    @functools.cached_property
    def top(self):
        """top_pairs_cases.oracle over all pairs"""
        import top_pairs_cases as tpc
        cs = self.cs
        with fast(self.cnt):
            return tpc.oracle(cs["Xo"], cs["gid"], cs["ngroups"], cs["a"], cs["b"])

    @functools.cached_property
    def top_masked(self):
        import top_pairs_cases as tpc
        cs = self.cs
        if cs["top_pairs_mask"] is None:
            return self.top
        with fast(self.cnt):
            return tpc.oracle(cs["Xo"], cs["gid"], cs["ngroups"], cs["a"], cs["b"], cs["top_pairs_mask"])

    def partners(self, queries=None, mask="case"):
        """top_partners_cases.row_oracle of every queried row"""
        import top_partners_cases as tprc
        cs = self.cs
        mask = cs["top_partners_mask"] if isinstance(mask, str) else mask
        queries = cs["queries"] if queries is None else queries
        return [tprc.row_oracle(cs["Xo"], cs["gid"], cs["ngroups"], cs["a"], cs["b"], self.top.D, int(q), mask) for q in queries]

    @functools.cached_property
    def null(self):
        cs = self.cs
        with fast(self.cnt):
            return tpnc.restate(cs["Xo"], cs["null_rows"], cs["null_cuts"], cs["null_mask"])

    @functools.cached_property
    def loo(self):
        import top_pairs_loo_cases as tlc
        cs = self.cs
        self.top                                                                 # (the sides' sums first: every fold is one sample away)
        with fast(self.cnt):
            return tlc.restate(cs["Xo"], cs["gid"], cs["ngroups"], cs["a"], cs["b"], cs["kmax"], cs["loo_mask"])

    @functools.lru_cache(maxsize=None)
    def perm_codes(self, p):
        cs = self.cs
        k = cs["perm_k"]
        with fast(self.cnt):
            return pnc.permuted_codes(cs["Xo"], cs["perm_rows"][p], (int(self.thr[0, k]), int(self.thr[1, k])), cs["ctx_seed"])

    def one_pass(self, code, ref, pval_deg, padj_deg):
        import oracle as orc
        return orc.iterate(code, ref, pval_deg, padj_deg, 1, 0)[0]

    @functools.cached_property
    def degs(self):
        """(result, passes, trace, the reference set of the last pass) of oracle.iterate on the expected table"""
        import oracle as orc
        cs = self.cs
        res, it, trace = orc.iterate(self.codes, cs["ref0"], PVAL_DEG, PADJ_DEG, cs["n_iter"], 1)
        r = last = np.asarray(cs["ref0"], dtype=bool)
        for _ in range(it):
            one = self.one_pass(self.codes, r, PVAL_DEG, PADJ_DEG)
            last, r = r, ~((one[:, 0] <= PVAL_DEG) & (one[:, 1] <= PADJ_DEG))
        assert np.array_equal(orc.tally(self.codes, last), res[:, 2:11].astype(np.int32))
        return res, it, trace, last


@functools.lru_cache(maxsize=3)
def expect(no) -> Expect:
    return Expect(no)


def check_top_pairs(tp, o, n, tag=None):
    """a TopPairs against the first n pairs of a top_pairs_cases.Oracle, field by field"""
    k = min(n, o.gene_i.size)
    assert tp.gene_i.dtype == np.int32 and tp.gene_i.size == k, (tag, tp.gene_i.size, k)
    assert np.array_equal(tp.gene_i, o.gene_i[:k]) and np.array_equal(tp.gene_j, o.gene_j[:k]), tag
    assert np.array_equal(tp.n_gt, o.counts[:k, 0::2]) and np.array_equal(tp.n_eq, o.counts[:k, 1::2]), tag
    assert tp.num.dtype == np.int64 and np.array_equal(tp.num, o.num[:k]) and np.array_equal(tp.rank_num, o.rank_num[:k]), tag
    assert tuple(int(v) for v in tp.side_sizes) == tuple(o.sizes), tag


def check_null(got, exp, tag=None):
    for f in ("max_num", "arg_i", "arg_j", "n_reach"):
        g, e = getattr(got, f), getattr(exp, f)
        assert g.dtype == e.dtype and g.shape == e.shape and np.array_equal(g, e), (tag, f, g.tolist(), e.tolist())
