"""Cases for the core path above 131 071 genes (18 position planes): inputs and a THIN exact reference.  No fixtures, no GPU.

The whole-table oracle (oracle.build_codes: G^2 bytes on the host, G^2 S compares) ends near 70 000 genes; at 131 584 its table would be
17 GB.  What is here costs O(G x strip x S) and is still the oracle's own arithmetic:

  coins           oracle.tie_wins / reo_numpy.tie_wins for arrays of keys (uint64 wrap-around arithmetic, n_eq <= 64: one word of the stream)
  expected_codes  the class codes of a block of ordered pairs from oracle.pair_counts and coins -- the rule of _expected_block_codes in
                  tests/test_gpu_parity.py (the pair with the smaller gene is evaluated, the other one mirrored as 8 - c, 255 on the
                  diagonal, comparison k against the rest), vectorised: a strip of 32 x G or G x 32 in a fraction of a second
  strip_tally     the 9 tallies of every gene over the columns of a G x w strip of codes
  reference_run   the loop of oracle_iterate (oracle/reo_oracle.c) with the tallies of each pass taken from a function, each pass computed
                  by oracle.iter_stats (the C oracle_iter_stats)
tests/test_big_plane_cases_cpu.py holds each of them to the whole-table oracle at a few hundred genes, and shows that every comparison of
tests/test_gpu_big_planes.py fails on one planted error."""
from __future__ import annotations

import numpy as np

_U = np.uint64
S = 16                  # samples of every two-group case
PVAL_REO = 0.1          # threshold(8, 0.1) = 7 < 8: every one of the nine classes occurs
STRIP = 32


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def popcount64(v):
    v = np.asarray(v, dtype=np.uint64)
    with np.errstate(over="ignore"):
        v = v - ((v >> _U(1)) & _U(0x5555555555555555))
        v = (v & _U(0x3333333333333333)) + ((v >> _U(2)) & _U(0x3333333333333333))
        v = (v + (v >> _U(4))) & _U(0x0F0F0F0F0F0F0F0F)
        return ((v * _U(0x0101010101010101)) >> _U(56)).astype(np.int64)


def coins(seed, i, j, g, n_eq):
    """oracle_tie_wins(seed, i, j, g, n_eq) for arrays i, j, n_eq (broadcast against each other; g a scalar or an array): how many of
    the n_eq tied samples of the unordered pair (i < j) and group g count as "i greater".  int64."""
    n_eq = np.asarray(n_eq, dtype=np.int64)
    assert n_eq.size == 0 or (n_eq.min() >= 0 and n_eq.max() <= 64), "one word of the coin stream: n_eq <= 64"
    i = np.asarray(i, dtype=np.uint64)
    j = np.asarray(j, dtype=np.uint64)
    g = np.asarray(g, dtype=np.uint64)
    with np.errstate(over="ignore"):
        base = mix64(_U(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ mix64((i << _U(32)) | j)) + (g << _U(40))
        bits = mix64(base)
        n = np.broadcast_to(n_eq, bits.shape)
        mask = np.where(n >= 64, _U(0xFFFFFFFFFFFFFFFF), (_U(1) << np.minimum(n, 63).astype(np.uint64)) - _U(1))
    return popcount64(bits & mask)


def thresholds(oracle, gid, ngroups, pval_reo=PVAL_REO):
    """the 2 x ngroups threshold matrix (src/RankCompV3.jl:362): row 0 the comparison's own group, row 1 every other sample"""
    sizes = np.bincount(gid, minlength=ngroups)
    n = int(sizes.sum())
    return np.array([[oracle.threshold(int(s), pval_reo) for s in sizes], [oracle.threshold(n - int(s), pval_reo) for s in sizes]], dtype=np.int32)


def expected_codes(oracle, X, gid, thr, seed, i0, i1, j0, j1, ngroups=2, k=0):
    """Class codes of the block [i0, i1) x [j0, j1) of ordered pairs, uint8.  X: G x S, float64 (column-major costs no copy)."""
    gid = np.ascontiguousarray(gid, dtype=np.int32)
    gt, eq = oracle.pair_counts(X, gid, ngroups, i0, i1, j0, j1)
    sizes = np.bincount(gid, minlength=ngroups).astype(np.int64)
    n = int(sizes.sum())
    ii = np.arange(i0, i1, dtype=np.int64)[:, None]
    jj = np.arange(j0, j1, dtype=np.int64)[None, :]
    low = ii > jj                                                   # the reference evaluated (j, i): the counts of that ordered pair
    lo, hi = np.broadcast_arrays(np.minimum(ii, jj), np.maximum(ii, jj))
    gt, eq = gt.astype(np.int64), eq.astype(np.int64)
    tot = np.zeros(gt.shape[:2], dtype=np.int64)
    nk = None
    for g in range(ngroups):
        g2 = np.where(low, sizes[g] - gt[:, :, g] - eq[:, :, g], gt[:, :, g])
        nre = g2
        tied = np.nonzero(eq[:, :, g])                               # (n_eq = 0: no coin, as the oracle)
        if tied[0].size:
            nre[tied] += coins(seed, lo[tied], hi[tied], g, eq[:, :, g][tied])
        tot += nre
        if g == k:
            nk = nre
    nt = tot - nk
    m1, m2 = int(thr[0, k]), int(thr[1, k])
    sk, st = int(sizes[k]), n - int(sizes[k])
    ic = np.where(nk >= m1, 2, np.where(sk - nk >= m1, 0, 1))
    it = np.where(nt >= m2, 2, np.where(st - nt >= m2, 0, 1))
    c = 3 * ic + it
    out = np.where(low, 8 - c, c)
    out[ii == jj] = 255
    return out.astype(np.uint8)


def mirror(codes):
    """the codes of the transposed block by the mirror rule (:386): c(j, i) = 8 - c(i, j), the diagonal stays 255"""
    t = np.asarray(codes).T
    return np.where(t == 255, 255, 8 - t.astype(np.int16)).astype(np.uint8)


def strip_tally(codes):
    """codes: G x w.  cont[i, c] = #{columns j of the strip : codes[i, j] == c}, G x 9 int32 (the diagonal's 255 counts nowhere)"""
    codes = np.asarray(codes)
    return np.stack([(codes == c).sum(axis=1) for c in range(9)], axis=1).astype(np.int32)


def column_histogram(codes):
    """codes: G x w, the strip of columns j0 .. j0 + w.  out[b, c] = #{i : codes[i, b] == 8 - c}: by the mirror rule the tallies of
    gene j0 + b over ALL genes, w x 9 int32"""
    codes = np.asarray(codes)
    return np.stack([(codes == 8 - c).sum(axis=0) for c in range(9)], axis=1).astype(np.int32)


def reference_run(tally_fn, G, ref0, pval_deg, padj_deg, n_iter, n_conv):
    """oracle_iterate (oracle/reo_oracle.c; src/RankCompV3.jl:396-425) with cont = tally_fn(ref) in the place of oracle_tally.
    Returns (result G x 15, passes, trace) as oracle.iterate does."""
    import oracle                                                    # (the repository root is on the path: tests/conftest.py)
    ref = np.ascontiguousarray(np.asarray(ref0) != 0, dtype=np.uint8)
    assert ref.size == G
    result = np.zeros((G, 15), order="F")                            # :398
    trace = []
    i_iter = 0
    while i_iter < n_iter:                                            # :400
        cont = np.asarray(tally_fn(ref.copy()))
        assert cont.shape == (G, 9)
        result, inds, nn = oracle.iter_stats(cont, pval_deg, padj_deg)
        trace.append((G - nn, nn))
        if abs(int(ref.sum()) - nn) < n_conv:                         # :419-422
            break
        i_iter += 1                                                   # :423
        ref = inds                                                    # :424
    return result, len(trace), trace


# ------------------------------------------------------------------------------------------------------------------ inputs

def labels(S_=S, ngroups=2):
    """interleaved groups 0 1 0 1 ...: the transform re-orders the samples"""
    return (np.arange(S_) % ngroups).astype(np.int32)


def _u64(seed, g, s):
    g = np.asarray(g, dtype=np.uint64)
    s = np.asarray(s, dtype=np.uint64)
    return mix64(_U(seed & 0xFFFFFFFFFFFFFFFF) ^ mix64((g << _U(32)) | s))


def _effects(seed, G):
    """the synthetic families' effects: 10 % of the genes shifted in one group (half up, half down), magnitude 1..4 base units"""
    h = _u64(seed + 2, np.arange(G), 0)
    sel = (h % _U(20)).astype(np.int64)
    mag = (1 + ((h >> _U(8)) % _U(4))).astype(np.int64)
    return np.where(sel == 0, mag, np.where(sel == 1, -mag, 0))


def free(G, seed, S_=S, gid=None):
    """Tie-free, Int64: every sample a permutation of 0 .. G - 1.  The recipe of the package's synth.t0_ranks (a base level per gene, an
    effect in the samples of group 1, 20 bits of noise; ranked by (value, gene)), restated: this file imports nothing GPU-side."""
    gid = labels(S_) if gid is None else np.asarray(gid)
    g = np.arange(G)[:, None]
    s = np.arange(S_)[None, :]
    base = (_u64(seed + 1, np.arange(G), 0) % _U(64)).astype(np.int64)[:, None]
    eff = _effects(seed, G)[:, None] * (gid == 1)[None, :]
    noise = (_u64(seed, g, s) >> _U(44)).astype(np.int64)
    v = (base + eff) * (1 << 18) + noise
    order = np.argsort(v, axis=0, kind="stable")
    X = np.empty((G, S_), dtype=np.int64)
    np.put_along_axis(X, order, np.broadcast_to(np.arange(G, dtype=np.int64)[:, None], (G, S_)), axis=0)
    return X


def counts(G, seed, S_=S, gid=None):
    """Tie-rich, Int64: integers in 0 .. 39 (tie groups of G / 40 genes per sample; the top value's group ends at position G), the same
    effects as `free`, in steps of 6, clipped to the range"""
    gid = labels(S_) if gid is None else np.asarray(gid)
    X = np.random.default_rng(seed).integers(0, 40, size=(G, S_))
    eff = 6 * _effects(seed, G)[:, None] * (gid == 1)[None, :]
    return np.clip(X + eff, 0, 39).astype(np.int64)


def band(G, seed, S_=S):
    """Float64 with three decimals: the 0.1 band ties values that are not equal"""
    return np.round(np.random.default_rng(seed).normal(8, 2, size=(G, S_)), 3)


MATRICES = {"free": (free, 0), "counts": (counts, 1), "band": (band, 1)}     # recipe, has_ties


def ref_runs(G, w=STRIP):
    """First columns of the four runs of w genes that make the reference set: at 0, across 65 536, across 131 072 (a third and two
    thirds of G where G is smaller than that), and ending at G"""
    b1, b2 = (65536, 131072) if G >= 131072 + w else (G // 3, 2 * G // 3)
    runs = [0, b1 - w // 2, b2 - w // 2, G - w]
    assert all(0 <= a and a + w <= b for a, b in zip(runs, runs[1:] + [G + w])), "the runs do not overlap"
    return runs


def ref_set(G, w=STRIP):
    m = np.zeros(G, dtype=bool)
    for j0 in ref_runs(G, w):
        m[j0:j0 + w] = True
    return m


# Items of the pair kernel that launch_k1 deals as two half-height items (rows 0-15 and 16-31 of the tile) at 131 584 genes, one 32-sample
# block per side, 256 compute units: k1_item_list (csrc/k1_items.h) halves 48 items there, all of the treat side and none in the last rows of
# the table -- the list is interleaved over eight queues, so its tail is spread over the last chunks' columns.  (first row, first column) of
# blocks of 32 x 64 in five of them (of the diagonal tile at 131 296 the last 64 columns of its chunk); the column strip at 131 056 crosses
# three more, at rows 113 952, 115 872 and 124 064, and the strip at 131 552 the last of the five.
# test_half_height_items_at_18_planes (tests/test_big_plane_cases_cpu.py) runs the list on the host and holds this to it.
HALF_ITEMS = [(113984, 114688), (123648, 124416), (117920, 122624), (131296, 131264), (116160, 131328)]
HALF_ITEM_ROWS_IN_STRIPS = {131056: [113952, 115872, 124064], 131552: [116160]}


def column_strips(oracle, Xf, gid, thr, seed, G, ngroups=2, k=0, w=STRIP):
    """{j0: G x w codes} of the four runs of ref_runs: every tally over ref_set(G) has an exact CPU reference in them"""
    return {j0: expected_codes(oracle, Xf, gid, thr, seed, 0, G, j0, j0 + w, ngroups, k) for j0 in ref_runs(G, w)}


def ref_set_tally(strips):
    """tally over ref_set(G) of every gene: the sum of the four strips' tallies"""
    return sum(strip_tally(c).astype(np.int64) for c in strips.values()).astype(np.int32)


# ------------------------------------------------------------- the comparisons of tests/test_gpu_big_planes.py (each one fails on a planted
# error: tests/test_big_plane_cases_cpu.py)

def check_codes(got, exp, i0, j0, what=""):
    """a block of the class table against the reference's, by equality; names the first cell that differs"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == np.uint8, (what, got.shape, exp.shape, got.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (f"{what}: {len(bad)} cells differ, first ({i0 + bad[0][0]}, {j0 + bad[0][1]}): "
                           f"{got[tuple(bad[0])]} for {exp[tuple(bad[0])]}")


def check_mirror(c_ab, c_ba, a, b, what=""):
    """c(i, j) == 8 - c(j, i) off the diagonal, 255 on it: c_ab the block at rows a.., columns b..; c_ba its transpose's block"""
    c1, c2 = np.asarray(c_ab).astype(np.int16), np.asarray(c_ba).astype(np.int16)
    off = np.arange(a, a + c1.shape[0])[:, None] != np.arange(b, b + c1.shape[1])[None, :]
    assert np.array_equal(c1[off], (8 - c2.T)[off]) and ((c1 == 255) == ~off).all(), (what, a, b)


def check_tally(got, exp, rows=None, what=""):
    """tallies (G x 9, or the listed rows of them) against the reference's, by equality; names the first gene that differs"""
    got, exp = np.asarray(got), np.asarray(exp)
    rows = np.arange(got.shape[0]) if rows is None else np.asarray(rows)
    assert got.shape == exp.shape and got.shape[1] == 9, (what, got.shape, exp.shape)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, f"{what}: {len(bad)} genes differ, first gene {rows[bad[0]]}: {got[bad[0]].tolist()} for {exp[bad[0]].tolist()}"


def check_run(got, exp, check_result, what=""):
    """(result, passes, trace) of a run against the reference's: passes and trace equal, then check_result(result, expected result) --
    tests/test_gpu_parity.py's: tallies equal, p and padj within P_ATOL, the statistics within STAT_RTOL"""
    (res, iters, trace), (eres, eit, etr) = got, exp
    assert iters == eit and list(trace) == list(etr), (what, iters, eit, trace, etr)
    check_result(np.asarray(res), np.asarray(eres))
