"""Cases for the plane-reading kernels at 12, 15 and 16 position planes (tests/test_gpu_planes.py): gene counts, seeded matrices, the
rectangles a test looks at, and numpy restatements of the masked and the permuted class table ON A RECTANGLE -- no G x G array exists at
these sizes.  No fixtures, no GPU.

plane_bits(G) is 12 up to 4 095 genes, 15 up to 32 767, 16 up to 65 535.  A gene count that is the first of a plane count does not make
the new top plane carry information: at 4 096 and 32 768 genes every position still fits the old width and only an upper band edge equal
to G reaches the new plane.  So the boundary sizes test the dispatch, the pads and the ragged last tiles.  Gp, the next multiple of 1 024,
is 4 096 for 4 095 and for 4 096 genes, 32 768 for 32 767 and 32 768, 65 536 for 65 535: at 4 096 and 32 768 genes no padding column
exists at all, and PAD_G adds the two sizes one gene further, whose last gene stands alone in a pad of its own (Gp = 5 120 and 33 792).
DEEP_G tests that planes 12 - 14 (9 000 genes) and plane 15 (65 535) are compared correctly, which truncated_gt shows on the CPU: every
rectangle's counts change when the ranks lose the bits above 11 (above 14 at 65 535).

The restatements follow include/reo_hip.h ("Missing values", "Label-permutation null"), per sample, in int64: a cell (i, j) of a rectangle
is classified from the counts of its pair with the SMALLER index first -- the coins are keyed that way -- and holds 8 minus that class
below the diagonal, 255 on it."""
from __future__ import annotations

import numpy as np

import masked_pairs_cases as mpc
import perm_null_cases as pnc
from oracle import reo_numpy as rn

PLANE_G = [4095, 4096, 9000, 32767, 32768, 65535]
DEEP_G = [9000, 65535]
PAD_G = [4097, 32769]
QUERY_G = [4096, 9000, 32768, 65535]
KINDS = ("ranks", "ties")
MASKED_FRAC = 0.10        # missing at random: with sides of 9 - 33 both "short" and "no majority" make class 2 (asserted on the CPU)
SEED = 0x5EED0E00


def plane_bits(G):
    return 12 if G <= 4095 else 15 if G <= 32767 else 16


def padded(G):
    return -(-G // 1024) * 1024


def sides(G):
    """12 / 9 at the boundary sizes (one block of 32 slots each); 33 / 12 at DEEP_G (2 + 1 blocks, padding slots in both)"""
    return (33, 12) if G in DEEP_G else (12, 9)


def boundary_kind(G):
    """the one matrix of a boundary size in the permuted build, whose tie-free form is a kernel of its own: the forms alternate"""
    return KINDS[(PLANE_G + PAD_G).index(G) % 2]


def rectangles(G):
    """(i0, i1, j0, j1), at most 40 x 200 pairs each: the first rows against the last columns; the last rows against the first columns
    (below the diagonal: the mirror rule); the last 9 rows against the last 70 columns (ragged row and column tiles, the diagonal); where
    they fit, blocks on the diagonal across 4 096 and across 32 768"""
    out = [(0, 40, G - 200, G), (G - 40, G, 0, 200), (G - 9, G, G - 70, G)]
    for seam in (4096, 32768):
        if seam + 100 <= G:
            out.append((seam - 20, seam + 20, seam - 100, seam + 100))
    return out


def grid(rect):
    i0, i1, j0, j1 = rect
    return np.meshgrid(np.arange(i0, i1, dtype=np.int64), np.arange(j0, j1, dtype=np.int64), indexing="ij")


def _pair_counts(X, V, gid, ngroups, I, J):
    """(gt, eq, n) of the ordered pairs (I, J), elementwise, per group: int64 arrays of I's shape + (ngroups,).  Float64: tied when
    abs(x_i - x_j) < 0.1; Int64: tied when equal."""
    X = np.asarray(X)
    assert X.dtype in (np.float64, np.int64), X.dtype
    gt = np.zeros(I.shape + (ngroups,), dtype=np.int64)
    eq = np.zeros_like(gt)
    n = np.zeros_like(gt)
    for s in range(X.shape[1]):
        x = X[:, s]
        a, b = x[I], x[J]
        tie = (np.abs(a - b) < 0.1) if X.dtype == np.float64 else (a == b)
        v = np.ones(I.shape, dtype=bool) if V is None else (V[I, s] != 0) & (V[J, s] != 0)
        g = int(gid[s])
        gt[..., g] += v & ~tie & (a > b)
        eq[..., g] += v & tie
        n[..., g] += v
    return gt, eq, n


def masked_counts_block(X, V, gid, ngroups, rect):
    """masked_pairs_cases.masked_counts on a rectangle: (n_gt, n_eq, n_avail) of the ORDERED pairs, int32, (i1 - i0) x (j1 - j0) x ngroups"""
    I, J = grid(rect)
    return tuple(c.astype(np.int32) for c in _pair_counts(X, V, gid, ngroups, I, J))


def _first_counts(X, V, gid, ngroups, rect, seed):
    """the counts of every cell's pair with the smaller index first, and nre = gt + the keyed coins of (seed, lo, hi, g)"""
    I, J = grid(rect)
    lo, hi = np.minimum(I, J), np.maximum(I, J)
    gt, eq, n = _pair_counts(X, V, gid, ngroups, lo, hi)
    up = gt.copy()
    for a, b, g in np.argwhere(eq > 0):
        if lo[a, b] != hi[a, b]:
            up[a, b, g] += rn.tie_wins(seed, int(lo[a, b]), int(hi[a, b]), int(g), int(eq[a, b, g]))
    return I, J, up, eq, n


def _place(I, J, c):
    """the class of the pair (smaller, larger) into the cell: as it is above the diagonal, 8 minus it below, 255 on the diagonal"""
    return np.where(I < J, c, np.where(I > J, 8 - c, 255)).astype(np.uint8)


def masked_codes_block(X, V, gid, ngroups, rect, k, pval_reo, min_complete, seed, detail=False):
    """masked_pairs_cases.masked_codes on a rectangle.  detail=True: also a dict of boolean arrays over the cells off the diagonal --
    short_c, short_t, nomaj_c, nomaj_t (why a side is class 2) and eq_c, eq_t (the side has ties)"""
    I, J, up, eq, n = _first_counts(X, V, gid, ngroups, rect, seed)
    a, n1 = up[..., k], n[..., k]
    b, n2 = up.sum(axis=-1) - a, n.sum(axis=-1) - n1
    m = mpc.threshold_table(int(max(n1.max(), n2.max())), float(pval_reo))
    short_c, short_t = n1 < min_complete[0], n2 < min_complete[1]
    ic = np.where(short_c, 2, np.where(a >= m[n1], 3, np.where(n1 - a >= m[n1], 1, 2)))
    it = np.where(short_t, 2, np.where(b >= m[n2], 3, np.where(n2 - b >= m[n2], 1, 2)))
    code = _place(I, J, 3 * (ic - 1) + (it - 1))
    if not detail:
        return code
    off = I != J
    return code, {"short_c": short_c & off, "short_t": short_t & off, "nomaj_c": (ic == 2) & ~short_c & off, "nomaj_t": (it == 2) & ~short_t & off,
                  "eq_c": (eq[..., k] > 0) & off, "eq_t": (eq.sum(axis=-1) - eq[..., k] > 0) & off}


def permuted_codes_block(X, row, thr, seed, rect, detail=False):
    """perm_null_cases.permuted_codes on a rectangle: sides by `row` (1 = side A), coins keyed by side 0 / 1, thresholds thr = (m1, m2).
    detail=True: also eq_a, eq_b (the side has ties), boolean over the cells off the diagonal"""
    row = np.asarray(row).astype(np.int64)
    side = 1 - row
    I, J, up, eq, _ = _first_counts(X, None, side, 2, rect, seed)
    n1, n2 = int(row.sum()), int(row.size - row.sum())
    a, b = up[..., 0], up[..., 1]
    ic = np.where(a >= thr[0], 3, np.where(n1 - a >= thr[0], 1, 2))
    it = np.where(b >= thr[1], 3, np.where(n2 - b >= thr[1], 1, 2))
    code = _place(I, J, 3 * (ic - 1) + (it - 1))
    if not detail:
        return code
    off = I != J
    return code, {"eq_a": (eq[..., 0] > 0) & off, "eq_b": (eq[..., 1] > 0) & off}


def sample_ranks(X):
    """per sample, the number of genes strictly smaller (int64, G x S), from np.argsort on the column"""
    X = np.asarray(X)
    R = np.empty(X.shape, dtype=np.int64)
    for s in range(X.shape[1]):
        x = X[:, s]
        xs = x[np.argsort(x, kind="stable")]
        R[:, s] = np.searchsorted(xs, x, side="left")
    return R


def truncated_gt(X, gid, rect, bits, ranks=None, V=None):
    """The gt counts of the rectangle, (i1 - i0) x (j1 - j0) x ngroups, when every sample's ranks (sample_ranks; `ranks`, when the caller
    has them) are reduced modulo 2^bits before they are compared -- what a borrow chain that ignored the planes from `bits` upwards would
    count.  bits = 18 truncates nothing.  V: a validity mask, under which only the samples valid for both genes count."""
    R = (sample_ranks(X) if ranks is None else ranks) & ((1 << bits) - 1)
    I, J = grid(rect)
    return _pair_counts(R, V, gid, int(np.max(gid)) + 1, I, J)[0]


# ---- the seeded cases of the GPU tests

def masked_case(G, kind):
    """X, V, gid, seed of the masked build at G genes: `ties` = Float64 rounded to two decimals (tie bands thousands of genes wide at
    DEEP_G), `ranks` = tie-free; gene levels and G / 8 genes planted up and as many down in group 1, so that stable and reversed pairs occur"""
    seed = SEED + G + (1 if kind == "ranks" else 0)
    if kind == "ranks":
        X, V, gid = mpc.rank_case(G, sides(G), MASKED_FRAC, seed, level=0.8, shift=2.0, planted=G // 8)
    else:
        X, V, gid = mpc.float_case(G, sides(G), MASKED_FRAC, seed, shift=2.0, planted=G // 8)
    return np.asfortranarray(X), np.asfortranarray(V), gid, seed


def perm_case(G, kind):
    """X (Fortran order), gid, seed of the permuted build at G genes; the data of masked_case without a mask, under a seed of its own"""
    seed = SEED + 0x100000 + G + (1 if kind == "ranks" else 0)
    kw = {"level": 0.8} if kind == "ranks" else {}
    X, gid = pnc.case(G, sides(G), kind, seed, shift=2.0, planted=G // 8, **kw)
    return X, gid, seed


def perm_rows(gid, seed, k=0):
    """two shuffled label rows (1 = side A): a free shuffle, under which the sides are mixtures of the groups and few pairs are stable, and
    the observed labels with one sample of each side exchanged, under which the planted genes still give reversed pairs"""
    free = pnc.shuffled_rows(gid, k, 1, seed + 1)[0]
    rng = np.random.default_rng(seed + 2)
    near = (np.asarray(gid) == k).astype(np.uint8)
    a, b = rng.choice(np.flatnonzero(near == 1)), rng.choice(np.flatnonzero(near == 0))
    near[a], near[b] = 0, 1
    return np.stack([free, near])


def query_genes(G):
    """the first gene, the last gene and one on each side of 4 096 and 32 768, as far as they exist"""
    return np.array(sorted({g for g in (0, 4095, 4096, 32767, 32768, G - 1) if g < G}), dtype=np.int32)


def query_marks(G):
    return [g for g in (0, 4095, 4096, 32767, 32768, G - 1) if g < G]


QUERY_SEED = {4096: 4170, 9000: 9068, 32768: 32831, 65535: 65596}   # Int64 below 30 000: seeds at which query genes tie with marked partners


def query_ranks(G, seed, S=8):
    """tie-free Int64 for the queries: every sample a permutation of 0 .. G - 1 around gene levels, Fortran order"""
    X = mpc.rank_case(G, (S // 2, S - S // 2), 0.0, seed, level=0.8)[0]
    return np.asfortranarray((X / 10.0).astype(np.int64))
