"""Cases for the slot order of the pair kernel (csrc/k1_slots.h; kernels.hip, launch_k1): the rule in numpy and the matrices that the
slot tests run.  No fixtures, no GPU, no import of the package: tests/test_slot_cases_cpu.py asserts on the CPU what each case is there
for, tests/test_gpu_slot_matrix.py (and test_gpu_slot_order.py / test_gpu_slot_queue.py) run them.

Sides: a comparison k of two groups has side 0, the samples of group k (the pair kernel's control side: cb, nc, m1), and side 1, the
rest.  Every function here takes `side`, one 0 / 1 per sample in file order; a group id array gives side = (gid != k).

All planted matrices hold integers below 2^24 that differ by at least 1 inside a sample, so the same matrix is tie-free and exact as
Int64, Int32, Float64 and Float32 (the float rule ties values closer than 0.1)."""
from __future__ import annotations

import functools

import numpy as np

TILE, CHUNK = 32, 256   # kSlotTile, kSlotChunk of k1_slots.h: gene rows of an item, genes of a wave chunk


def extremes(X, side):
    """(key, [(min, max) of side 0, (min, max) of side 1]) per gene: positions (ranks inside a sample; tie-free data) -> per-side extremes
    over the side's samples -> key = their sum."""
    side = np.asarray(side)
    pos = np.argsort(np.argsort(X, axis=0, kind="stable"), axis=0, kind="stable")
    ext = []
    for z in (0, 1):
        p = pos[:, side == z]
        ext.append((p.min(axis=1), p.max(axis=1)))
    return ext[0][0] + ext[0][1] + ext[1][0] + ext[1][1], ext


def masks(X, side):
    """The rule with the places kept: extremes -> slots by (key, gene) -> ranges of the 32-slot tiles and 256-slot chunks -> live
    (tile, chunk) pairs and, per side, the separated ones with cmax < rmin (every sample counts: `full`, the count is the side's size) or
    rmax < cmin (none does: `none`, the count is 0).  Returns (is_live[tile, chunk], {side: (full, none)})."""
    G = X.shape[0]
    key, ext = extremes(X, side)
    s2g = np.lexsort((np.arange(G), key))
    NT, NQ = (G + TILE - 1) // TILE, (G + CHUNK - 1) // CHUNK
    t, q = np.meshgrid(np.arange(NT), np.arange(NQ), indexing="ij")
    is_live = CHUNK * q + CHUNK - 1 >= (TILE * t // 64) * 64
    out = {}
    for z in (0, 1):
        mn, mx = ext[z][0][s2g], ext[z][1][s2g]
        rmin = np.array([mn[TILE * a:TILE * a + TILE].min() for a in range(NT)]); rmax = np.array([mx[TILE * a:TILE * a + TILE].max() for a in range(NT)])
        cmin = np.array([mn[CHUNK * a:CHUNK * a + CHUNK].min() for a in range(NQ)]); cmax = np.array([mx[CHUNK * a:CHUNK * a + CHUNK].max() for a in range(NQ)])
        out[z] = ((cmax[None, :] < rmin[:, None]) & is_live, (rmax[:, None] < cmin[None, :]) & is_live)
    return is_live, out


def model(X, side):
    """masks() counted: (live (tile, chunk, side) triples, {side: [separated with count n_side, with count 0]})."""
    is_live, sep = masks(X, side)
    out = {}
    for z in (0, 1):
        full, none = sep[z]
        assert not (full & none).any()
        out[z] = [int(full.sum()), int(none.sum())]
    return 2 * int(is_live.sum()), out


def model_count(X, side):
    """separated items of both sides; info()["k1_half_tiles_separated"] is twice this (a full item counts 2, a half-height item 1)"""
    return sum(sum(v) for v in model(X, side)[1].values())


# ---- layouts: which sample is on which side, and the group ids that give that side to comparison k

def layout_side(n0, n1, order, k, seed=0):
    """side per sample for n0 samples on side 0 and n1 on side 1.  The library numbers the groups in order of first appearance, so the
    first sample of the file belongs to group 0, which is side k of comparison k.  order: "contiguous" -- group 0's samples, then group
    1's; "shuffled" -- a seeded permutation behind that first sample; "split" -- one sample of group 0, all of group 1, the rest of
    group 0: the group with id 0 comes (but for one sample) second in the file."""
    first, other = k, 1 - k
    n_first, n_other = (n0, n1) if first == 0 else (n1, n0)
    if order == "contiguous":
        side = [first] * n_first + [other] * n_other
    elif order == "split":
        side = [first] + [other] * n_other + [first] * (n_first - 1)
    else:
        assert order == "shuffled", order
        rest = np.array([first] * (n_first - 1) + [other] * n_other)
        side = [first] + np.random.default_rng(seed).permutation(rest).tolist()
    side = np.asarray(side, dtype=np.int32)
    assert (side == 0).sum() == n0 and (side == 1).sum() == n1
    return side


def gid_of(side, k):
    """group ids (first appearance order) under which comparison k has these sides: side = (gid != k)"""
    gid = (np.asarray(side, dtype=np.int32) ^ k).astype(np.int32)
    assert gid[0] == 0 and np.array_equal(gid != k, np.asarray(side) != 0)
    return gid


# ---- generators

def planted(gid_side, G, seed):
    """G genes in four classes of G - 3 (G // 4), G // 4, G // 4, G // 4 on levels far apart, other bands per side: class -> band a =
    [0, 2, 4, 1] on side 0 and b = [2, 1, 0, 4] on side 1, the sums (2, 3, 4, 5) in slot order, so that chunks later in slot order lie
    BELOW earlier tiles on one side and both constants occur on both sides.  The half level changes sides (it cancels in the key).  With
    a gene count that is no multiple of 256 a chunk holds its class and the first genes of the next one, and the last chunk ends in
    padding columns.  The side of sample s is gid_side[s]."""
    rng = np.random.default_rng(seed)
    gid_side = np.asarray(gid_side)
    S = gid_side.size
    a = np.array([0, 2, 4, 1]); b = np.array([2, 1, 0, 4])
    cls = rng.permutation(np.repeat(np.arange(4), [G - 3 * (G // 4), G // 4, G // 4, G // 4]))
    sub = rng.integers(0, 2, size=G)
    X = np.empty((G, S), dtype=np.int64)
    for s in range(S):
        level = 2 * a[cls] + sub if gid_side[s] == 0 else 2 * b[cls] + 1 - sub
        X[:, s] = level * 1_000_000 + rng.permutation(G)
    return X


def same_order(G, S, seed):
    """every column the same permutation of 0 .. G - 1: a gene's range is a single point, the same on both sides, and its key four times
    that point -- all keys distinct, min == max everywhere.  Tiles lie below every later chunk: every separated item has count 0."""
    return np.tile(np.random.default_rng(seed).permutation(G).astype(np.int64)[:, None], (1, S))


def mirrored(G, n0, n1, seed):
    """(X, side): the n0 samples of side 0 hold one permutation x, the n1 samples of side 1 hold G - 1 - x.  Every key equals 2 (G - 1):
    the gene index decides the whole order, slots are genes, and a tile of 32 genes spans nearly all positions: nothing separates."""
    x = np.random.default_rng(seed).permutation(G).astype(np.int64)
    side = np.array([0] * n0 + [1] * n1, dtype=np.int32)
    return np.where(side[None, :] == 0, x[:, None], G - 1 - x[:, None]), side


DTYPES = ("int64", "float64", "float32", "int32")


def random_levels(rng, shuffled):
    """one case of the differential sweep: a dict with G, the side sizes n0 / n1, k, side (per sample), pval_reo, dtype, workers, queue
    (None: the variable stays unset), levels and the matrix X = level[side][class] * 1_000_000 + permutation(G), with 2 to 8 classes of
    equal size (genes dealt at random) and an independent permutation of the levels per side."""
    G = int(rng.integers(257, 1500))
    n0, n1 = (int(v) for v in rng.integers(2, 70, size=2))
    k = int(rng.choice([0, 1]))
    pval = float(rng.choice([0.01, 0.05, 0.3]))
    dtype = str(rng.choice(DTYPES))
    workers = [None, 1, 13, 40][int(rng.integers(0, 4))]
    queue = [None, 0][int(rng.integers(0, 2))]
    L = int(rng.integers(2, 9))
    level = [rng.permutation(L), rng.permutation(L)]
    side = layout_side(n0, n1, "shuffled" if shuffled else "contiguous", k, seed=int(rng.integers(0, 2 ** 31)))
    cls = rng.permutation(np.arange(G) * L // G)
    X = np.empty((G, n0 + n1), dtype=np.int64)
    for s in range(n0 + n1):
        X[:, s] = level[side[s]][cls] * 1_000_000 + rng.permutation(G)
    return dict(G=G, n0=n0, n1=n1, k=k, side=side, pval_reo=pval, dtype=dtype, workers=workers, queue=queue, levels=L, X=X)


SWEEP_SEED, SWEEP_CASES, SWEEP_MIN_SEPARATED = 20261019, 24, 16


@functools.lru_cache(maxsize=None)
def sweep():
    """the 24 cases of the sweep from one seed, contiguous and shuffled labels alternating; each with its model count under "separated" """
    rng = np.random.default_rng(SWEEP_SEED)
    cases = []
    for no in range(SWEEP_CASES):
        cs = random_levels(rng, shuffled=bool(no % 2))
        cs["separated"] = model_count(cs["X"], cs["side"])
        cases.append(cs)
    return tuple(cases)


# ---- the named cases of tests/test_gpu_slot_matrix.py

PLANTED_G, PLANTED_SEED = 1013, 11
# (side 0, side 1, order, pval_reo): a side of 2; 2 next to 62 (most slices of k1_slot_part empty; another number of sample blocks);
# 3 + 33 (a one-sample second block); exactly 32 and exactly 64 samples (no padding slots) next to one sample more; 5 + 96 (one block
# against three); shuffled labels; the group with id 0 second in the file
LAYOUTS = [(2, 2, "contiguous", 0.01), (2, 62, "contiguous", 0.01), (3, 33, "contiguous", 0.01), (32, 33, "contiguous", 0.01),
           (64, 65, "contiguous", 0.3), (5, 96, "contiguous", 0.3), (20, 44, "shuffled", 0.01), (40, 24, "split", 0.01)]
FORM_LAYOUT = (20, 44, "shuffled", 0.01)
FORMS = ("float64", "float32", "int32", "int64_rowmajor", "csc_host", "csc_device", "dense_device_ld")
UNSLOT_G = [20480, 20481, 30720, 30721, 32769, 61440, 61441, 65535]
TINY_G = [2, 31, 33, 256, 257]


def layout_id(lay):
    return f"{lay[0]}+{lay[1]}{'' if lay[2] == 'contiguous' else '-' + lay[2]}"


def planted_case(lay, k, G=PLANTED_G, seed=PLANTED_SEED):
    """(X, side, gid) of a layout of LAYOUTS under comparison k"""
    n0, n1, order, _ = lay
    side = layout_side(n0, n1, order, k, seed=seed + 1)
    return planted(side, G, seed), side, gid_of(side, k)
