"""Cases for the PER-SIDE slot order of the pair kernel (csrc/k1_slots.h: slot_side_key, slot_sides_wanted; kernels.hip, launch_k1): the
rule in numpy beside the common rule of tests/slot_cases.py, and the matrices that tests/test_slot_sides_cpu.py checks and
tests/test_gpu_slot_sides.py runs.  No fixtures, no GPU, no import of the package.

The common rule orders the genes once, by key = pmin_0 + pmax_0 + pmin_1 + pmax_1; the per-side rule orders them once per side z, by
key_z = pmin_z + pmax_z, and takes the ranges of side z's tiles and chunks in side z's order.  Sides, layouts and group ids: as in
slot_cases (side 0 = the samples of group k of comparison k).

What the per-side rule cannot do: separate an item with the count n_side.  That needs a chunk LATER in the side's order whose every
gene lies BELOW every gene of the tile (cmax < rmin).  A later gene has key_z at least the tile gene's, and pmax' < pmin gives
key' = pmin' + pmax' < 2 pmin <= pmin + pmax = key.  So every separated item of a per-side build has the count 0, whatever the data
(test_slot_sides_cpu.py asserts it on every case); the constant n_side belongs to the common order, which the same matrices run as
the A/B partner and in which both constants occur on both sides.

All planted matrices hold integers below 2^24 that differ by at least 1 inside a sample: tie-free and exact in every dtype."""
from __future__ import annotations

import functools

import numpy as np

import slot_cases as sc

TILE, CHUNK = sc.TILE, sc.CHUNK
SIDES_BLOCKS = 16   # kSlotSidesBlocks of k1_slots.h: sample blocks of both sides together from which a build orders its sides separately


def orders(X, side):
    """[s2g of side 0, s2g of side 1] under the per-side rule, and the extremes they come from"""
    G = X.shape[0]
    _, ext = sc.extremes(X, side)
    return [np.lexsort((np.arange(G), ext[z][0] + ext[z][1])) for z in (0, 1)], ext


def masks(X, side):
    """slot_cases.masks with every side in its own order: (is_live[tile, chunk], {side: (full, none)})"""
    G = X.shape[0]
    s2g, ext = orders(X, side)
    NT, NQ = (G + TILE - 1) // TILE, (G + CHUNK - 1) // CHUNK
    t, q = np.meshgrid(np.arange(NT), np.arange(NQ), indexing="ij")
    is_live = CHUNK * q + CHUNK - 1 >= (TILE * t // 64) * 64
    out = {}
    for z in (0, 1):
        mn, mx = ext[z][0][s2g[z]], ext[z][1][s2g[z]]
        rmin = np.minimum.reduceat(mn, np.arange(0, G, TILE)); rmax = np.maximum.reduceat(mx, np.arange(0, G, TILE))
        cmin = np.minimum.reduceat(mn, np.arange(0, G, CHUNK)); cmax = np.maximum.reduceat(mx, np.arange(0, G, CHUNK))
        out[z] = ((cmax[None, :] < rmin[:, None]) & is_live, (rmax[:, None] < cmin[None, :]) & is_live)
    return is_live, out


def model(X, side):
    """(live (tile, chunk, side) triples, {side: [separated with count n_side, with count 0]}) under the per-side rule"""
    is_live, sep = masks(X, side)
    out = {}
    for z in (0, 1):
        full, none = sep[z]
        assert not (full & none).any()
        out[z] = [int(full.sum()), int(none.sum())]
    return 2 * int(is_live.sum()), out


def model_count(X, side):
    """separated items of both sides under the per-side rule; info()["k1_half_tiles_separated"] of a per-side build is twice this: an
    item of the model is a whole (tile, chunk, side) triple, which the library lists as one full item or as two half-height items"""
    return sum(sum(v) for v in model(X, side)[1].values())


def blocks_of(n):
    return (n + 31) // 32


def sides_by_rule(n0, n1):
    """what an unforced build reports as k1_slot_sides"""
    return 2 if blocks_of(n0) + blocks_of(n1) >= SIDES_BLOCKS else 1


# ---- generators

# The levelled matrices are slot_cases.planted: four classes on levels far apart, class -> band [0, 2, 4, 1] on side 0 and [2, 1, 0, 4] on
# side 1 -- two different permutations of the classes, so the common order (sums 2, 3, 4, 5) puts chunks BELOW earlier tiles on either
# side (both constants occur on both sides of a common build) and leaves every class but one out of place on each side, while each
# side's own order is sorted by level.
planted = sc.planted
LEVELS1 = np.array([2, 1, 0, 4])


def flat_side0(side, G, seed):
    """Side 0: its samples hold, in turn, a permutation x and G - 1 - x, so every gene's key on that side is G - 1 and the gene index
    alone decides side 0's order (slots are genes: nothing separates there).  Side 1: four classes on the levels of planted()'s side 1.  Side 0 needs an even
    number of samples, at least two."""
    rng = np.random.default_rng(seed)
    side = np.asarray(side)
    assert (side == 0).sum() % 2 == 0 and (side == 0).sum() >= 2
    x = rng.permutation(G).astype(np.int64)
    L = len(LEVELS1)
    cls = rng.permutation(np.arange(G) * L // G)
    X = np.empty((G, side.size), dtype=np.int64)
    flip = 0
    for s in range(side.size):
        if side[s] == 0:
            X[:, s] = x if flip == 0 else G - 1 - x
            flip ^= 1
        else:
            X[:, s] = LEVELS1[cls] * 1_000_000 + rng.permutation(G)
    return X


# ---- the named cases: name -> (G, side 0, side 1, order, k, generator)
SEED = 17
CASES = {
    "257": (257, 4, 4, "contiguous", 0, "planted"),                 # two chunks, the smallest with a separated item
    "1000x64": (1000, 32, 32, "contiguous", 0, "planted"),          # 12 planes, half-height items
    "2049x66": (2049, 33, 33, "contiguous", 0, "planted"),          # 15 planes, padded sample slots, a one-gene last tile
    "65535x8": (65535, 4, 4, "contiguous", 0, "planted"),           # 16 planes, the narrow un-permute, the 64-bit rank
    "30000x8": (30000, 4, 4, "contiguous", 0, "planted"),           # the wide un-permute
    "2+62": (1013, 2, 62, "contiguous", 0, "planted"),
    "33+32": (1013, 33, 32, "contiguous", 0, "planted"),
    "shuffled": (1013, 20, 44, "shuffled", 0, "planted"),
    "comparison1": (1013, 20, 44, "contiguous", 1, "planted"),      # the sides swapped: side 0 is group 1, second in the file
    "flat_side0": (1013, 6, 10, "contiguous", 0, "flat_side0"),
}


@functools.lru_cache(maxsize=4)
def case(name):
    """(X, side, gid, k) of a named case; the arrays are shared between tests and never written"""
    G, n0, n1, order, k, gen = CASES[name]
    side = sc.layout_side(n0, n1, order, k, seed=SEED + 1)
    X = planted(side, G, SEED) if gen == "planted" else flat_side0(side, G, SEED)
    X.setflags(write=False)
    side.setflags(write=False)
    return X, side, sc.gid_of(side, k), k
