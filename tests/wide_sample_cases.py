"""Cases for the query and derived-table kernels on wide sample axes (tests/test_gpu_wide_samples.py, tests/test_wide_sample_cases_cpu.py):
the sample layouts and the seeded data.  No fixtures, no GPU, no import of the package.

Every kernel behind reo_sample_counts / _tests / _calls, reo_pair_support, the masked build, the permuted tables and the contrasts walks the
sample axis in blocks of 32 slots, each group padded to whole blocks (perm_null_cases.slot_map restates csrc/sample_counts.h's
sc_slot_map); k_sample_counts cuts the blocks into chunks of CHUNK_BLOCKS.  The layouts below are the smallest at which each seam exists:

  name             group sizes                        S    blocks           chunks   what it reaches
  seam_in_group    130, 135 (shuffled)                265  5 + 5 = 10       8 + 2    a chunk seam inside the second group; a short last chunk;
                                                                                     padding in both groups
  full_blocks      256, 256 (contiguous)              512  8 + 8 = 16       8 + 8    no padding slot anywhere; the chunk seam on the group
                                                                                     seam; 9-bit side counts; more than 64 ties of a side
  three_groups     300, 33, 31 (shuffled)             364  10 + 2 + 1 = 13  8 + 5    a group longer than a chunk
  mostly_padding   [1, 2, 3] * 5 + [20, 30] (shuffled) 80  17               8 + 8 + 1  a last chunk of one block; most slots are padding
  contrast_groups  300, 260, 40 (shuffled)            600  10 + 9 + 2 = 21  --       counts above 255 in two count planes

Group ids are numbered in order of first appearance, as the package's encode_groups numbers them, so a group's id depends on the shuffle:
group_of_size names a group by its size.  tests/test_wide_sample_cases_cpu.py asserts, from the numpy oracle, the conditions under which
the GPU tests mean something (blocks and chunks, all nine classes, more than 64 ties of a side, columns that differ)."""
from __future__ import annotations

import functools

import numpy as np

import perm_null_cases as pnc
from query_cases import planted_ranks, tie_rich

CHUNK_BLOCKS = 8   # kScChunkBlocks of csrc/sample_counts.h

#          name: (group sizes in the table's order, shuffled?, shuffle seed, blocks in all, blocks per chunk)
LAYOUTS = {"seam_in_group": ((130, 135), True, 101, 10, (8, 2)),
           "full_blocks": ((256, 256), False, 0, 16, (8, 8)),
           "three_groups": ((300, 33, 31), True, 103, 13, (8, 5)),
           "mostly_padding": (tuple([1, 2, 3] * 5 + [20, 30]), True, 104, 17, (8, 8, 1)),
           "contrast_groups": ((300, 260, 40), True, 105, 21, (8, 8, 5))}

QUERY_LAYOUTS = ("seam_in_group", "full_blocks", "three_groups", "mostly_padding")
G_QUERY, G_TABLE, G_CONTRAST = 130, 70, 200   # the query entries, whole-table comparisons, the contrasts
QUERY_SEED, QUERY_PVAL_REO = 9, 0.1          # int_ties(name, G_QUERY, QUERY_SEED, k): all nine classes occur at 0.1 (asserted on the CPU)
# int_ties(name, G_TABLE, seed, k, pattern=False): on seam_in_group and full_blocks a pair is tied in more than 64 samples of a group, so
# that tie_wins takes a second word of its stream (asserted on the CPU; seam_in_group has two such pairs at this seed, most seeds none)
TABLE_SEED = {"seam_in_group": 21, "full_blocks": 9, "three_groups": 9}


def first_appearance(labels) -> np.ndarray:
    """ids 0, 1, ... in order of first appearance (oracle.reo_numpy.group_ids, the package's encode_groups), int32"""
    seen: dict = {}
    return np.asarray([seen.setdefault(v, len(seen)) for v in np.asarray(labels).tolist()], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def _gid(name: str) -> np.ndarray:
    sizes, shuffled, seed, _, _ = LAYOUTS[name]
    raw = np.repeat(np.arange(len(sizes)), sizes)
    if shuffled:
        raw = np.random.default_rng(seed).permutation(raw)
    gid = first_appearance(raw)
    gid.setflags(write=False)
    return gid


def gid_of(name: str) -> np.ndarray:
    """the group id of every sample column of a layout, int32, read-only"""
    return _gid(name)


def sizes_of(name: str) -> np.ndarray:
    return np.bincount(gid_of(name))


def group_of_size(name: str, n: int) -> int:
    """the id of the one group of a layout that has n samples"""
    at = np.flatnonzero(sizes_of(name) == n)
    assert at.size == 1, (name, n, sizes_of(name).tolist())
    return int(at[0])


def query_cases():
    """(layout, k) of the query entries' tests: three_groups for k = 0 and 2, mostly_padding against its 30-sample group"""
    return [("seam_in_group", 0), ("full_blocks", 0), ("three_groups", 0), ("three_groups", 2),
            ("mostly_padding", group_of_size("mostly_padding", 30))]


def slot_map(name: str) -> np.ndarray:
    gid = gid_of(name)
    return pnc.slot_map(gid, int(gid.max()) + 1)


def blocks_of(name: str):
    """(blocks of 32 slots per group in id order, blocks in all, blocks per chunk of CHUNK_BLOCKS) from the group sizes"""
    per_group = [(int(n) + 31) // 32 for n in sizes_of(name)]
    nblk = sum(per_group)
    return per_group, nblk, tuple(min(CHUNK_BLOCKS, nblk - b) for b in range(0, nblk, CHUNK_BLOCKS))


def sample_pattern(G: int, S: int) -> np.ndarray:
    """every sample its own pattern on the odd genes (tests/test_gpu_sample_counts.py, test_interleaved_labels_33_and_37): a swapped or
    shifted column shows"""
    return np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)


@functools.lru_cache(maxsize=None)
def _tie_rich(name: str, G: int, seed: int, k: int, pattern: bool) -> np.ndarray:
    gid = gid_of(name)
    X = tie_rich(G, gid.size, seed, gid != k)
    if pattern:
        X = X + sample_pattern(G, gid.size)
    X = np.asfortranarray(X.astype(np.int64))
    X.setflags(write=False)
    return X


def int_ties(name: str, G: int, seed: int, k: int = 0, pattern: bool = True) -> np.ndarray:
    """tie-rich Int64 (query_cases.tie_rich) with the effect in every sample outside group k; pattern: plus sample_pattern.  Read-only."""
    return _tie_rich(name, G, seed, k, pattern)


@functools.lru_cache(maxsize=None)
def _ranks(name: str, G: int, seed: int, effect_group) -> np.ndarray:
    gid = gid_of(name)
    S = gid.size
    X = planted_ranks(G, S, seed)
    if effect_group is not None:                      # planted_ranks shifts its genes in the columns S // 2 ..: hand those to the group
        inside = np.flatnonzero(gid == effect_group)
        assert inside.size == S - S // 2, (name, effect_group, inside.size)
        order = np.empty(S, dtype=np.int64)
        order[inside] = np.arange(S // 2, S)
        order[np.flatnonzero(gid != effect_group)] = np.arange(S // 2)
        X = X[:, order]
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


def ranks(name: str, G: int, seed: int, effect_group=None) -> np.ndarray:
    """tie-free Int64 (query_cases.planted_ranks): every sample a permutation of 0 .. G - 1; effect_group: the columns with the planted
    genes shifted are those of that group (which must hold half of the samples).  Read-only."""
    return _ranks(name, G, seed, effect_group)


@functools.lru_cache(maxsize=None)
def _planted_ties(name: str, G: int, seed: int, n: int) -> np.ndarray:
    gid = gid_of(name)
    X = tie_rich(G, gid.size, seed, np.zeros(gid.size, dtype=bool))             # gene levels and ties, no effect yet
    for g in range(1, int(gid.max()) + 1):                                       # n genes up and n down in every group but the first
        at = 2 * n * (g - 1)
        X[at: at + n, gid == g] += 4
        X[at + n: at + 2 * n, gid == g] -= 4
    X = np.asfortranarray(X.astype(np.int64))
    X.setflags(write=False)
    return X


def planted_ties(name: str, G: int, seed: int, n: int = 6) -> np.ndarray:
    """tie-rich Int64 (query_cases.tie_rich) with few planted genes, so that an iteration converges on them: genes 2 n (g - 1) ..
    2 n (g - 1) + n - 1 are 4 higher in group g >= 1 and the next n are 4 lower.  Read-only."""
    return _planted_ties(name, G, seed, n)


@functools.lru_cache(maxsize=None)
def _float_ties(name: str, G: int, seed: int, k: int) -> np.ndarray:
    gid = gid_of(name)
    rng = np.random.default_rng(seed)
    X = np.round(0.6 * rng.normal(0.0, 1.0, size=(G, gid.size)) + 0.5 * rng.normal(0.0, 1.0, size=(G, 1)), 2)
    X[: G // 8, gid != k] += 1.5
    X[G // 8: G // 4, gid != k] -= 1.5
    X = np.asfortranarray(X)
    X.setflags(write=False)
    return X


def float_ties(name: str, G: int, seed: int, k: int = 0) -> np.ndarray:
    """Float64 rounded to two decimals (masked_pairs_cases.float_case's kind): ties inside the 0.1 band in every group, an effect in the
    samples outside group k for a quarter of the genes.  Read-only."""
    return _float_ties(name, G, seed, k)


def random_valid(name: str, G: int, seed: int, frac: float = 0.30) -> np.ndarray:
    """a validity mask with `frac` of the cells missing at random, plus the four special genes of masked_pairs_cases.special_rows"""
    import masked_pairs_cases as mpc
    gid = gid_of(name)
    rng = np.random.default_rng(seed)
    V = mpc.random_mask(rng, G, gid.size, frac)
    return mpc.special_rows(V, gid, rng)
