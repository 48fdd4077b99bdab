"""Cases for the forms of the pair kernel that a run with more than two groups takes, and for the forms for more than 65 535 samples, at 15
and 16 position planes (tests/test_gpu_multi_planes.py): gene counts, sample layouts, seeded matrices, the cells a test looks at, and thin
exact references of the one-vs-rest and of the contrast class table ON THOSE CELLS.  No fixtures, no GPU.

plane_bits(G) is 12 up to 4 095 genes, 15 up to 32 767, 16 up to 65 535 (tests/plane_cases.py says what the boundary sizes do and do not
test).  GENES: 4 096 and 32 768, the first of a plane count, no padding column; 9 000 and 65 535, DEEP_G, where the new planes carry ranks
(65 535: Gp = 65 536, a count plane of exactly 2^32 elements, the documented limit of the workgroup forms); 32 767, the last 15-plane count,
and 4 097, whose last gene stands alone in a pad of 1 024.

Three groups: 27 interleaved samples, 9 / 9 / 9 ("even"), or 54 shuffled ones, 33 / 12 / 9 ("uneven": two blocks of 32 sample slots plus
one plus one, padding slots in every group), at pval_reo = 0.1.  Two matrices, both Int64: `free`, every sample a permutation of 0 .. G - 1,
and `counts`, integers in 0 .. 39 -- the recipes of tests/big_plane_cases.py with effects planted in group 1 AND in group 2, so that every
contrast of two groups has reversed pairs.  Two groups ("two"): that file's own recipes, 16 samples.

The cells: the rectangles of plane_cases.rectangles(G); the four column strips of big_plane_cases.ref_runs(G), 32 columns over all rows
(every row tile; their tallies are the tallies over ref_set(G)); three row strips of 8 rows over all columns -- the first rows, rows across
G / 2, the last rows (every column chunk and panel of the workgroup forms, the mirror rule below the diagonal).

The references: the one-vs-rest codes are big_plane_cases.expected_codes; the contrast of group ctrl against group treat is classified by
tests/test_gpu_contrasts._classify (each side held to its own group's thr[0, g]) from nre_g = gt_g + coins of the pair with the SMALLER
index first, the cell holding 8 - c below the diagonal and 255 on it.  Both take their counts from oracle.pair_counts, counted once per
block (Counts).  tests/test_multi_plane_cases_cpu.py holds both to the whole-table oracle on a few hundred genes and asserts what the
seeds below were chosen for: all nine classes in every table, ties exactly in the tie-rich cases, counts that change when the ranks lose
the planes from 12 (from 15) upwards.

More than 65 535 samples (WIDE_G = 4 200 genes, 15 planes): a side of 65 505 samples is 2 048 blocks of 32 slots, one more than a run of
2 047 of the wide count loop; with a second side of 31 samples (16 + 15 with three groups) S = 65 536, the smallest such sample count.  The
matrix is Int32, made in that dtype in a second or two: wide_counts draws a gene level plus a uniform value, 2 800 values wide, so that
every sample has ties and a pair ties in about 23 samples of a side -- one word of the coin stream, which big_plane_cases.coins asserts;
wide_free makes those values unique within a sample.  The counts come from WideCounts, numpy over all samples at once, since
oracle.pair_counts would take minutes; the cells are the rectangles and two column strips of 8 columns.
16 planes with more than 65 535 samples would take a host matrix of 32 768 x 65 536 x 4 bytes = 8.6 GB and is out of scope."""
from __future__ import annotations

import functools
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np

import big_plane_cases as bp
import plane_cases as pc
from test_gpu_contrasts import _classify

GENES = [4096, 4097, 9000, 32767, 32768, 65535]
DEEP_G = [9000, 65535]
CONTRAST_G = [9000, 32768, 65535]
RECOUNT_G = [4096, 9000, 32768, 65535]
KINDS = ("free", "counts")
HAS_TIES = {"free": 0, "counts": 1}
PVAL_REO = bp.PVAL_REO
CONTRASTS = [(0, 1), (2, 1), (1, 0), (0, 2)]
K_ORDER = (2, 0, 1)                      # the order of the builds: the count planes are made by the first, whichever it is
ROW_STRIP = 8
SEED = 0x5EED0C15
THREADS = 8                              # the blocks of a reference are independent: ctypes and numpy release the interpreter lock

WIDE_G = 4200
WIDE_SIDE = 2048 * 32 - 31               # 65 505 samples: 2 048 blocks, the last one with a single sample
WIDE_VALUES = 4000
WIDE_STRIP = 8


def boundary_kind(G):
    """the one matrix of a gene count that is not in DEEP_G: the forms alternate"""
    return KINDS[GENES.index(G) % 2]


def kinds_of(G):
    return KINDS if G in DEEP_G else (boundary_kind(G),)


def gene_cases(genes, uneven=False):
    """(G, kind, layout) of a three-group form at `genes`: both matrices at DEEP_G, one in turn elsewhere; uneven: the 33 / 12 / 9 layout
    at DEEP_G on top, tie-rich and tie-free at 9 000 and tie-rich at 65 535"""
    out = [(G, kind, "even") for G in genes for kind in kinds_of(G)]
    if uneven:
        out += [(G, kind, "uneven") for G, kind in ((9000, "free"), (9000, "counts"), (65535, "counts")) if G in genes]
    return out


SHARED_CASES = gene_cases(GENES, uneven=True)                                   # (a)
RECOUNT_CASES = gene_cases(RECOUNT_G, uneven=True)                              # (c)
WG_COUNT_CASES = [(9000, "free", "even"), (9000, "counts", "even"), (65535, "counts", "even")]                    # (d), three groups
WG_TWO_CASES = [(G, kind, "two") for G in (9000, 32768) for kind in KINDS]      # (d), two groups
PASS_CASES = [(9000, "counts", "even"), (65535, "free", "even")]                # (e)
SHARD_CASES = [(9000, "free", "even"), (9000, "counts", "even")]                # (f)
WIDE_CASES = [(WIDE_G, "counts", "wide2"), (WIDE_G, "free", "wide2"), (WIDE_G, "counts", "wide3")]               # (g)


def labels(layout):
    """group ids in order of first appearance.  even: 0 1 2 0 1 2 ...; uneven: 33 / 12 / 9 shuffled; two: 0 1 0 1 ...; wide2 / wide3: the
    small groups' samples spread evenly through the large one's"""
    if layout == "even":
        return bp.labels(27, 3)
    if layout == "two":
        return bp.labels(bp.S, 2)
    if layout == "uneven":
        rest = np.repeat(np.arange(3, dtype=np.int32), (32, 11, 8))
        return np.concatenate([np.arange(3, dtype=np.int32), rest[np.random.default_rng(SEED).permutation(51)]])
    S = WIDE_SIDE + 31
    gid = np.zeros(S, dtype=np.int32)
    at = 1 + np.arange(31) * ((S - 1) // 31)
    gid[at] = 1 if layout == "wide2" else 1 + np.arange(31) % 2       # 31 samples of group 1, or 16 of group 1 and 15 of group 2
    return gid


def ngroups_of(layout):
    return 2 if layout in ("two", "wide2") else 3


def seed_of(G, kind, layout):
    return SEED + 16 * G + 4 * ("even", "uneven", "two", "wide2", "wide3").index(layout) + KINDS.index(kind)


def _effects(seed, G, gid):
    """G x S: the effects of big_plane_cases._effects in the samples of group 1, and others, under a seed of their own, in group 2"""
    gid = np.asarray(gid)
    return bp._effects(seed, G)[:, None] * (gid == 1)[None, :] + bp._effects(seed + 0x77, G)[:, None] * (gid == 2)[None, :]


def free(G, seed, gid):
    """big_plane_cases.free with the effects of both groups: tie-free, Int64, every sample a permutation of 0 .. G - 1"""
    S_ = len(gid)
    base = (bp._u64(seed + 1, np.arange(G), 0) % bp._U(64)).astype(np.int64)[:, None]
    noise = (bp._u64(seed, np.arange(G)[:, None], np.arange(S_)[None, :]) >> bp._U(44)).astype(np.int64)
    v = (base + _effects(seed, G, gid)) * (1 << 18) + noise
    order = np.argsort(v, axis=0, kind="stable")
    X = np.empty((G, S_), dtype=np.int64)
    np.put_along_axis(X, order, np.broadcast_to(np.arange(G, dtype=np.int64)[:, None], (G, S_)), axis=0)
    return X


def counts(G, seed, gid):
    """big_plane_cases.counts with the effects of both groups: tie-rich, Int64 in 0 .. 39"""
    X = np.random.default_rng(seed).integers(0, 40, size=(G, len(gid)))
    return np.clip(X + 6 * _effects(seed, G, gid), 0, 39).astype(np.int64)


def wide_free(G, seed, gid):
    """Tie-free, Int32, column-major: wide_counts' values times 8 192 plus the gene's index -- no two genes of a sample are equal, and the
    order of two genes is that of their wide_counts values wherever those differ"""
    X = wide_counts(G, seed, gid)
    X *= np.int32(8192)
    X += np.arange(G, dtype=np.int32)[:, None]
    return X


def wide_counts(G, seed, gid):
    """Tie-rich, Int32, column-major: a level per gene (0 .. 7, times 150) plus a uniform draw from 600 .. WIDE_VALUES - 601; in groups
    1 and 2 a tenth of the genes 600 higher or lower.  4 200 genes on 2 800 values: every sample has ties; a pair of one level ties in 1 of
    2 800 samples, about 23 of a side"""
    rng = np.random.default_rng(seed)
    gid = np.asarray(gid)
    X = rng.integers(600, WIDE_VALUES - 600, size=(len(gid), G), dtype=np.int32).T               # (the transpose of a row-major draw is column-major)
    X += (150 * rng.integers(0, 8, size=G, dtype=np.int32))[:, None]
    for k in range(1, int(gid.max()) + 1):
        eff = (600 * rng.choice(np.array([-1, 0, 1], dtype=np.int32), size=G, p=(0.05, 0.9, 0.05))).astype(np.int32)
        cols = np.flatnonzero(gid == k)
        X[:, cols] += eff[:, None]
    return X


def matrix(G, kind, layout, gid, seed):
    if layout.startswith("wide"):
        return (wide_free if kind == "free" else wide_counts)(G, seed, gid)
    if layout == "two":
        return (bp.free if kind == "free" else bp.counts)(G, seed, len(gid), gid)
    return (free if kind == "free" else counts)(G, seed, gid)


def row_strips(G, n=ROW_STRIP):
    """first rows of the three strips of n rows over all columns: the first rows, rows across G / 2, the last rows"""
    return [0, G // 2 - n // 2, G - n]


def blocks(G, layout="even"):
    """{name: (i0, i1, j0, j1)} of the cells a test looks at: ("rect", r), ("cols", j0), ("rows", i0).  The wide cases take two column
    strips of WIDE_STRIP columns, the first and the last, and no row strips: their reference costs 65 536 samples per pair"""
    out = {("rect", r): rect for r, rect in enumerate(pc.rectangles(G))}
    runs = bp.ref_runs(G)
    wide = layout.startswith("wide")
    out.update({("cols", j0): (0, G, j0, j0 + WIDE_STRIP) for j0 in (0, G - WIDE_STRIP)} if wide else {("cols", j0): (0, G, j0, j0 + bp.STRIP) for j0 in runs})
    if not wide:
        out.update({("rows", i0): (i0, i0 + ROW_STRIP, 0, G) for i0 in row_strips(G)})
    return out


class Counts:
    """oracle.pair_counts with the blocks' counts kept: the comparisons and the contrasts of a case classify the same counts.  Stands in
    for the oracle in big_plane_cases.expected_codes, which reads them and leaves them unchanged"""

    def __init__(self, oracle):
        self.oracle, self.kept = oracle, {}

    def pair_counts(self, X, gid, ngroups, i0, i1, j0, j1):
        key = (i0, i1, j0, j1)
        if key not in self.kept:
            gt, eq = self.oracle.pair_counts(X, gid, ngroups, i0, i1, j0, j1)
            d = np.arange(max(i0, j0), min(i1, j1))
            eq[d - i0, d - j0] = 0           # a gene against itself ties in every sample: no pair, no coins (the cell becomes 255 whatever is here)
            gt.setflags(write=False)
            eq.setflags(write=False)
            self.kept[key] = (gt, eq)
        return self.kept[key]


class WideCounts:
    """Counts for more than 65 535 samples, where oracle.pair_counts (16-bit counts, one strided pass over the samples per pair) would
    take minutes: numpy on a gene-major copy of the Int32 matrix, over ALL samples at once, with the small groups counted on their own
    columns and group 0 as the difference.  gt: x_i > x_j, eq: x_i == x_j, int64 (tests/test_multi_plane_cases_cpu.py holds them to
    oracle.pair_counts on a small matrix).  ties=False: eq is not counted -- every sample is known to be tie-free"""

    def __init__(self, X, gid, ngroups, ties=True, threads=THREADS):
        assert X.dtype == np.int32
        self.all = np.ascontiguousarray(X)                                         # gene-major: a gene's samples lie together
        self.small = [np.ascontiguousarray(X[:, np.flatnonzero(np.asarray(gid) == g)]) for g in range(1, ngroups)]
        self.ngroups, self.ties, self.threads, self.kept = ngroups, ties, threads, {}

    @staticmethod
    def _count(M, i0, i1, j, op):
        b = M[j]
        return np.concatenate([np.count_nonzero(op(M[a:min(a + 128, i1)], b), axis=1) for a in range(i0, i1, 128)])

    def pair_counts(self, X, gid, ngroups, i0, i1, j0, j1):
        key = (i0, i1, j0, j1)
        if key not in self.kept:
            out = []
            with ThreadPoolExecutor(self.threads) as ex:
                for op in (np.greater, np.equal) if self.ties else (np.greater,):
                    n = np.empty((i1 - i0, j1 - j0, self.ngroups), dtype=np.int64)
                    total = np.stack(list(ex.map(lambda j: self._count(self.all, i0, i1, j, op), range(j0, j1))), axis=1)
                    for g, M in enumerate(self.small, start=1):
                        n[:, :, g] = np.stack([self._count(M, i0, i1, j, op) for j in range(j0, j1)], axis=1)
                    n[:, :, 0] = total - n[:, :, 1:].sum(axis=2)
                    out.append(n)
            gt, eq = out if self.ties else (out[0], np.zeros_like(out[0]))
            d = np.arange(max(i0, j0), min(i1, j1))
            eq[d - i0, d - j0] = 0
            self.kept[key] = (gt, eq)
        return self.kept[key]


def nre_block(cnt, X, gid, ngroups, seed, block):
    """[i1 - i0, j1 - j0, ngroups] int64: nre_g of every cell's pair with the smaller index first -- its gt count plus the keyed coins of
    (seed, lo, hi, g) where the pair ties (tests/test_gpu_contrasts._nre, for all cells at once); without meaning on the diagonal"""
    i0, i1, j0, j1 = block
    gt, eq = cnt.pair_counts(X, gid, ngroups, i0, i1, j0, j1)
    sizes = np.bincount(gid, minlength=ngroups).astype(np.int64)
    ii = np.arange(i0, i1, dtype=np.int64)[:, None]
    jj = np.arange(j0, j1, dtype=np.int64)[None, :]
    low = ii > jj
    lo, hi = np.broadcast_arrays(np.minimum(ii, jj), np.maximum(ii, jj))
    n = np.empty(gt.shape, dtype=np.int64)
    for g in range(ngroups):
        e = eq[:, :, g].astype(np.int64)
        n[:, :, g] = np.where(low, sizes[g] - gt[:, :, g] - e, gt[:, :, g])
        tied = np.nonzero(e)
        if tied[0].size:
            n[:, :, g][tied] += bp.coins(seed, lo[tied], hi[tied], g, e[tied])
    return n


def contrast_codes(nre, gid, thr, ctrl, treat, block):
    """the class codes of group ctrl against group treat on a block, from nre_block's counts: each side held to its own group's thr[0, g]"""
    i0, i1, j0, j1 = block
    sizes = np.bincount(gid, minlength=nre.shape[2])
    ii = np.arange(i0, i1, dtype=np.int64)[:, None]
    jj = np.arange(j0, j1, dtype=np.int64)[None, :]
    c = _classify(nre, sizes, thr, ctrl, treat)
    return np.where(ii < jj, c, np.where(ii > jj, 8 - c, 255)).astype(np.uint8)


def block_codes(oracle, X, gid, thr, seed, ngroups, block, ks, contrasts=(), cnt=None):
    """{k: codes} and {(ctrl, treat): codes} of one block, its pairs counted once (by cnt; by the oracle without one)"""
    cnt = Counts(oracle) if cnt is None else cnt
    one = {k: bp.expected_codes(cnt, X, gid, thr, seed, *block, ngroups, k) for k in ks}
    if contrasts:
        nre = nre_block(cnt, X, gid, ngroups, seed, block)
        one.update({ct: contrast_codes(nre, gid, thr, *ct, block) for ct in contrasts})
    return one


def problem(G, kind, layout):
    """the matrix (as the context takes it), the labels and the seed of a case; kept, but for the wide cases' 1.1 GB"""
    return _problem.__wrapped__(G, kind, layout) if layout.startswith("wide") else _problem(G, kind, layout)


@functools.lru_cache(maxsize=None)
def _problem(G, kind, layout):
    gid = labels(layout)
    seed = seed_of(G, kind, layout)
    X = matrix(G, kind, layout, gid, seed)
    X.setflags(write=False)
    return SimpleNamespace(G=G, kind=kind, layout=layout, ngroups=ngroups_of(layout), gid=gid, seed=seed, X=X, has_ties=HAS_TIES[kind],
                           Gp=pc.padded(G), ks=K_ORDER if ngroups_of(layout) == 3 else (0,),
                           contrasts=tuple(CONTRASTS) if (G in CONTRAST_G and layout in ("even", "uneven")) else ())


_REFERENCES = {}


def reference(oracle, G, kind, layout):
    """problem(...) with .thr and .codes = {k or (ctrl, treat): {block name: codes}}: every table of the case on every block, computed once
    per process and shared by the tests, read-only"""
    key = (G, kind, layout)
    if key not in _REFERENCES:
        p = problem(G, kind, layout)
        thr = bp.thresholds(oracle, p.gid, p.ngroups, PVAL_REO)
        named = blocks(G, layout)
        if layout.startswith("wide"):       # one block after the other, the threads inside; and one wide case at a time
            for other in [o for o in _REFERENCES if o[2].startswith("wide")]:
                del _REFERENCES[other]
            cnt = WideCounts(p.X, p.gid, p.ngroups, ties=bool(p.has_ties))
            per_block = [block_codes(oracle, p.X, p.gid, thr, p.seed, p.ngroups, b, p.ks, cnt=cnt) for b in named.values()]
            del cnt
        else:
            Xf = np.asfortranarray(p.X.astype(np.float64))
            with ThreadPoolExecutor(THREADS) as ex:
                per_block = list(ex.map(lambda b: block_codes(oracle, Xf, p.gid, thr, p.seed, p.ngroups, b, p.ks, p.contrasts), named.values()))
        codes = {}
        for name, one in zip(named, per_block):
            for table, c in one.items():
                c.setflags(write=False)
                codes.setdefault(table, {})[name] = c
        _REFERENCES[key] = SimpleNamespace(**vars(p), thr=thr, blocks=named, codes=codes)
    return _REFERENCES[key]


def column_strips(ref, table):
    """{j0: G x 32 codes} of a table: what big_plane_cases.ref_set_tally sums"""
    return {name[1]: c for name, c in ref.codes[table].items() if name[0] == "cols"}


# ------------------------------------------------------------- the comparisons of tests/test_gpu_multi_planes.py beyond big_plane_cases'
# (each one fails on a planted error: tests/test_multi_plane_cases_cpu.py)

def check_table(read, ref, table, what=""):
    """every block of a table, read(i0, i1, j0, j1) -> codes, against the reference's by big_plane_cases.check_codes.  Returns what was
    read, {block name: codes}"""
    got = {}
    for name, block in ref.blocks.items():
        got[name] = read(*block)
        bp.check_codes(got[name], ref.codes[table][name], block[0], block[2], f"{what} {table} {name}")
    return got


def check_same_tables(got, want, blocks_, what=""):
    """two readings of a table, cell for cell on every block"""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for name in want:
        bp.check_codes(got[name], want[name], blocks_[name][0], blocks_[name][2], f"{what} {name}")


def strips_raw_counters(strips, mirror):
    """the 8 raw counters of every gene over the genes of ref_set(G), from the column strips of a (partial) class table: `mirror` is
    tests/sharding_mirror.  Cells that a shard does not own decode as class 4 and count nowhere"""
    return sum(mirror.raw_counters(c, np.ones(c.shape[1], dtype=bool)).astype(np.int64) for c in strips.values())
