"""tests/multi_plane_cases.py without a GPU: its references equal the whole-table oracle and tests/test_gpu_contrasts.composed_rows on a
few hundred genes; the seeded cases of tests/test_gpu_multi_planes.py hold all nine classes in every table and ties exactly where they
claim to, and cannot be matched by a borrow chain that ignores the upper position planes; every comparison of the GPU file fails on one
planted error."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import big_plane_cases as bp
import multi_plane_cases as mc
import plane_cases as pc
import sharding_mirror
from test_gpu_contrasts import composed_rows

ALL_CASES = sorted(set(mc.SHARED_CASES + mc.RECOUNT_CASES + mc.WG_COUNT_CASES + mc.WG_TWO_CASES + mc.PASS_CASES + mc.SHARD_CASES))
SMALL = [(G, kind, layout) for G, layout in ((300, "even"), (450, "uneven"), (333, "two")) for kind in mc.KINDS]


def _small(oracle, G, kind, layout):
    p = mc.problem(G, kind, layout)
    return p, np.asfortranarray(p.X.astype(np.float64)), bp.thresholds(oracle, p.gid, p.ngroups, mc.PVAL_REO)


def test_the_cases_cover_every_form_at_15_and_16_planes():
    assert [pc.plane_bits(G) for G in mc.GENES] == [15, 15, 15, 15, 16, 16] and [pc.padded(G) for G in mc.GENES] == [4096, 5120, 9216, 32768, 32768, 65536]
    assert np.bincount(mc.labels("even")).tolist() == [9, 9, 9] and mc.labels("even")[:4].tolist() == [0, 1, 2, 0]
    assert np.bincount(mc.labels("uneven")).tolist() == [33, 12, 9] and mc.labels("uneven")[:3].tolist() == [0, 1, 2]
    assert np.bincount(mc.labels("two")).tolist() == [8, 8]
    assert (np.diff(np.flatnonzero(mc.labels("uneven") == 0)) > 1).any()                   # not one run of samples: the transform re-orders them
    forms = lambda cases: {(pc.plane_bits(G), mc.HAS_TIES[kind]) for G, kind, _ in cases}   # noqa: E731
    every = {(nb, t) for nb in (15, 16) for t in (0, 1)}
    assert forms(mc.SHARED_CASES) == forms(mc.RECOUNT_CASES) == forms(mc.WG_TWO_CASES) == every
    assert forms(c for c in mc.SHARED_CASES if c[0] in mc.CONTRAST_G) == every
    assert forms(mc.WG_COUNT_CASES) == {(15, 0), (15, 1), (16, 1)}                         # (what the issue asks of k1_group_counts)
    assert {G for G, _, _ in mc.SHARED_CASES} == set(mc.GENES) and {c for c in mc.SHARED_CASES if c[2] == "uneven"} == {(9000, "free", "uneven"), (9000, "counts", "uneven"), (65535, "counts", "uneven")}
    assert len({mc.seed_of(*c) for c in ALL_CASES + mc.WIDE_CASES}) == len(ALL_CASES) + 3
    assert mc.WIDE_CASES == [(4200, "counts", "wide2"), (4200, "free", "wide2"), (4200, "counts", "wide3")] and pc.plane_bits(mc.WIDE_G) == 15
    for G in mc.GENES:
        named = mc.blocks(G)
        assert len(named) == len(pc.rectangles(G)) + 4 + 3
        assert [b for n, b in named.items() if n[0] == "rows"] == [(0, 8, 0, G), (G // 2 - 4, G // 2 + 4, 0, G), (G - 8, G, 0, G)]
        assert all(0 <= i0 < i1 <= G and 0 <= j0 < j1 <= G for i0, i1, j0, j1 in named.values())


@pytest.mark.parametrize("G,kind,layout", SMALL)
def test_references_equal_the_whole_table_oracle_and_composed_rows(oracle, G, kind, layout):
    """(1) the one-vs-rest codes of every block equal oracle.build_codes for every k; (2) the contrast codes equal composed_rows off the
    diagonal and hold 255 on it -- on the rectangles, the column strips and the row strips as the GPU file cuts them"""
    p, Xf, thr = _small(oracle, G, kind, layout)
    C = p.ngroups
    whole = {k: oracle.build_codes(Xf, p.gid, C, k, thr[:, k], p.seed) for k in range(C)}
    contrasts = mc.CONTRASTS + [(2, 0), (1, 2)] if C == 3 else []
    cache = {}
    for name, block in mc.blocks(G).items():
        i0, i1, j0, j1 = block
        got = mc.block_codes(oracle, Xf, p.gid, thr, p.seed, C, block, tuple(range(C)), tuple(contrasts))
        for k in range(C):
            assert got[k].dtype == np.uint8 and np.array_equal(got[k], whole[k][i0:i1, j0:j1]), (name, k)
        if contrasts:
            rows, off = composed_rows(oracle, Xf, p.gid, C, thr, p.seed, i0, i1, contrasts, cache)
            for ct in contrasts:
                want = np.where(off, rows[ct], 255)[:, j0:j1]
                assert np.array_equal(got[ct], want), (name, ct)
    if C == 3:
        assert not np.array_equal(whole[0], whole[1]) and len(cache) > 0
    ties = oracle.pair_counts(Xf, p.gid, C, 0, 40, 40, G)[1].sum()
    assert (ties > 0) == bool(p.has_ties)


@pytest.mark.parametrize("G,kind,layout", ALL_CASES)
def test_every_table_of_a_gpu_case_holds_all_nine_classes(oracle, G, kind, layout):
    """(3) conditions on the seeds: in the union of a case's blocks every comparison and every ordered contrast used has all nine classes
    and the diagonal; the rectangles alone hold at least eight of them; ties occur exactly in the tie-rich matrix, in every rectangle"""
    ref = mc.reference(oracle, G, kind, layout)
    assert ref.X.dtype == np.int64 and set(ref.codes) == set(ref.ks) | set(ref.contrasts)
    assert len(ref.contrasts) == (4 if (G in mc.CONTRAST_G and ref.ngroups == 3) else 0)
    for table, per in ref.codes.items():
        seen = sum(np.bincount(c.ravel(), minlength=256) for c in per.values())
        assert (seen[:9] > 0).all() and seen[255] > 0 and seen[9:255].sum() == 0, (table, seen[:9])
        in_rects = sum(np.bincount(c.ravel(), minlength=256) for name, c in per.items() if name[0] == "rect")
        assert (in_rects[:9] > 0).sum() >= 8, (table, in_rects[:9])
    if kind == "free":
        assert (np.sort(ref.X, axis=0) == np.arange(G)[:, None]).all()                     # a permutation per sample: no tie anywhere
    else:
        Xf = np.asfortranarray(ref.X.astype(np.float64))
        for rect in pc.rectangles(G):
            eq = oracle.pair_counts(Xf, ref.gid, ref.ngroups, *rect)[1].astype(np.int64)
            off = np.not_equal(*pc.grid(rect))
            assert (eq[off].sum(axis=0) > 0).all(), rect                                   # pairs that tie, in every group
            assert ((eq[off] > 0).sum(axis=-1) >= 2).any(), rect                           # ... and in two groups at once


@pytest.mark.parametrize("G,kind,layout", [c for c in ALL_CASES if c[0] in mc.DEEP_G])
def test_every_deep_rectangle_changes_under_truncated_ranks(G, kind, layout):
    """(4) a condition on the cases: the gt counts of every group, in every rectangle, change when the ranks are cut to 12 bits (and, at
    65 535 genes, to 15) -- in a quarter of the rectangle's pairs at least.  A chain that ignored the upper planes matches no rectangle"""
    p = mc.problem(G, kind, layout)
    R = pc.sample_ranks(p.X)
    for rect in pc.rectangles(G):
        full = pc.truncated_gt(p.X, p.gid, rect, 18, R)
        if kind == "free":
            assert np.array_equal(full, pc._pair_counts(p.X, None, p.gid, p.ngroups, *pc.grid(rect))[0]), rect   # tie-free: comparing ranks is comparing values
        for bits in (12, 15) if G > 32767 else (12,):
            changed = pc.truncated_gt(p.X, p.gid, rect, bits, R) != full
            assert changed.any(axis=(0, 1)).all(), (rect, bits)                            # every group
            assert changed.any(axis=-1).mean() >= 0.25, (rect, bits, float(changed.any(axis=-1).mean()))


# ------------------------------------------------------------------------------------------- more than 65 535 samples

def test_wide_counts_equal_the_oracles_pair_counts(oracle):
    """WideCounts, the numpy counts of the wide cases, on 300 genes x 500 Int32 samples in three groups (group 0 the large one, as there):
    oracle.pair_counts on blocks above, below and across the diagonal -- but for the diagonal's n_eq, which it leaves at zero"""
    G, S = 300, 500
    gid = np.zeros(S, dtype=np.int32)
    gid[7::40], gid[11::50] = 1, 2
    X = np.asfortranarray(np.random.default_rng(3).integers(0, 60, size=(G, S), dtype=np.int32))
    cnt = mc.WideCounts(X, gid, 3, ties=True, threads=2)
    free = mc.WideCounts(X, gid, 3, ties=False, threads=2)
    for block in ((0, 40, 100, 300), (260, 300, 0, 200), (100, 260, 90, 130), (0, 300, 292, 300)):
        egt, eeq = (c.astype(np.int64) for c in oracle.pair_counts(X.astype(np.float64), gid, 3, *block))
        d = np.arange(max(block[0], block[2]), min(block[1], block[3]))
        assert (eeq[d - block[0], d - block[2]] == np.bincount(gid)).all()
        eeq[d - block[0], d - block[2]] = 0
        gt, eq = cnt.pair_counts(None, gid, 3, *block)
        assert gt.dtype == np.int64 and np.array_equal(gt, egt) and np.array_equal(eq, eeq) and eeq.sum() > 0, block
        gt, eq = free.pair_counts(None, gid, 3, *block)
        assert np.array_equal(gt, egt) and not eq.any()


def _ranks(X, sel):
    """plane_cases.sample_ranks of the genes `sel` for a wide column-major Int32 matrix with values below 2^50 / 8 192: the number of genes
    strictly smaller, int32, len(sel) x S.  A sample's genes are sorted as keys value << 13 | gene, 2 048 samples at a time on threads"""
    G, S = X.shape
    assert G <= 8192 and X.flags.f_contiguous
    R = np.empty((len(sel), S), dtype=np.int32)
    at = np.arange(G, dtype=np.int32)[None, :]

    def chunk(a):
        x = X[:, a:a + 2048].T                                                             # samples x genes, no copy
        keys = np.sort((x.astype(np.int64) << 13) | at, axis=1)
        order, xs = keys & 8191, keys >> 13
        new = np.concatenate([np.ones((len(xs), 1), dtype=bool), xs[:, 1:] != xs[:, :-1]], axis=1)
        first = np.maximum.accumulate(np.where(new, at, 0), axis=1)                       # the position of the first of a run of equal values
        r = np.empty(first.shape, dtype=np.int32)
        np.put_along_axis(r, order, first, axis=1)
        R[:, a:a + 2048] = r[:, sel].T

    with ThreadPoolExecutor(mc.THREADS) as ex:
        list(ex.map(chunk, range(0, S, 2048)))
    return R


@pytest.mark.parametrize("G,kind,layout", mc.WIDE_CASES)
def test_wide_cases_hold_all_nine_classes_and_change_under_truncated_ranks(oracle, G, kind, layout):
    """conditions (3) and (4) on the wide recipes: all nine classes and the diagonal in every table; ties exactly in the tie-rich matrix;
    the gt counts of every group, in every rectangle, change when the ranks are cut to 12 bits"""
    ref = mc.reference(oracle, G, kind, layout)
    assert pc.plane_bits(G) == 15 and ref.X.dtype == np.int32 and ref.X.flags.f_contiguous and ref.X.shape[1] == 65536
    sizes = np.bincount(ref.gid).tolist()
    assert sizes == ([65505, 31] if layout == "wide2" else [65505, 16, 15]) and ref.gid[:2].tolist() == [0, 1]
    assert -(-sizes[0] // 32) == 2048 > 2047                                               # a side of more than one run of the wide count loop
    assert len(ref.blocks) == len(pc.rectangles(G)) + 2 == 6 and set(ref.codes) == set(ref.ks)
    for table, per in ref.codes.items():
        seen = sum(np.bincount(c.ravel(), minlength=256) for c in per.values())
        assert (seen[:9] > 0).all() and seen[255] > 0 and seen[9:255].sum() == 0, (table, seen[:9])
    xs = np.sort(ref.X[:, ::97], axis=0)
    assert ((xs[1:] == xs[:-1]).any(axis=0)).all() == (kind == "counts") and ((xs[1:] == xs[:-1]).any()) == (kind == "counts")
    # the rectangles' genes alone, gene-major, ranks whole and cut to 12 bits
    rects = pc.rectangles(G)
    sel = np.unique(np.concatenate([np.arange(a, b) for i0, i1, j0, j1 in rects for a, b in ((i0, i1), (j0, j1))]))
    R = _ranks(ref.X, sel)
    assert np.array_equal(R[:, :3], pc.sample_ranks(np.asarray(ref.X[:, :3]))[sel])
    assert R.max() >= 4096
    at = lambda g: int(np.searchsorted(sel, g))                                            # noqa: E731
    counted = [mc.WideCounts(np.asfortranarray(M), ref.gid, ref.ngroups, ties=False) for M in (R, R & 4095)]
    for i0, i1, j0, j1 in rects:
        block = (at(i0), at(i0) + i1 - i0, at(j0), at(j0) + j1 - j0)
        full, cut = (c.pair_counts(None, ref.gid, ref.ngroups, *block)[0] for c in counted)
        if kind == "free":
            values = mc.WideCounts(np.asfortranarray(ref.X[sel]), ref.gid, ref.ngroups, ties=False).pair_counts(None, ref.gid, ref.ngroups, *block)[0]
            assert np.array_equal(full, values)                                            # tie-free: comparing ranks is comparing values
        changed = cut != full
        assert changed.any(axis=(0, 1)).all() and changed.any(axis=-1).mean() >= 0.25, ((i0, i1, j0, j1), float(changed.any(axis=-1).mean()))


# ------------------------------------------------------------------------------------------- planted errors: every comparison can fail

@pytest.fixture(scope="module")
def small_ref(oracle):
    """the reference of a 600-gene tie-rich case, with the contrasts"""
    G = 600
    p, Xf, thr = _small(oracle, G, "counts", "even")
    named = mc.blocks(G)
    codes = {}
    for name, block in named.items():
        for table, c in mc.block_codes(oracle, Xf, p.gid, thr, p.seed, 3, block, p.ks, tuple(mc.CONTRASTS)).items():
            c.setflags(write=False)
            codes.setdefault(table, {})[name] = c
    whole = oracle.build_codes(Xf, p.gid, 3, 1, thr[:, 1], p.seed)
    from types import SimpleNamespace
    return SimpleNamespace(**vars(p), thr=thr, blocks=named, codes=codes, whole=whole)


def _reader(ref, table, shift=0, flip=None):
    """get_codes of a device that holds the reference's table: shifted by `shift` columns, or with one cell of one block flipped"""
    def read(i0, i1, j0, j1):
        name = {b: n for n, b in ref.blocks.items()}[(i0, i1, j0, j1)]
        c = ref.codes[table][name].copy()
        if shift and name[0] == "cols":
            c = ref.whole[i0:i1, j0 + shift:j1 + shift].copy()
        if flip is not None and name == flip[0]:
            a, b = flip[1]
            c[a, b] = 4 if c[a, b] != 4 else 5
        return c
    return read


def test_one_flipped_code_fails_the_table_comparisons(small_ref):
    ref = small_ref
    for table in list(ref.ks) + mc.CONTRASTS:
        got = mc.check_table(_reader(ref, table), ref, table)
        assert set(got) == set(ref.blocks)
        mc.check_same_tables(got, ref.codes[table], ref.blocks)
    j0 = bp.ref_runs(ref.G)[2]
    for name, cell, where in ((("cols", j0), (599, 31), (599, j0 + 31)), (("rows", 296), (7, 0), (303, 0)), (("rect", 2), (0, 0), (591, 530)),
                              (("cols", j0), (j0 + 3, 3), (j0 + 3, j0 + 3))):                      # the last one is on the diagonal
        for table in (1, (2, 1)):
            with pytest.raises(AssertionError, match=rf"first \({where[0]}, {where[1]}\)"):
                mc.check_table(_reader(ref, table, flip=(name, cell)), ref, table, "planted")
            bad = {n: (_reader(ref, table, flip=(name, cell))(*b)) for n, b in ref.blocks.items()}
            with pytest.raises(AssertionError, match=rf"first \({where[0]}, {where[1]}\)"):
                mc.check_same_tables(bad, ref.codes[table], ref.blocks, "planted")
    with pytest.raises(AssertionError):                                                     # a block missing from one reading
        mc.check_same_tables({n: c for n, c in ref.codes[1].items() if n != ("rect", 0)}, ref.codes[1], ref.blocks)
    # a table of another comparison, or the contrast the other way round, is not the table
    for a, b in ((1, 0), ((2, 1), (1, 0)), ((0, 1), (1, 0))):
        with pytest.raises(AssertionError):
            mc.check_table(_reader(ref, a), ref, b)


def test_a_strip_shifted_by_one_column_fails(small_ref):
    ref = small_ref
    mc.check_table(_reader(ref, 1, shift=0), ref, 1)
    with pytest.raises(AssertionError, match="cells differ"):
        mc.check_table(_reader(ref, 1, shift=1), ref, 1, "planted")
    with pytest.raises(AssertionError):                                                     # (the strip at column 0 comes back empty)
        mc.check_table(_reader(ref, 1, shift=-1), ref, 1, "planted")
    # ... and the tallies over the reference set see it as well
    strips = mc.column_strips(ref, 1)
    shifted = {j0: ref.whole[:, j0 + 1:j0 + 1 + bp.STRIP] for j0 in list(strips)[:3]}
    shifted[list(strips)[3]] = strips[list(strips)[3]]
    with pytest.raises(AssertionError, match="genes differ"):
        bp.check_tally(bp.ref_set_tally(shifted), bp.ref_set_tally(strips), what="planted")


def test_one_count_off_by_one_fails_the_tally_comparisons(oracle, small_ref):
    ref = small_ref
    ref0 = bp.ref_set(ref.G)
    strips = mc.column_strips(ref, 1)
    assert list(strips) == bp.ref_runs(ref.G)
    exp = bp.ref_set_tally(strips)
    bp.check_tally(oracle.tally(ref.whole, ref0), exp)
    for gene, c in ((0, 0), (ref.G - 1, 8), (299, 4)):
        bad = exp.copy()
        bad[gene, c] += 1
        with pytest.raises(AssertionError, match=rf"first gene {gene}:"):
            bp.check_tally(bad, exp, what="planted")
    # the shards' sum: raw counters over the strips of two partial tables (what a shard does not own is class 4) give the tallies
    # over ref_set; with one cell lost by both shards, or counted by both, they do not
    owner = np.random.default_rng(1).integers(0, 2, size=(ref.G, ref.G))
    owner = np.triu(owner) + np.triu(owner, 1).T
    parts = [{j0: np.where((owner[:, j0:j0 + bp.STRIP] == r) | (c == 255), c, 4).astype(np.uint8) for j0, c in strips.items()} for r in range(2)]
    tot = sum(mc.strips_raw_counters(p, sharding_mirror) for p in parts)
    bp.check_tally(sharding_mirror.derive_tallies(tot, ref0), exp)
    j0 = list(strips)[1]
    a = int(np.flatnonzero(strips[j0][:, 5] == 0)[0])                                      # a class other than 4: a cell that has bits
    for change in ("lost", "twice"):
        bad = [{k: v.copy() for k, v in p.items()} for p in parts]
        for p in bad:
            p[j0][a, 5] = 4 if change == "lost" else 0
        tot = sum(mc.strips_raw_counters(p, sharding_mirror) for p in bad)
        with pytest.raises(AssertionError, match=rf"first gene {a}:"):
            bp.check_tally(sharding_mirror.derive_tallies(tot, ref0), exp, what="planted")
