"""tests/plane_cases.py without a GPU: the rectangle restatements equal the whole-matrix functions they restate, and the seeded cases of
tests/test_gpu_planes.py cannot be passed by a kernel that ignores the upper position planes or never meets a tie, a coin, a short side."""
import functools

import numpy as np
import pytest

import masked_pairs_cases as mpc
import perm_null_cases as pnc
import plane_cases as pc
import sample_counts_cases as scc
from oracle import reo_numpy as rn

SMALL = {"ties70": lambda: mpc.float_case(70, (12, 9), 0.30, 0x5EED0E70) + (2,),
         "ranks130": lambda: mpc.rank_case(130, (12, 9), 0.30, 0x5EED0E71, level=0.8, shift=2.0, planted=16) + (2,),
         "three": lambda: mpc.float_case(70, (10, 12, 9), 0.30, 0x5EED0E72, shift=2.0, planted=8) + (3,)}


def small_rects(G):
    """above the diagonal, below it, across it, and the ragged corner"""
    return [(0, 20, G - 40, G), (G - 25, G, 0, 30), (10, 50, 20, 60), (G - 9, G, G - 30, G)]


@pytest.mark.parametrize("name", sorted(SMALL))
def test_block_restatements_equal_the_whole_matrix_functions(name):
    X, V, gid, ng = SMALL[name]()
    G = X.shape[0]
    seed = 0x5EED0E7F
    counts = mpc.masked_counts(X, V, gid, ng)
    sizes = np.bincount(gid, minlength=ng)
    mcs = {k: (mpc.default_min_complete(sizes, k, 0.01), (3, 4)) for k in range(ng)}     # the default (8 at 0.01) and a low one: few short sides
    whole = {(k, mc): mpc.masked_codes(counts, k, 0.01, mc, seed) for k in range(ng) for mc in mcs[k]}
    rows = pnc.shuffled_rows(gid, ng - 1, 2, 5)
    thr = [(rn.threshold(int(r.sum())), rn.threshold(int(r.size - r.sum()))) for r in rows]
    perm = [pnc.permuted_codes(X, r, t, seed) for r, t in zip(rows, thr)]
    assert (counts[1][np.triu_indices(G, 1)] > 0).any() == (name != "ranks130")
    for rect in small_rects(G):
        i0, i1, j0, j1 = rect
        got = pc.masked_counts_block(X, V, gid, ng, rect)
        for g, w in zip(got, counts):
            assert g.dtype == np.int32 and np.array_equal(g, w[i0:i1, j0:j1]), (name, rect)
        for (k, mc), w in whole.items():
            code = pc.masked_codes_block(X, V, gid, ng, rect, k, 0.01, mc, seed)
            assert code.dtype == np.uint8 and np.array_equal(code, w[i0:i1, j0:j1]), (name, rect, k, mc)
        for r, t, w in zip(rows, thr, perm):
            assert np.array_equal(pc.permuted_codes_block(X, r, t, seed, rect), w[i0:i1, j0:j1]), (name, rect)
    assert all(len(np.unique(w)) >= 6 for (k, mc), w in whole.items() if mc == (3, 4))   # the small cases are not one class throughout
    assert all(len(np.unique(w)) >= 6 for w in perm)


def test_gene_counts_pads_and_rectangles():
    assert [pc.plane_bits(G) for G in pc.PLANE_G] == [12, 15, 15, 15, 16, 16] and set(pc.DEEP_G) <= set(pc.PLANE_G)
    assert [pc.padded(G) for G in pc.PLANE_G + pc.PAD_G] == [4096, 4096, 9216, 32768, 32768, 65536, 5120, 33792]
    assert [pc.plane_bits(G) for G in pc.PAD_G] == [15, 16]
    for G in pc.PLANE_G + pc.PAD_G:
        rects = pc.rectangles(G)
        assert len(rects) == 3 + (G >= 4196) + (G >= 32868)
        for i0, i1, j0, j1 in rects:
            assert 0 <= i0 < i1 <= G and 0 <= j0 < j1 <= G and (i1 - i0) * (j1 - j0) <= 8000
        assert rects[0][2] > rects[0][1] and rects[1][0] > rects[1][3]            # wholly above, wholly below the diagonal
        assert rects[2][1] == G and rects[2][3] == G
        assert pc.sides(G) == ((33, 12) if G in pc.DEEP_G else (12, 9))
    assert {pc.boundary_kind(G) for G in pc.PLANE_G} == set(pc.KINDS)


@functools.lru_cache(maxsize=None)
def deep_case(which, G, kind):
    """the matrix, the labels and the seed as the GPU tests take them, and the sample ranks"""
    if which == "masked":
        X, V, gid, seed = pc.masked_case(G, kind)
    else:
        (X, gid, seed), V = pc.perm_case(G, kind), None
    return X, V, gid, seed, pc.sample_ranks(X)


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("G", pc.DEEP_G)
@pytest.mark.parametrize("which", ["masked", "perm"])
def test_every_deep_rectangle_changes_under_truncated_ranks(which, G, kind):
    """A condition on the seeds, not a measurement: with 45 samples per pair the counts of nearly every pair change when the ranks are
    cut to 12 bits (and, at 65 535 genes, to 15); a quarter of every rectangle is asked for."""
    X, V, gid, seed, R = deep_case(which, G, kind)
    # the partitions of the samples that the GPU test counts under: the groups under the mask, or the sides of its two label rows
    parts = [gid] if which == "masked" else [(1 - row).astype(np.int32) for row in pc.perm_rows(gid, seed)]
    for rect in pc.rectangles(G):
        for part in parts:
            true = pc.masked_counts_block(X, V, part, 2, rect)[0]                 # the gt counts inside the expectation of the GPU test
            full = pc.truncated_gt(X, part, rect, 18, R, V)
            if kind == "ranks":
                assert np.array_equal(full, true), rect                           # tie-free: comparing ranks is comparing values
            for bits in (12, 15) if G > 32767 else (12,):
                cut = pc.truncated_gt(X, part, rect, bits, R, V)
                for ref in (true, full):
                    changed = (cut != ref).any(axis=-1)
                    assert changed.mean() >= 0.25, (which, G, kind, rect, bits, float(changed.mean()))


@pytest.mark.parametrize("G", pc.DEEP_G)
def test_tie_rich_deep_cases_hold_every_code_ties_on_both_sides_and_both_reasons(G):
    X, V, gid, seed, _ = deep_case("masked", G, "ties")
    sizes = np.bincount(gid)
    seen, why = set(), {}
    for rect in pc.rectangles(G):
        code, d = pc.masked_codes_block(X, V, gid, 2, rect, 0, 0.01, mpc.default_min_complete(sizes, 0, 0.01), seed, detail=True)
        seen |= set(np.unique(code).tolist())
        for key, val in d.items():
            why[key] = why.get(key, 0) + int(val.sum())
        assert (d["eq_c"] & d["eq_t"]).any(), rect                               # pairs with ties on both sides, in every rectangle
    assert seen >= set(range(9)), seen
    assert why["short_t"] > 0 and why["nomaj_c"] > 0 and why["nomaj_t"] > 0, why   # (33 samples with 10 % missing are never short)
    X, _, gid, seed, _ = deep_case("perm", G, "ties")
    rows = pc.perm_rows(gid, seed)
    thr = (rn.threshold(int(sizes[0])), rn.threshold(int(sizes[1])))
    seen = set()
    for row in rows:
        assert int(row.sum()) == int(sizes[0])
        for rect in pc.rectangles(G):
            code, d = pc.permuted_codes_block(X, row, thr, seed, rect, detail=True)
            seen |= set(np.unique(code).tolist())
            assert (d["eq_a"] & d["eq_b"]).any(), rect
    assert seen >= set(range(9)), seen
    assert not np.array_equal(rows[0], rows[1]) and (rows[1] != (gid == 0)).sum() == 2


@pytest.mark.parametrize("kind", pc.KINDS)
@pytest.mark.parametrize("G", pc.DEEP_G)
def test_masked_deep_cases_have_both_reasons_for_class_2(G, kind):
    X, V, gid, seed, _ = deep_case("masked", G, kind)
    sizes = np.bincount(gid)
    for k in (0, 1):
        why = {}
        classes = set()
        for rect in pc.rectangles(G):
            code, d = pc.masked_codes_block(X, V, gid, 2, rect, k, 0.01, mpc.default_min_complete(sizes, k, 0.01), seed, detail=True)
            classes |= set(np.unique(code).tolist())
            for key, val in d.items():
                why[key] = why.get(key, 0) + int(val.sum())
        assert why["short_c"] + why["short_t"] > 0 and why["nomaj_c"] + why["nomaj_t"] > 0, (k, why)
        assert len(classes - {255}) >= 7, classes                                 # stable, unstable and reversed pairs all occur


@pytest.mark.parametrize("G", pc.DEEP_G)
def test_query_rows_change_under_truncated_ranks(G):
    """the tie-free matrix of the query tests: every query gene's counts against the marked partners change under 12 (15) bits"""
    X = pc.query_ranks(G, pc.SEED + G)
    assert X.dtype == np.int64 and all(np.array_equal(np.sort(X[:, s]), np.arange(G)) for s in range(X.shape[1]))
    gid = np.array([0, 1] * 4, dtype=np.int32)
    R = pc.sample_ranks(X)
    marks = pc.query_marks(G)
    for q in pc.query_genes(G):
        rect = (int(q), int(q) + 1, 0, G)
        full = pc.truncated_gt(X, gid, rect, 18, R)
        for bits in (12, 15) if G > 32767 else (12,):
            changed = (pc.truncated_gt(X, gid, rect, bits, R) != full).any(axis=-1)[0]
            assert changed.mean() >= 0.25 and changed[[m for m in marks if m != q]].any(), (G, int(q), bits)


@pytest.mark.parametrize("G", pc.QUERY_G)
def test_int64_query_cases_have_ties_among_the_marked_partners(G):
    """values below 30 000 tie rarely: the seeds are those at which at least two query genes meet an equal value among their partners"""
    X, pm = scc.plane_case_data(G, pc.query_marks(G), pc.QUERY_SEED[G])
    q = pc.query_genes(G)
    assert q[0] == 0 and q[-1] == G - 1 and pm[pc.query_marks(G)].all() and 1000 <= pm.sum() <= 1006
    ties = [int((X[pm] == X[i][None, :]).sum()) - 8 * int(pm[i]) for i in q]
    assert sum(t > 0 for t in ties) >= 2, ties
