"""The plane-reading kernels at 12, 15 and 16 position planes: k_pairs_masked / k_counts_masked (csrc/maskedpairs.hip), k_pairs_permuted
(csrc/permpairs.hip), k_sample_counts (csrc/samplecounts.hip, and through it the sample tests and calls) and k_pair_support
(csrc/pairsupport.hip) at the gene counts of tests/plane_cases.py -- either side of 4 095 / 4 096 and 32 767 / 32 768, 9 000 genes (planes
12 - 14 carry ranks) and 65 535, the documented limit of the masked and the permuted build (plane 15).  Every check is an equality.  The
expected tables are numpy restatements on rectangles (no G x G host array exists, no class table is read back whole);
tests/test_plane_cases_cpu.py holds them to the whole-matrix restatements on small cases and shows that none of the rectangles could be
matched by a borrow chain that ignored the upper planes.  The helpers are those of the entry points' own test files."""
import numpy as np
import pytest

import masked_pairs_cases as mpc
import plane_cases as pc
from oracle import reo_numpy as rn
import test_gpu_pair_support as tps
import test_gpu_sample_calls as tcalls
import test_gpu_sample_counts as tcnt
import test_gpu_sample_tests as ttests
from test_gpu_masked_pairs import open_masked
from test_gpu_perm_null import check_null_against_relabelled, open_ctx, rel  # noqa: F401  (rel: the fixture)

pytestmark = pytest.mark.gpu


def same_arrays(got, want, tag):
    assert got.shape == want.shape and np.array_equal(got, want), (tag, int((got != want).sum()), np.argwhere(got != want)[:4].tolist())


# ---- the masked build

def masked_cases():
    out = []
    for G in pc.PLANE_G + pc.PAD_G:
        out += [(G, kind) for kind in (pc.KINDS if G in pc.DEEP_G else ("ties",))]
    return out


@pytest.mark.parametrize("G,kind", masked_cases())
def test_masked_counts_and_codes(pkg, G, kind):
    """reo_pair_counts_masked, then reo_build_pairs_masked(0) + reo_get_codes, on every rectangle against the restatement; at DEEP_G
    tie-free and tie-rich, and the tie-rich run also builds k = 1"""
    X, V, gid, seed = pc.masked_case(G, kind)
    sizes = np.bincount(gid)
    rects = pc.rectangles(G)
    with open_masked(pkg, X, V, gid, seed) as ctx:
        for rect in rects:
            got = ctx.pair_counts_masked(*rect)
            want = pc.masked_counts_block(X, V, gid, 2, rect)
            for name, g, w in zip(("n_gt", "n_eq", "n_avail"), got, want):
                assert g.dtype == np.int32
                same_arrays(g, w, (G, kind, rect, name))
            off = np.not_equal(*pc.grid(rect))
            assert (want[1][off].sum() > 0) == (kind == "ties")
        for k in (0, 1) if (G in pc.DEEP_G and kind == "ties") else (0,):
            mc = mpc.default_min_complete(sizes, k, 0.01)
            assert tuple(ctx.build_pairs_masked(k)) == mc
            info = ctx.info()
            assert info["masked_build"] == 1 and info["Gp"] == pc.padded(G), info
            for rect in rects:
                same_arrays(ctx.get_codes(*rect), pc.masked_codes_block(X, V, gid, 2, rect, k, 0.01, mc, seed), (G, kind, rect, k))


@pytest.mark.parametrize("G,kind", [(9000, "ranks"), (9000, "ties"), (32768, "ranks"), (32768, "ties")])
def test_all_ones_mask_is_the_plain_build(pkg, G, kind):
    """byte for byte in row strips of 500: all of them at 9 000 genes; the first, the last and the one across row 4 096 at 32 768"""
    X, _, gid, seed = pc.masked_case(G, kind)
    sizes = np.bincount(gid)
    strips = list(range(0, G, 500)) if G < 10000 else [0, 3846, G - 500]
    with open_masked(pkg, X, np.ones(X.shape, dtype=bool), gid, seed) as ctx:
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["masked_build"] == 0 and info["has_ties"] == (kind == "ties")
        assert info["k1_slot_order"] == (kind == "ranks"), info                   # the tie-free plain build runs in slot order
        plain = [ctx.get_codes(i0, min(i0 + 500, G), 0, G) for i0 in strips]
        assert len(np.unique(np.concatenate([np.unique(p) for p in plain]))) == 10   # all nine classes and the diagonal
        for mc in (None, (int(sizes[0]), int(sizes[1]))):
            ctx.build_pairs_masked(0, 0.01, mc)
            assert ctx.info()["masked_build"] == 1
            for p, i0 in zip(plain, strips):
                same_arrays(ctx.get_codes(i0, min(i0 + 500, G), 0, G), p, (G, kind, mc, i0))


# ---- the permuted build

def perm_cases():
    out = []
    for G in pc.PLANE_G + pc.PAD_G:
        out += [(G, kind) for kind in (pc.KINDS if G in pc.DEEP_G else (pc.boundary_kind(G),))]
    return out


def check_perm_codes(pkg, rel, G, kind, rows=(0, 1), rects=None):
    """reo_perm_codes on the rectangles against the restatement and against the relabelled plain build; the resident table stays"""
    X, gid, seed = pc.perm_case(G, kind)
    sizes = np.bincount(gid)
    rects = pc.rectangles(G) if rects is None else rects
    r = rel(seed)
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        thr = (rn.threshold(int(sizes[0])), rn.threshold(int(sizes[1])))      # the reference's own thresholds; the context's must be these
        assert tuple(int(t) for t in ctx.get_thresholds()[:, 0]) == thr
        keep = pc.rectangles(G)[2]
        before = ctx.get_codes(*keep)
        for row in pc.perm_rows(gid, seed)[list(rows)]:
            assert int(row.sum()) == int(sizes[0])
            r.build(X, row)
            for rect in rects:
                got = ctx.perm_codes(row, 0, *rect)
                same_arrays(got, pc.permuted_codes_block(X, row, thr, seed, rect), (G, kind, rect, "restatement"))
                same_arrays(got, r.ctx.get_codes(*rect), (G, kind, rect, "relabelled build"))
                same_arrays(ctx.get_codes(*keep), before, (G, kind, rect, "resident table"))
        info = ctx.info()
        assert info["has_ties"] == (kind == "ties") and info["Gp"] == pc.padded(G), info   # which form of k_pairs_permuted ran


@pytest.mark.parametrize("G,kind", perm_cases())
def test_perm_codes(pkg, rel, monkeypatch, G, kind):
    """two shuffled rows; at DEEP_G the tie-free form (TIES = false) and the form with ties, at the other sizes one of them in turn"""
    if G >= 32767:
        monkeypatch.setenv("REO_PERM_BATCH", "1")
    check_perm_codes(pkg, rel, G, kind)


def test_perm_codes_in_the_second_launch_group_at_9000(pkg, rel, monkeypatch):
    """REO_PERM_CODES_SLOT = 17: the table sits 17 x table_words behind the buffer's start, in the second launch group of 16"""
    monkeypatch.setenv("REO_PERM_CODES_SLOT", "17")
    check_perm_codes(pkg, rel, 9000, "ties", rows=(1,))


@pytest.mark.parametrize("G,kind,batch,n_perm", [(9000, "ties", 2, 3), (65535, "ranks", 2, 2)])
def test_perm_null_against_the_relabelled_pass(pkg, rel, monkeypatch, G, kind, batch, n_perm):
    """reo_perm_null with all genes in the reference set: delta1_null, n_up / n_down and se_null bit for bit the relabelled context's pass,
    n_ge the numpy count, the resident table read before and after the call.  9 000 genes: B = 3 in batches of 2.  65 535 genes, the documented limit: B = 2 in one batch, the second table
    5.4e8 words (2.1 GB) behind the first."""
    monkeypatch.setenv("REO_PERM_BATCH", str(batch))
    X, gid, seed = pc.perm_case(G, kind)
    rows = pkg.permuted_labels(gid, 0, n_perm, seed=batch)
    pn, info, called = check_null_against_relabelled(pkg, rel, X, gid, seed, 0, rows, np.ones(G, dtype=bool), keep=pc.rectangles(G)[2])
    assert info["perm_batch"] == batch and info["perm_kernel_us"] > 0 and info["Gp"] == pc.padded(G)
    assert len({d.tobytes() for d in pn.delta1_null}) == n_perm and np.abs(pn.delta1_null).max() > 0


# ---- the queries

@pytest.mark.parametrize("G,tie_free", [(G, False) for G in pc.QUERY_G] + [(G, True) for G in pc.DEEP_G])
def test_sample_counts(pkg, G, tie_free):
    """the case of test_17_plane_layout: queries at the first and the last gene and either side of 4 096 and 32 768, partners marked
    there and at 1 000 random genes, ties=True and False; at DEEP_G also on a tie-free matrix"""
    X = pc.query_ranks(G, pc.SEED + G) if tie_free else None
    tcnt.plane_case(pkg, G, pc.query_genes(G), pc.query_marks(G), pc.QUERY_SEED[G], X)


@pytest.mark.parametrize("G,tie_free", [(G, False) for G in pc.QUERY_G] + [(G, True) for G in pc.DEEP_G])
def test_pair_support(pkg, G, tie_free):
    """big_case: rows for the same genes, the marks among every row's partners, outcomes, ties=True and False; at DEEP_G also on the
    tie-free matrix of the sample counts, whose rows the CPU file shows to change under truncated ranks"""
    X = pc.query_ranks(G, pc.SEED + G) if tie_free else None
    tps.big_case(pkg, G, pc.query_genes(G), pc.query_marks(G), 61 + G, X)


LIMIT_Q = [65534, 0, 40000, 32767, 32768, 7]
LIMIT_MARKS = [0, 4095, 4096, 32767, 32768, 65534]


def test_sample_tests_at_65535(pkg):
    """the six-query case of test_17_plane_layout in the 16-plane layout; the log-factorial table is at its 16-plane maximum"""
    ttests.plane_case(pkg, 65535, LIMIT_Q, LIMIT_MARKS, 61, "16 planes")


def test_sample_calls_at_65535(pkg):
    tcalls.plane_case(pkg, 65535, LIMIT_Q, LIMIT_MARKS, 61, "16 planes")


# ---- planes on demand

@pytest.mark.parametrize("G", [32768, 65535])
def test_planes_on_demand_after_a_slot_build(pkg, rel, monkeypatch, G):
    """tie-free, matrix before groups: the plain build runs in slot order and leaves the gene-order planes unmade; the first reader
    (reo_sample_counts) makes them once, the second (reo_perm_codes) finds them"""
    monkeypatch.setenv("REO_PERM_BATCH", "1")
    seed = pc.SEED + G
    X = pc.query_ranks(G, seed)
    labels = np.array(["a", "b"] * 4, dtype=object)
    gid, _ = pkg.encode_groups(labels)
    q, marks = pc.query_genes(G), pc.query_marks(G)
    pm = np.zeros(G, dtype=bool)
    pm[np.random.default_rng(seed).choice(G, 1000, replace=False)] = True
    pm[marks] = True
    with tcnt.open_ctx(pkg, X, labels, pval_reo=0.3, seed=seed, matrix_first=True) as ctx:
        info = ctx.info()
        assert (info["k1_slot_order"], info["has_ties"], info["planes_on_demand"]) == (1, 0, 0), info
        got, exp = tcnt.check(ctx, X, q, tcnt.ALL, pm, pkg)
        assert exp[1].sum() > 0 and ctx.info()["planes_on_demand"] == 1
        thr = (rn.threshold(4, 0.3), rn.threshold(4, 0.3))
        assert tuple(int(t) for t in ctx.get_thresholds()[:, 0]) == thr
        row = pc.perm_rows(gid, seed)[0]
        r = rel(seed)
        r.build(X, row, pval_reo=0.3)
        keep = pc.rectangles(G)[2]
        before = ctx.get_codes(*keep)
        for rect in pc.rectangles(G)[:3]:
            code = ctx.perm_codes(row, 0, *rect)
            same_arrays(code, pc.permuted_codes_block(X, row, thr, seed, rect), (G, rect, "restatement"))
            same_arrays(code, r.ctx.get_codes(*rect), (G, rect, "relabelled build"))
            same_arrays(ctx.get_codes(*keep), before, (G, rect, "resident table"))
        info = ctx.info()
        assert (info["k1_slot_order"], info["planes_on_demand"]) == (1, 1), info
