"""The top-scoring family at 12, 15 and 16 position planes on ordinary data: reo_rank_shift, reo_top_pairs, reo_top_partners,
reo_top_pairs_null, reo_top_partners_null and reo_top_pairs_loo (csrc/queries.hip; band_chain.h, top_count.h) at the gene counts of
tests/plane_cases.py -- either side of 4 095 / 4 096 and 32 767 / 32 768, one gene into a pad, 9 000 genes (planes 12 - 14 carry ranks) and
65 535 (plane 15) -- on tie-free Int64, on tie-rich Int64 and once on Float64 in the 0.1 band.  Every check is an equality.  The expected
values are the restatements of tests/top_plane_cases.py: D of every gene, every pair inside a set of 300 genes, every cell of about eight
query rows across all partners.  tests/test_top_plane_cases_cpu.py holds them to the whole-matrix restatements on small cases and shows
that the cases have ties on both sides, cannot be matched by a chain blind to the upper planes, and that no comparison here is blind.

Every context carries a class table, a reference set and a pass, and what reo_get_codes, reo_get_ref_mask and reo_get_info say of them is
read before the queries and again after them.

The second half runs many genes and a wide sample axis together: `cross`, 9 000 genes x 1 050 samples in 34 blocks (the family above, and
reo_sample_counts, reo_pair_support, reo_sample_tests, reo_sample_calls, the masked and the permuted build through the helpers of their
own test files), and `big_wide`, 65 600 genes x 265 samples: the 17-plane forms of the last three beyond S = 8."""
import numpy as np
import pytest

import masked_pairs_cases as mpc
import plane_cases as pc
import sample_counts_cases as scc
import top_plane_cases as tc
import wide_top_pairs_cases as wt
from oracle import reo_numpy as rn
import test_gpu_pair_support as tps
import test_gpu_sample_calls as tcalls
import test_gpu_sample_counts as tcnt
import test_gpu_sample_tests as ttests
from test_gpu_masked_pairs import open_masked
from test_gpu_perm_null import open_ctx
from test_gpu_planes import same_arrays
from test_gpu_top_partners_null import overall_is

pytestmark = pytest.mark.gpu

OWN = ("planes_on_demand", "top_pairs_hist_us", "top_pairs_emit_us", "top_pairs_null_batch", "top_pairs_null_us", "top_pairs_loo_words_us",
       "top_pairs_loo_select_us", "top_partners_count_us", "top_partners_select_us", "top_partners_null_batch", "top_partners_null_us")


class Opened:
    """a context with the matrix, a class table and one pass; leaving it checks that the queries in between disturbed none of them"""

    def __init__(self, pkg, X, gid, kind, seed=11):
        self.G, self.kind = X.shape[0], kind
        self.ctx = pkg.Context(device=0, seed=seed)
        self.ctx.set_groups(gid, 2)
        self.ctx.compute_thresholds(0.01)
        self.ctx.set_matrix(X)
        self.ctx.build_pairs(0)
        ref = np.zeros(self.G, dtype=bool)
        ref[:: max(self.G // 200, 1)] = True
        self.ctx.identify_degs(ref, 1.0, 0.05, 1, 0)

    def __enter__(self):
        ctx = self.ctx
        self.keep = pc.rectangles(self.G)[2]
        self.before = ctx.get_codes(*self.keep), ctx.ref_mask(), ctx.info()
        info = self.before[2]
        assert info["has_ties"] == (self.kind != "ranks") and info["Gp"] == pc.padded(self.G), info   # which form of the kernels runs
        return ctx

    def __exit__(self, kind, value, tb):
        try:
            if kind is None:
                ctx = self.ctx
                codes, ref, info = self.before
                assert np.array_equal(ctx.get_codes(*self.keep), codes) and np.array_equal(ctx.ref_mask(), ref)
                after = ctx.info()
                assert all(after[k] == info[k] for k in info if k not in OWN), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        finally:
            self.ctx.close()
        return False


def opened(pkg, G, kind):
    X, gid = tc.case(G, kind)
    return Opened(pkg, X, gid, kind)


def check_shift_pairs_and_partners(ctx, e, tag):
    """checks 1 - 3: D of every gene; every pair inside the gene set; the query rows in chunks of 1 024 partners and their head"""
    G, m = e.mask.size, e.genes.size
    D = ctx.rank_shift()
    assert D.dtype == np.int64 and D.shape == (G,) and not tc.diff_shift(D, e), (tag, np.flatnonzero(D[e.computed] != e.D[e.computed])[:4])
    tp = ctx.top_pairs(m * (m - 1) // 2, gene_mask=e.mask)
    assert not tc.diff_pairs(tp, e.top), (tag, tc.diff_pairs(tp, e.top))
    if e.partner_mask is not None:
        got = ctx.top_partners(e.q, tc.CHUNK, partner_mask=e.partner_mask)
        assert not tc.diff_partners(got, e.rows_full), (tag, tc.diff_partners(got, e.rows_full))
        return
    for lo, hi in tc.chunks(G):
        chunk = np.zeros(G, dtype=bool)
        chunk[lo:hi] = True
        got = ctx.top_partners(e.q, tc.CHUNK, partner_mask=chunk)
        want = [tc.cut_row(r, lo, hi) for r in e.rows_full]
        assert not tc.diff_partners(got, want), (tag, lo, tc.diff_partners(got, want))
    head = ctx.top_partners(e.q, tc.CHUNK)
    assert not tc.diff_partners(head, e.rows_full), (tag, "head", tc.diff_partners(head, e.rows_full))


def check_the_two_nulls(ctx, e, tag):
    """checks 4 and 5, and I2: on the observed row a query's maximum is |N| of its first partner"""
    got = ctx.top_pairs_null(e.label_rows, gene_mask=e.mask, cuts=e.cuts)
    assert not tc.diff_null(got, e.null), (tag, tc.diff_null(got, e.null), got, e.null)
    assert ctx.info()["top_pairs_null_batch"] == tc.B_ROWS
    rows = ctx.top_partners_null(e.label_rows, e.q, cuts=e.pcuts)
    assert not tc.diff_pnull(rows, e.pnull), (tag, tc.diff_pnull(rows, e.pnull), rows.max_num, e.pnull.max_num)
    first = ctx.top_partners(e.q, 1)
    assert np.array_equal(rows.max_num[0], np.abs(first.num[:, 0])) and (first.n_found == 1).all(), tag


@pytest.mark.parametrize("G,kind", tc.cases())
def test_shift_pairs_and_partners(pkg, G, kind):
    """reo_rank_shift for every gene; reo_top_pairs inside the 300 genes: all 44 850 pairs, counts, N, Gamma and order; reo_top_partners of
    the query genes in chunks of 1 024 partners that cover every gene, and the head of the rows without a mask.  The Float64 case knows D
    inside the 300 genes only: its rows are listed inside them."""
    with opened(pkg, G, kind) as ctx:
        check_shift_pairs_and_partners(ctx, tc.expected(G, kind), (G, kind))


@pytest.mark.parametrize("G,kind", tc.cases())
def test_the_two_nulls(pkg, G, kind):
    """17 label rows -- the observed labels, the inverted ones, 15 shuffles: a launch group of 16 and one row.  reo_top_pairs_null inside
    the 300 genes with the cuts 0, 1, the observed maximum and one above; reo_top_partners_null of the query genes over all partners"""
    with opened(pkg, G, kind) as ctx:
        check_the_two_nulls(ctx, tc.expected(G, kind), (G, kind))


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_every_gene_a_query_at_9000(pkg, kind):
    """I1 where planes 12 - 14 carry ranks: the rows of reo_top_partners_null over all 9 000 genes reduce to reo_top_pairs_null without a
    mask on the same context, label row by label row; the columns of the query genes are those of the restatement"""
    G = 9000
    e = tc.expected(G, kind)
    with opened(pkg, G, kind) as ctx:
        every = ctx.top_partners_null(e.label_rows)
        glob = ctx.top_pairs_null(e.label_rows)
    overall_is(every, glob, (G, kind))
    assert np.array_equal(every.max_num[:, e.q], e.pnull.max_num) and np.array_equal(every.arg_partner[:, e.q], e.pnull.arg_partner)


@pytest.mark.parametrize("G,kind", tc.loo_cases())
def test_leave_one_out(pkg, G, kind):
    """reo_top_pairs_loo, kmax = 5, inside about 120 genes: every fold's picks, N, Gamma of the fold and the outcome, the cut and the
    number of candidates"""
    want = tc.expected_loo(G, kind)
    with opened(pkg, G, kind) as ctx:
        got = ctx.top_pairs_loo(tc.KMAX, gene_mask=tc.mask_of(tc.loo_genes(G, kind), G))
    assert not tc.diff_loo(got, want), (G, kind, tc.diff_loo(got, want))
    assert want.cut > 0 and (want.gene_i[want.side != 2] >= 0).all()


@pytest.mark.parametrize("n", tc.CAP_N)
def test_the_capacity_at_its_floor(pkg, monkeypatch, n):
    """9 000 genes with ties, the first n of the 44 850 pairs inside the 300 genes.  With the default capacity one histogram pass leaves
    fewer candidates than records; with REO_TOP_PAIRS_CAP at n, the lowest the library takes, the select must refine through the digits of
    |N|, Gamma and (i, j) -- k_top_pairs<HIST> under a non-empty prefix -- until exactly n keys are left.  The passes are those of
    wide_top_pairs_cases.select_passes, the model of tp_select; the answer is the same."""
    G, kind = 9000, "ties"
    e = tc.expected(G, kind)
    with opened(pkg, G, kind) as ctx:
        wide = ctx.top_pairs(n, gene_mask=e.mask)
        monkeypatch.setenv("REO_TOP_PAIRS_CAP", str(n))                           # (read per call)
        tight = ctx.top_pairs(n, gene_mask=e.mask)
        monkeypatch.delenv("REO_TOP_PAIRS_CAP")
    assert not tc.diff_pairs(wide, e.top, n) and not tc.diff_pairs(tight, e.top, n), (n, tc.diff_pairs(wide, e.top, n), tc.diff_pairs(tight, e.top, n))
    assert tight.passes > wide.passes
    assert (wide.passes, tight.passes) == (wt.select_passes(e.top, G, n, wt.default_capacity(n))[0], wt.select_passes(e.top, G, n, n)[0])


# ---- many genes and a wide sample axis together: 9 000 genes, 520 + 530 samples under shuffled labels, 34 blocks

def cross_opened(pkg, kind):
    X, gid = tc.cross_case(kind)
    return Opened(pkg, X, gid, kind)


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_shift_pairs_and_partners(pkg, kind):
    with cross_opened(pkg, kind) as ctx:
        assert ctx.info()["sample_slots"] // 32 == tc.CROSS_BLOCKS
        check_shift_pairs_and_partners(ctx, tc.cross_expected(kind), ("cross", kind))


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_nulls_and_every_gene_a_query(pkg, kind):
    """the two nulls against the restatements, and I1 over all 9 000 genes"""
    e = tc.cross_expected(kind)
    with cross_opened(pkg, kind) as ctx:
        assert ctx.info()["sample_slots"] // 32 == tc.CROSS_BLOCKS
        check_the_two_nulls(ctx, e, ("cross", kind))
        every = ctx.top_partners_null(e.label_rows)
        glob = ctx.top_pairs_null(e.label_rows)
    overall_is(every, glob, ("cross", kind))
    assert np.array_equal(every.max_num[:, e.q], e.pnull.max_num) and np.array_equal(every.arg_partner[:, e.q], e.pnull.arg_partner)


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_leave_one_out(pkg, kind):
    """1 050 folds inside 40 genes"""
    want = tc.cross_expected_loo(kind)
    with cross_opened(pkg, kind) as ctx:
        got = ctx.top_pairs_loo(tc.KMAX, gene_mask=tc.mask_of(tc.cross_loo_genes(kind), tc.CROSS_G))
    assert not tc.diff_loo(got, want), (kind, tc.diff_loo(got, want))
    assert want.cut > 0 and (want.gene_i >= 0).all() and want.gene_i.shape == (1050, tc.KMAX)


# ---- the plane-reading query kernels and the derived tables on `cross`

def cross_query_case(kind):
    X, gid = tc.cross_case(kind)
    return X, gid, tc.labels_of(gid), pc.query_genes(tc.CROSS_G), tc.cross_partner_mask(pc.query_marks(tc.CROSS_G))


def layout_is(ctx, G, blocks, ties):
    info = ctx.info()
    assert info["Gp"] == pc.padded(G) and info["sample_slots"] // 32 == blocks and info["has_ties"] == ties, info


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_sample_counts(pkg, kind):
    """reo_sample_counts over 34 blocks in five chunks and three tiles, more than 2 048 listed partners in the first tile; ties=True and
    False; tie-rich and tie-free"""
    X, gid, labels, q, pm = cross_query_case(kind)
    assert pm[:4096].sum() > 2048
    with tcnt.open_ctx(pkg, X, labels, pval_reo=0.01) as ctx:
        layout_is(ctx, tc.CROSS_G, tc.CROSS_BLOCKS, kind == "ties")
        got, exp = tcnt.check(ctx, X, q, tcnt.ALL, pm, pkg)
        assert got.n_sel.tolist() == [int(pm.sum()) - int(pm[i]) for i in q] and got.n_sel.max() > 2048
        assert exp[1].max() > 2048 and (exp[2].sum() == 0 if kind == "ranks" else exp[2].max() > 255)   # counts past eleven and past eight counter planes
        assert len({tuple(c) for c in exp[1].T.tolist()}) > 500                  # the columns differ: their order is checked
        tcnt.check(ctx, X, q, tcnt.ALL, pm, pkg, ties=False)
        tcnt.check(ctx, X, q, "reversed", pm, pkg)


def test_cross_sample_counts_of_every_gene(pkg):
    """all 9 000 genes in one call: 32 MiB hold 7 710 count rows of 1 088 slots, so the batch seam occurs with nothing set.  32 rows are
    compared, those on either side of the seam among them"""
    X, gid, labels, _, pm = cross_query_case("ties")
    rows = tc.cross_rows_checked()
    assert tc.CROSS_BATCH == 7710 and {tc.CROSS_BATCH - 1, tc.CROSS_BATCH} <= set(rows.tolist()) and rows.size == 32
    with tcnt.open_ctx(pkg, X, labels, pval_reo=0.01) as ctx:
        layout_is(ctx, tc.CROSS_G, tc.CROSS_BLOCKS, True)
        every = ctx.sample_counts(np.arange(tc.CROSS_G, dtype=np.int32), tcnt.ALL, pm)
        assert every.n_gt.shape == (tc.CROSS_G, X.shape[1])
        codes = {int(i): ctx.get_codes(int(i), int(i) + 1, 0, tc.CROSS_G)[0] for i in rows}
    for at in range(0, rows.size, 8):                                            # (eight rows of states at a time: 9 000 x 1 050 cells each)
        part = rows[at: at + 8]
        n_sel, n_gt, n_eq = scc.expected_counts(X, lambda i: codes[i], part, tcnt.ALL, pm)
        assert np.array_equal(every.n_sel[part], n_sel) and np.array_equal(every.n_gt[part], n_gt) and np.array_equal(every.n_eq[part], n_eq), part


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_pair_support(pkg, kind):
    """reo_pair_support with outcomes over 1 050 samples: rows of the query genes, the marks among every row's partners"""
    X, gid, labels, q, _ = cross_query_case(kind)
    csr = tc.row_lists(q, pc.query_marks(tc.CROSS_G), tc.CROSS_G, 61)
    with tps.open_plain(pkg, X, labels) as ctx:                                  # no table is built: only the transform runs, in the first call
        ps, exp = tps.check(ctx, X, gid, csr, pkg, outcomes=True)
        layout_is(ctx, tc.CROSS_G, tc.CROSS_BLOCKS, kind == "ties")
        assert exp[0].max() > 255 and (exp[1].sum() == 0 if kind == "ranks" else exp[1].sum() > 0) and (exp[2] == 0).any()
        tps.check(ctx, X, gid, csr, pkg, ties=False, exp=exp)


def test_cross_sample_tests_and_calls(pkg):
    """reo_sample_tests of the genes on either side of the tile seam: the integers bit for bit, the tails against the exact ones under
    the tolerance of their background (2 100 tables of some 2 700 partners: the cost of this test); then reo_sample_calls of all four
    query genes against the host route on the same context"""
    X, gid, labels, q, pm = cross_query_case("ties")
    with ttests.open_ctx(pkg, X, labels, pval_reo=0.01) as ctx:
        layout_is(ctx, tc.CROSS_G, tc.CROSS_BLOCKS, True)
        two = q[np.isin(q, (4095, 4096))]
        got, exp = ttests.check(ctx, X, two, pm, pkg, tag="cross")
        assert two.size == 2 and int((got.n_above_ctrl + got.n_below_ctrl).max()) > 100 and exp["u"].max() > 50 and exp["d"].max() > 50 and exp["tied"].max() > 0
        _, st, calls, cut = tcalls.check(ctx, q, pm, 1.0, 0.2, "cross")
        assert (calls != 0).any()
        tcalls.check(ctx, q, pm, 0.05, 1.0, "cross, pval_deg", st)


def cross_masked_case():
    X, gid = tc.cross_case("ties")
    seed = tc.SEED + 13
    return X, np.asfortranarray(mpc.random_mask(np.random.default_rng(seed), tc.CROSS_G, X.shape[1], pc.MASKED_FRAC)), gid, seed


def test_cross_masked_counts(pkg):
    """reo_pair_counts_masked on the rectangles of 9 000 genes, 10 % of the cells missing"""
    X, V, gid, seed = cross_masked_case()
    with open_masked(pkg, X, V, gid, seed) as ctx:
        for rect in pc.rectangles(tc.CROSS_G):
            got = ctx.pair_counts_masked(*rect)
            want = pc.masked_counts_block(X, V, gid, 2, rect)
            for name, g, w in zip(("n_gt", "n_eq", "n_avail"), got, want):
                assert g.dtype == np.int32
                same_arrays(g, w, ("cross", rect, name))
            assert want[1].max() > 64 and want[2].max() > 255
        layout_is(ctx, tc.CROSS_G, tc.CROSS_BLOCKS, True)                        # (the transform ranks the whole matrix: the mask hides no tie from it)


@pytest.mark.parametrize("at", range(len(pc.rectangles(tc.CROSS_G))))
def test_cross_masked_codes(pkg, at):
    """reo_build_pairs_masked(0) + reo_get_codes on the same rectangles, one a test: the coins of a rectangle are drawn one by one on the host"""
    X, V, gid, seed = cross_masked_case()
    G = tc.CROSS_G
    rect = pc.rectangles(G)[at]
    with open_masked(pkg, X, V, gid, seed) as ctx:
        mc = mpc.default_min_complete(np.bincount(gid), 0, 0.01)
        assert tuple(ctx.build_pairs_masked(0)) == mc
        assert ctx.info()["masked_build"] == 1
        layout_is(ctx, G, tc.CROSS_BLOCKS, True)
        same_arrays(ctx.get_codes(*rect), pc.masked_codes_block(X, V, gid, 2, rect, 0, 0.01, mc, seed), ("cross", rect))


@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_cross_perm_codes(pkg, kind):
    """reo_perm_codes under two shuffled label rows on the rectangles; the resident table stays"""
    X, gid = tc.cross_case(kind)
    G, seed = tc.CROSS_G, tc.SEED + 14
    sizes = np.bincount(gid)
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        layout_is(ctx, G, tc.CROSS_BLOCKS, kind == "ties")
        thr = (rn.threshold(int(sizes[0])), rn.threshold(int(sizes[1])))
        assert tuple(int(t) for t in ctx.get_thresholds()[:, 0]) == thr
        keep = pc.rectangles(G)[2]
        before = ctx.get_codes(*keep)
        for row in pc.perm_rows(gid, seed):
            assert int(row.sum()) == int(sizes[0])
            for rect in pc.rectangles(G):
                same_arrays(ctx.perm_codes(row, 0, *rect), pc.permuted_codes_block(X, row, thr, seed, rect), ("cross", kind, rect))
                same_arrays(ctx.get_codes(*keep), before, ("cross", kind, rect, "resident table"))


# ---- 65 600 genes, 17 planes, on 10 sample blocks: the BIG forms beyond S = 8

def big_wide():
    X, gid, pm = tc.big_wide_case()
    return X, gid, tc.labels_of(gid), np.asarray(tc.BIG_WIDE_Q, dtype=np.int32), pm


def test_big_wide_pair_support(pkg):
    X, gid, labels, q, _ = big_wide()
    csr = tc.row_lists(q, tc.BIG_WIDE_MARKS, tc.BIG_WIDE_G, 61)
    with tps.open_plain(pkg, X, labels) as ctx:
        ps, exp = tps.check(ctx, X, gid, csr, pkg, outcomes=True)
        layout_is(ctx, tc.BIG_WIDE_G, 10, True)
        assert exp[0].sum() > 0 and exp[1].sum() > 0 and (exp[2] == 0).any()
        tps.check(ctx, X, gid, csr, pkg, ties=False, exp=exp)


def test_big_wide_sample_tests_and_calls(pkg):
    X, gid, labels, q, pm = big_wide()
    with ttests.open_ctx(pkg, X, labels, pval_reo=0.01) as ctx:
        layout_is(ctx, tc.BIG_WIDE_G, 10, True)
        got, exp = ttests.check(ctx, X, q, pm, pkg, tag="big_wide")
        assert int((got.n_above_ctrl + got.n_below_ctrl).max()) > 100 and exp["u"].max() > 50 and exp["d"].max() > 50
        _, st, calls, cut = tcalls.check(ctx, q, pm, 1.0, 0.2, "big_wide")
        assert (calls != 0).any()
        tcalls.check(ctx, q, pm, 0.05, 1.0, "big_wide, pval_deg", st)
