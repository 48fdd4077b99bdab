"""The top-scoring-pair family on wide sample axes (reo_top_pairs, reo_rank_shift, reo_top_pairs_null, reo_top_pairs_loo; csrc/toppairs.hip,
toppairsnull.hip, toppairsloo.hip): 10 to 21 blocks of 32 sample slots on the layouts of tests/wide_sample_cases.py, 332 blocks with Gamma at
and above 2^32 (deep_gamma), and 2 048 blocks at the documented limit of 65 535 samples, where 2 S_A S_B = 2^31 - 65 536 (limit) -- the
tests of each entry point stop at four blocks and at Gamma below 2^22.  tests/wide_top_pairs_cases.py has the cases and why each is there;
tests/test_wide_top_pairs_cases_cpu.py asserts, without a GPU, the conditions that keep these tests from passing vacuously and holds the
shortened references to the definitions.  Every comparison is an exact equality against the numpy restatements of the entry points' own
test files -- the helpers are imported from those files --; there is no tolerance anywhere.  Every test asserts the block count it runs at
from info()["sample_slots"], so that a layout changed later cannot fall back to a few blocks.

The leave-one-out is not run at the limit: its 65 535 folds would make the numpy reference the slow part, and what it would add -- N(s)
and Gamma(s) carried as two 32-bit halves through the reductions of k_loo_select, out_g above 2^32, hundreds of sample blocks in grid y of
k_loo_words -- deep_gamma covers with 10 616 folds."""
import numpy as np
import pytest

import top_pairs_loo_cases as lc
import wide_sample_cases as wc
import wide_top_pairs_cases as wt
from test_gpu_top_pairs import identical as tp_identical, same as tp_same
from test_gpu_top_pairs_loo import check as loo_check
from test_gpu_top_pairs_null import identical as null_identical, same as null_same

pytestmark = pytest.mark.gpu

N, K = wt.N, wt.K
ROWS = list(wt.ROWS)


def open_case(pkg, name, seed=11):
    """matrix and groups of a case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = wt.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def blocks(ctx, name):
    """the sample blocks that the context's kernels walk: those of the case, and for a row those of its layout's table"""
    slots = ctx.info()["sample_slots"]
    assert slots % 32 == 0
    nblk = slots // 32
    assert nblk == wt.blocks(name), (name, nblk)
    if name in wt.ROWS:
        assert nblk == wc.LAYOUTS[wt.ROWS[name][0]][3] >= 10, (name, nblk)
    return nblk


def search_both_ways(ctx, monkeypatch, name, a, b):
    """top_pairs(N) at the default capacity and under REO_TOP_PAIRS_CAP = N: the oracle's first N, the same result, more passes"""
    exp = wt.expected(name)
    wide = ctx.top_pairs(N, a=a, b=b)
    tp_same(wide, exp, N, name)
    assert (wide.a, wide.b) == (a, b) and wide.passes >= 1
    monkeypatch.setenv("REO_TOP_PAIRS_CAP", str(N))                               # (read per call)
    tight = ctx.top_pairs(N, a=a, b=b)
    monkeypatch.delenv("REO_TOP_PAIRS_CAP")
    tp_same(tight, exp, N, (name, "tight"))
    assert tp_identical(wide, tight) and tight.passes > wide.passes, (name, wide.passes, tight.passes)
    G = wt.case(name)[0].shape[0]                                                # the passes are those of the pass loop's numpy restatement
    assert wide.passes == wt.select_passes(exp, G, N, wt.default_capacity(N))[0] and tight.passes == wt.select_passes(exp, G, N, N)[0], name
    return wide, tight


# ---- 1. the wide layouts

@pytest.mark.parametrize("name", ROWS)
def test_search_and_rank_shift_across_blocks(pkg, monkeypatch, name):
    exp = wt.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) >= 10
        D = ctx.rank_shift(a=a, b=b)
        assert D.dtype == np.int64 and D.shape == exp.D.shape and np.array_equal(D, exp.D), name
        assert ctx.info()["has_ties"] == (0 if name == "full_ranks" else 1)      # (known once a call has needed the bit planes)
        wide, _ = search_both_ways(ctx, monkeypatch, name, a, b)
        full = 2 * exp.sizes[0] * exp.sizes[1]
        assert np.array_equal(wide.direction, np.sign(exp.num[:N]).astype(np.int8))
        assert np.array_equal(wide.score, np.abs(exp.num[:N]) / float(full))
        if name == wt.LONG_ROW:                                                  # a longer list crosses many equal |N|
            tp_same(ctx.top_pairs(wt.LONG_N, a=a, b=b), exp, wt.LONG_N, (name, wt.LONG_N))


@pytest.mark.parametrize("name", ROWS)
def test_null_across_blocks(pkg, monkeypatch, name):
    """33 label rows (two launch groups and one row) and the six cuts; then in launches of one row and of 20 + 13 rows"""
    exp, rows, cuts = wt.expected_null(name), wt.rows(name), wt.cuts(name)
    full = wt.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) >= 10
        plain = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
        null_same(plain, exp, name)
        assert (plain.a, plain.b) == (a, b) and np.array_equal(plain.cuts, cuts) and tuple(int(v) for v in plain.side_sizes) == full.sizes
        assert ctx.info()["top_pairs_null_batch"] == wt.B_NULL
        assert plain.max_num[0] == abs(int(ctx.top_pairs(1, a=a, b=b).num[0]))
        for batch in (1, 20):                                                    # the seam between launches: read per call
            monkeypatch.setenv("REO_TOP_NULL_BATCH", str(batch))
            got = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
            assert null_identical(got, plain), (name, batch)
            assert ctx.info()["top_pairs_null_batch"] == batch
        monkeypatch.delenv("REO_TOP_NULL_BATCH")
        bare = ctx.top_pairs_null(rows[:17], a=a, b=b)                           # no cuts: no counters
        assert bare.n_reach.shape == (17, 0) and np.array_equal(bare.max_num, exp.max_num[:17])
        assert np.array_equal(bare.arg_i, exp.arg_i[:17]) and np.array_equal(bare.arg_j, exp.arg_j[:17])


@pytest.mark.parametrize("name", ROWS)
def test_leave_one_out_across_blocks(pkg, name):
    """every fold against the incremental restatement of the definition; the cut and the candidates by restate_candidates' rule"""
    exp, band, full = wt.expected_loo(name), wt.expected_loo_candidates(name), wt.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) >= 10
        got = ctx.top_pairs_loo(K, a=a, b=b)
    loo_check(got, exp, name)
    assert (got.a, got.b) == (a, b) and tuple(int(v) for v in got.side_sizes) == full.sizes
    assert (got.cut, got.n_candidates) == (band.cut, band.n_candidates) and got.cut > 0, name
    X, gid, ng, _, _ = wt.case(name)
    neither = lc.sides_of(gid, ng, a, b) == 2
    assert np.array_equal(got.side == 2, neither) and int((~neither).sum()) == sum(full.sizes)
    assert (got.gene_i[neither] == -1).all() and (got.gene_j[neither] == -1).all()
    assert not got.num[neither].any() and not got.rank_num[neither].any() and not got.outcome[neither].any()
    assert (got.gene_i[~neither] >= 0).all()
    v = got.votes()
    assert np.array_equal(v, np.cumsum(np.sign(exp.num) * exp.outcome, axis=1))


def test_gene_mask_across_blocks(pkg):
    """three_groups, 33 against 31 samples with the 300-sample group on neither side, half of the genes: all three entry points"""
    name = wt.MASKED_ROW
    mask = wt.gene_mask(name)
    exp = wt.expected_masked(name)
    rows, cuts = wt.rows(name), wt.cuts(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 13
        tp = ctx.top_pairs(N, a=a, b=b, gene_mask=mask)
        tp_same(tp, exp, N, "half of the genes")
        assert mask[tp.gene_i].all() and mask[tp.gene_j].all() and not tp_identical(tp, ctx.top_pairs(N, a=a, b=b))
        nul = ctx.top_pairs_null(rows, a=a, b=b, gene_mask=mask, cuts=cuts)
        null_same(nul, wt.expected_null_masked(name), "half of the genes")
        assert mask[nul.arg_i].all() and mask[nul.arg_j].all()
        loo = ctx.top_pairs_loo(K, a=a, b=b, gene_mask=mask)
        band = wt.expected_loo_candidates(name, K, True)
        loo_check(loo, wt.expected_loo(name, K, True), "half of the genes")
        assert (loo.cut, loo.n_candidates) == (band.cut, band.n_candidates)
        picked = loo.gene_i >= 0
        assert mask[loo.gene_i[picked]].all() and mask[loo.gene_j[picked]].all()


# ---- 2. Gamma at and above 2^32: 6 016 / 4 600 samples, 332 blocks

def test_deep_gamma_search_and_rank_shift(pkg, monkeypatch):
    """648 pairs at |N| = 2 S_A S_B: Gamma decides, with the high word 0 in some of the first 50 and 1 in the others; the tight buffer
    refines through the digits of Gamma that lie in TpKey.hi"""
    name = "deep_gamma"
    exp = wt.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 332
        D = ctx.rank_shift(a=a, b=b)
        assert D.dtype == np.int64 and np.array_equal(D, exp.D) and ctx.info()["has_ties"] == 1
        wide, tight = search_both_ways(ctx, monkeypatch, name, a, b)
        assert np.unique(wide.rank_num >> 32).tolist() == [0, 1] and tight.passes >= 4
        tp_same(ctx.top_pairs(700, a=a, b=b), exp, 700, "past the 648 pairs")


def test_deep_gamma_null(pkg):
    name = "deep_gamma"
    exp, rows, cuts = wt.expected_deep_null(name), wt.deep_rows(name), wt.deep_cuts(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 332
        got = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
    null_same(got, exp, name)
    assert got.n_reach[0].tolist()[3:] == [648, 648, 0]


def test_deep_gamma_leave_one_out(pkg):
    """10 616 folds, Gamma(s) of the first picks at or above 2^32 and of the last below: the two halves of loo_shfl_xor, and out_g"""
    name = "deep_gamma"
    exp, band, full = wt.expected_loo(name), wt.expected_loo_candidates(name), wt.expected(name)
    assert exp.rank_num.max() >= 2 ** 32
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 332
        got = ctx.top_pairs_loo(K, a=a, b=b)
    loo_check(got, exp, name)
    assert (got.cut, got.n_candidates) == (band.cut, band.n_candidates) == (2 * full.sizes[0] * full.sizes[1] - 4 * full.sizes[0], 648)
    assert (got.side != 2).all() and tuple(int(v) for v in got.side_sizes) == full.sizes


# ---- 3. the sample limit: 32 768 / 32 767 samples, 2 048 blocks, 2 S_A S_B = 2^31 - 65 536

def test_limit_search_and_rank_shift(pkg):
    name = "limit"
    exp = wt.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 2048 and ctx.S == 65535
        D = ctx.rank_shift(a=a, b=b)
        assert D.dtype == np.int64 and np.array_equal(D, exp.D)
        tp = ctx.top_pairs(N, a=a, b=b)
    tp_same(tp, exp, N, name)
    assert int(np.abs(tp.num).max()) == 2 ** 31 - 65536 and int(tp.rank_num.max()) > 2 ** 37
    assert not tp.n_gt[:, 0].any() and (tp.n_gt[:, 1] == 32767).all()           # below in all of side A, above in all of side B


def test_limit_null(pkg):
    """the observed row and two shuffles; the cuts hold 2 S_A S_B, which 360 pairs reach on the observed row, and 2 S_A S_B + 1"""
    name = "limit"
    exp, rows, cuts = wt.expected_deep_null(name), wt.deep_rows(name), wt.deep_cuts(name)
    assert cuts[4] == 2 ** 31 - 65536 and cuts[5] == cuts[4] + 1
    ctx, a, b = open_case(pkg, name)
    with ctx:
        assert blocks(ctx, name) == 2048
        got = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
    null_same(got, exp, name)
    assert got.max_num[0] == cuts[4] and got.n_reach[0].tolist()[3:] == [360, 360, 0]
