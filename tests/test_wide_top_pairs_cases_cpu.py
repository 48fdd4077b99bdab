"""The wide cases of the top-scoring-pair family (tests/wide_top_pairs_cases.py), the parts that need no GPU: the conditions under which
tests/test_gpu_wide_top_pairs.py means something, asserted from the numpy oracles alone -- block counts, ties of a side above 64, counts
above 255, groups on neither side, a band with a cut above 0, Gamma with a high word that varies and decides, the sample limit --, and the
two shortened references held to the definitions they shorten: the incremental restatement of the leave-one-out against
top_pairs_loo_cases (a whole case, then the first, last and block-seam folds of every new case, then the band's picks against the
definition's), and the null's counts by matrix products against top_pairs_null_cases.restate."""
import numpy as np
import pytest

import perm_null_cases as pnc
import top_pairs_cases as tpc
import top_pairs_loo_cases as lc
import top_pairs_null_cases as tnc
import wide_sample_cases as wc
import wide_top_pairs_cases as wt

K = wt.K


# ---- the rows

@pytest.mark.parametrize("name", list(wt.ROWS))
def test_the_rows_reach_what_the_table_says(name):
    layout = wt.ROWS[name][0]
    X, gid, ng, a, b = wt.case(name)
    e = wt.expected(name)
    sizes = np.bincount(gid)
    assert wt.blocks(name) == wc.LAYOUTS[layout][3] >= 10 and X.shape == (wt.ROWS[name][4], gid.size)
    side = lc.sides_of(gid, ng, a, b)
    assert e.sizes == (int((side == 1).sum()), int((side == 0).sum())) and min(e.sizes) >= 20
    n, eq, gt = np.abs(e.num), e.counts[:, 1::2], e.counts[:, 0::2]
    assert 0 < n.max() <= 2 * e.sizes[0] * e.sizes[1] < 2 ** 18 and n.max() >= 1180    # |N| of 1 180 .. 147 840 in front
    if name == "full_ranks":                                                     # tie-free: the TIES = false kernels, and Gamma alone orders the head
        assert not eq.any() and (n[:wt.N] == n[0]).all() and np.unique(e.rank_num[:wt.N]).size > 40
    else:
        assert eq[:wt.N].any() and eq.max() >= 9                                 # ties among the pairs that are returned
    if name == "seam":                                                           # a list of LONG_N crosses many equal |N|
        assert wt.LONG_ROW == name and wt.LONG_N - np.unique(n[:wt.LONG_N]).size > 1000
        m = pnc.slot_map(gid, ng)
        assert sizes.tolist() == [135, 130] and (m[:160] < 0).sum() == 25 and (m[160:] < 0).sum() == 30   # padding in both sides
    if name == "full_ties":
        assert eq.max() > 64 and gt.max() == 256 and (pnc.slot_map(gid, ng) >= 0).all()   # a second word of ties; the ninth bit; no padding slot
    if name == "three_33_31":                                                    # ten blocks of the 300-group take no part
        assert int((side == 2).sum()) == 300 and e.sizes == (33, 31)
    if name == "three_300_rest":
        assert e.sizes == (300, 64) and b is None and ng == 3 and gt.max() > 255
    if name == "padding_30_rest":                                                # side B: 16 groups, 15 of them of 1 .. 3 samples
        assert e.sizes == (30, 50) and ng == 17 and sorted(sizes[np.arange(ng) != a].tolist()) == sorted([1, 2, 3] * 5 + [20])
    if name == "padding_20_30":                                                  # 15 blocks whose live word is 0
        assert e.sizes == (20, 30) and int((side == 2).sum()) == 30 and wt.blocks(name) - 2 == 15
    if name.startswith("padding"):
        assert (pnc.slot_map(gid, ng) < 0).mean() > 0.8
    if name == "contrast_300_260":
        assert e.sizes == (300, 260) and int((side == 2).sum()) == 40 and (gt[:, 0] > 255).any() and (gt[:, 1] > 255).any()


@pytest.mark.parametrize("name", list(wt.ROWS))
def test_the_rows_nulls_are_not_hollow(name):
    """33 rows, 32 of them shuffles: the observed labelling stands out, the shuffles differ among themselves, the cuts divide the pairs"""
    rows, cuts, nul = wt.rows(name), wt.cuts(name), wt.expected_null(name)
    e = wt.expected(name)
    pairs = e.gene_i.size
    assert rows.shape == (wt.B_NULL, wt.case(name)[1].size) and len({r.tobytes() for r in rows}) == wt.B_NULL
    assert ((rows == 2) == (rows[0] == 2)[None, :]).all() and (rows == 1).sum(axis=1).tolist() == [e.sizes[0]] * wt.B_NULL
    assert nul.max_num[0] == abs(int(e.num[0])) == cuts[3] and (nul.arg_i[0], nul.arg_j[0]) == min(
        (int(i), int(j)) for i, j, v in zip(e.gene_i, e.gene_j, e.num) if abs(int(v)) == cuts[3])
    assert (nul.max_num[1:] < nul.max_num[0]).all() and np.unique(nul.max_num).size > 10
    assert (nul.n_reach[:, 0] == pairs).all() and not nul.n_reach[:, 5].any() and pairs // 2 <= nul.n_reach[0, 2] <= pairs and 1 <= nul.n_reach[0, 3] <= nul.n_reach[0, 1] < pairs
    assert list(cuts[:2]) == [0, 1] and cuts[4] == 2 * e.sizes[0] * e.sizes[1] == cuts[5] - 1
    if name == wt.MASKED_ROW:
        mask = wt.gene_mask(name)
        m = int(mask.sum())
        got = wt.expected_null_masked(name)
        assert 40 < m < 90 and (got.n_reach[:, 0] == m * (m - 1) // 2).all() and mask[got.arg_i].all() and mask[got.arg_j].all()
        assert not np.array_equal(got.max_num, nul.max_num)


def test_row_counts_are_masked_counts_under_the_label_rows():
    """wide_top_pairs_cases.row_counts (matrix products) against top_pairs_cases.side_counts on the relabelled groups, and restate_null
    against top_pairs_null_cases.restate: on deep_gamma's three rows and on rows with samples that take no part"""
    for name, rows in (("deep_gamma", wt.deep_rows("deep_gamma")), ("three_33_31", wt.rows("three_33_31")[:4])):
        X = wt.case(name)[0]
        cuts = wt.cuts(name)
        fast = wt.restate_null(X, rows, cuts)
        ref = tnc.restate(X, rows, cuts)
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(fast, ref)), name
        got = wt.row_counts(X, rows[1:2])
        want = tpc.side_counts(X, tnc.relabel(rows[1]), 3, 0, 1)[:4]
        assert all(np.array_equal(g[0], w) for g, w in zip(got, want)), name


@pytest.mark.parametrize("name", list(wt.ROWS) + list(wt.DEEP))
def test_a_buffer_of_50_records_makes_the_pass_loop_refine(name):
    """select_passes restates tp_select (tests/test_top_pairs_cpu.py holds it to the library's own loop): at the default capacity one
    pass, at REO_TOP_PAIRS_CAP = 50 more than one -- through the digits of Gamma in TpKey.hi on deep_gamma and limit"""
    e, G = wt.expected(name), wt.case(name)[0].shape[0]
    wide, tight = wt.select_passes(e, G, wt.N, wt.default_capacity(wt.N)), wt.select_passes(e, G, wt.N, wt.N)
    assert wide[0] == 1 and wt.N <= wide[1] <= e.gene_i.size and tight[0] > 1 and tight[1] == wt.N, (wide, tight)
    if name in wt.DEEP:
        assert tight[0] >= 5 and wide[1] == (648 if name == "deep_gamma" else 360)   # |N| alone: pass 1; Gamma's digits at bits 72, 60, 48, ...


# ---- the incremental restatement of the leave-one-out

def same_order(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("gene_i", "gene_j", "num", "rank_num", "D")) and x.sizes == y.sizes


def test_the_incremental_restatement_equals_the_definition_on_a_whole_case():
    """count_i64 (40 / 24 samples, ties in every sample), K = 5: every fold's whole order, and the picks field by field"""
    name = "count_i64"
    X, gid, ng, a, b = tpc.case(name)
    inc = wt.Incremental(X, gid, ng, a, b)
    for s in range(X.shape[1]):
        assert same_order(inc.fold(s), lc.fold(name, s)), s
    got = lc.restate(X, gid, ng, a, b, K, folds=inc.fold)
    exp = lc.expected(name, K)
    assert lc.same(got, exp) and (got.cut, got.n_candidates) == (exp.cut, exp.n_candidates)
    band = lc.restate_candidates(X, gid, ng, a, b, K, folds=inc.fold, full=tpc.expected(name))
    ref = lc.expected_candidates(name, K)
    assert lc.same(band, ref) and (band.cut, band.n_candidates) == (ref.cut, ref.n_candidates)


def test_the_incremental_restatement_follows_the_element_type_and_the_mask():
    """Float32 is compared in Float32 arithmetic (count_f32), and a gene mask drops pairs but no gene from the rank shifts (float300)"""
    X, gid, ng, a, b = tpc.case("count_f32")
    inc = wt.Incremental(X, gid, ng, a, b)
    for s in (0, 1, X.shape[1] - 1):
        assert same_order(inc.fold(s), lc.fold("count_f32", s)), s
    X, gid, ng, a, b = tpc.case("float300")
    mask = tpc.half_mask(X.shape[0])
    inc = wt.Incremental(X, gid, ng, a, b, mask)
    side = lc.sides_of(gid, ng, a, b)
    for s in (0, 63):
        assert same_order(inc.fold(s), lc.fold_oracle(X, side, s, mask)), s


@pytest.mark.parametrize("name", list(wt.ROWS) + ["deep_gamma"])
def test_the_incremental_folds_equal_the_definition_at_the_ends_and_the_block_seams(name):
    X, gid, ng, a, b = wt.case(name)
    side = lc.sides_of(gid, ng, a, b)
    folds, n_seams = wt.seam_folds(name)
    assert {int(np.flatnonzero(side == v)[e]) for v in (0, 1) for e in (0, -1)} <= set(folds)
    if name == "padding_20_30":                                                  # (two sides of one block each, and the two blocks are no neighbours)
        assert n_seams == 0 and len(folds) == 4
    else:
        assert n_seams >= 1 and len(folds) >= 5
    loo = wt.expected_loo(name)
    for s in folds:
        ref = lc.fold_oracle(X, side, s)
        assert same_order(wt.fold(name, s), ref), (name, s)
        at = lc.greedy(ref, K)
        assert np.array_equal(loo.gene_i[s], ref.gene_i[at]) and np.array_equal(loo.rank_num[s], ref.rank_num[at]), (name, s)


@pytest.mark.parametrize("name", list(wt.ROWS) + ["deep_gamma"])
def test_the_band_holds_every_pick_of_every_fold(name):
    """the bound of csrc/top_pairs_loo.h at these sizes: restate_candidates' walk over the band gives the definition's picks"""
    loo, band = wt.expected_loo(name), wt.expected_loo_candidates(name)
    e = wt.expected(name)
    assert lc.same(loo, band)
    pairs = e.gene_i.size
    assert band.cut > 0 and 2 * K <= band.n_candidates < pairs // 2 and loo.n_candidates == pairs
    assert (loo.gene_i[loo.side != 2] >= 0).all() and (loo.gene_i[loo.side == 2] == -1).all() and not loo.num[loo.side == 2].any()
    assert int((loo.side != 2).sum()) == sum(e.sizes)
    assert len({tuple(g) for g in loo.rank_num[loo.side != 2].tolist()}) > sum(e.sizes) // 4   # the folds differ: their rows are checked
    if name == wt.MASKED_ROW:
        mask = wt.gene_mask(name)
        got, ref = wt.expected_loo(name, K, True), wt.expected_loo_candidates(name, K, True)
        assert lc.same(got, ref) and ref.cut > 0 and mask[got.gene_i[got.side != 2]].all() and not lc.same(got, loo)


# ---- Gamma at and above 2^32, and the sample limit

def by(e: tpc.Oracle, gam, n):
    """the first n (i, j) when `gam` stands in for Gamma in the order"""
    order = np.lexsort((e.gene_j, e.gene_i, -gam, -np.abs(e.num)))[:n]
    return list(zip(e.gene_i[order].tolist(), e.gene_j[order].tolist()))


def test_deep_gammas_high_word_varies_and_decides():
    name = "deep_gamma"
    e = wt.expected(name)
    s_a, s_b, _, m = wt.DEEP[name]
    full = 2 * s_a * s_b
    n = np.abs(e.num)
    assert e.sizes == (s_a, s_b) and wt.blocks(name) == 188 + 144 and full < 2 ** 31
    assert int((n == full).sum()) == m * (wt.G_DEEP - m) == 648 and (e.gene_i[:648] < m).all() and (e.gene_j[:648] >= m).all()
    head = e.rank_num[:wt.N]
    assert np.unique(head >> 32).tolist() == [0, 1] and 1 <= int((e.rank_num[:648] >= 2 ** 32).sum()) < wt.N
    assert e.counts[:, 1::2].max() > 1000                                        # more than a thousand ties of a side in one pair
    first = list(zip(e.gene_i[:wt.N].tolist(), e.gene_j[:wt.N].tolist()))
    assert by(e, e.rank_num, wt.N) == first
    assert by(e, e.rank_num & 0xFFFFFFFF, wt.N) != first and by(e, e.rank_num >> 32, wt.N) != first
    assert set(by(e, e.rank_num & 0xFFFFFFFF, wt.N)) != set(first)               # the low word alone selects other pairs, not only another order
    # the leave-one-out: the cut keeps the 648, and in a fold either half of Gamma alone picks otherwise
    band = wt.expected_loo_candidates(name)
    assert band.cut == full - 4 * s_a and band.n_candidates == 648
    loo = wt.expected_loo(name)
    assert (loo.rank_num[loo.side != 2][:, 0] >= 2 ** 32).all() and (loo.rank_num[loo.side != 2][:, K - 1] < 2 ** 32).all()
    low = high = 0
    for s in (0, 1, s_a + s_b - 1):
        o = wt.fold(name, s)
        want = (loo.gene_i[s].tolist(), loo.gene_j[s].tolist())
        assert wt.picks_with(o, o.rank_num, K) == want
        low += wt.picks_with(o, o.rank_num & 0xFFFFFFFF, K) != want
        high += wt.picks_with(o, o.rank_num >> 32, K) != want
    assert low >= 1 and high >= 1


def test_the_limit_case_sits_on_the_documented_limits():
    name = "limit"
    X, gid, ng, a, b = wt.case(name)
    e = wt.expected(name)
    ref = tpc.oracle(X, gid, ng, a, b)                                            # the expectation by matrix products is the oracle itself
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(e[:6] + e[7:], ref[:6] + ref[7:])) and e.sizes == ref.sizes
    d = wt.expected("deep_gamma")
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(wt.oracle_from_counts(*(c[0] for c in wt._deep_counts("deep_gamma")), *d.sizes), d) if not isinstance(x, tuple))
    s_a, s_b, _, m = wt.DEEP[name]
    full = 2 * s_a * s_b
    assert X.shape == (wt.G_DEEP, 65535) and e.sizes == (32768, 32767) and wt.blocks(name) == 2048
    assert full == 2 ** 31 - 65536 == 2147418112 and full >> 31 == 0 and (full + 1) >> 31 == 0 and full >> 30 == 1   # the top bit of the |N| field
    n = np.abs(e.num)
    assert int((n == full).sum()) == m * (wt.G_DEEP - m) == 360
    head = e.rank_num[:wt.N]
    assert np.unique(head >> 32).size >= 2 and head.max() > 2 ** 37 and int(e.D.max() - e.D.min()) < 2 ** 48
    assert e.counts[:, 1::2].max() > 4096 and e.counts[:, 0::2].max() == 32768   # counts that need 13 and 16 bits
    first = list(zip(e.gene_i[:wt.N].tolist(), e.gene_j[:wt.N].tolist()))
    assert by(e, e.rank_num & 0xFFFFFFFF, wt.N) != first and by(e, e.rank_num >> 32, wt.N) != first
    nul, cuts = wt.expected_deep_null(name), wt.deep_cuts(name)
    assert cuts[4] == full and cuts[5] == full + 1 and nul.n_reach[0].tolist()[3:] == [360, 360, 0] and nul.max_num[0] == full
    assert (nul.max_num[1:] < full // 8).all() and nul.n_reach[1:, 3:].sum() == 0 and (nul.n_reach[:, 0] == 2145).all()
    assert (nul.arg_i[0], nul.arg_j[0]) == (0, m)
