"""The query entries and the derived tables on wide sample axes: 10 to 21 blocks of 32 sample slots, where the tests of each entry point
stop at 5 (tests/wide_sample_cases.py has the layouts and why each is there; tests/test_wide_sample_cases_cpu.py asserts, without a GPU,
the conditions that keep these tests from passing vacuously).  Every comparison is an exact equality against the reference that the entry
point's own test file uses -- the helpers are imported from those files --; the one tolerance is sample_tests_cases.tolerance for the
Fisher tails.  Every test asserts the block count it runs at from info()["sample_slots"], so that a layout changed later cannot fall back
to a single chunk of sample blocks."""
import functools

import numpy as np
import pytest

import masked_pairs_cases as mpc
import perm_null_cases as pnc
import sample_calls_cases as cc
import sample_counts_cases as scc
import wide_sample_cases as wc
from query_cases import code_rows
from test_gpu_contrasts import ORDERED, _check_result, _subset, composed_rows
from test_gpu_masked_pairs import check_counts_and_codes, open_masked
from test_gpu_pair_support import check as support_check, expected as support_expected, make_csr, open_plain
from test_gpu_perm_null import check_codes, check_null_against_relabelled, open_ctx as open_perm, rel  # noqa: F401  (rel: a fixture)
from test_gpu_sample_calls import check as calls_check
from test_gpu_sample_counts import ALL, N13, check as counts_check, open_ctx
from test_gpu_sample_tests import bitwise as st_bitwise, check as st_check

pytestmark = pytest.mark.gpu

G = wc.G_QUERY


def blocks(ctx, name=None):
    """the sample blocks the context's kernels walk and the chunks k_sample_counts cuts them into; name: they are the layout's"""
    slots = ctx.info()["sample_slots"]
    assert slots % 32 == 0
    nblk = slots // 32
    nchunks = -(-nblk // wc.CHUNK_BLOCKS)
    if name is not None:
        assert nblk == wc.LAYOUTS[name][3] == wc.slot_map(name).size // 32 and nchunks == len(wc.LAYOUTS[name][4]), (name, nblk)
    return nblk, nchunks


@functools.lru_cache(maxsize=None)
def query_states(name, k):
    """sample_counts_cases.states of every gene of the query data of (layout, k): made once, read by every test that needs them"""
    gt, eq = scc.states(wc.int_ties(name, G, wc.QUERY_SEED, k), np.arange(G))
    gt.setflags(write=False)
    eq.setflags(write=False)
    return gt, eq


def open_query(pkg, name, k):
    X = wc.int_ties(name, G, wc.QUERY_SEED, k)
    return X, open_ctx(pkg, X, wc.gid_of(name), pval_reo=wc.QUERY_PVAL_REO, k=k)


# ---- a. reo_sample_counts (k_sample_counts; k1_counts behind reo_pair_counts)

@pytest.mark.parametrize("name,k", wc.query_cases())
def test_sample_counts_across_chunks(pkg, name, k):
    """all 130 genes as queries: every chunk of every layout writes its own columns, chunk 0 alone writes n_sel; both WITH_EQ forms"""
    X, ctx = open_query(pkg, name, k)
    with ctx:
        nblk, nchunks = blocks(ctx, name)
        assert nblk >= 10 and nchunks in (2, 3)
        codes = ctx.get_codes(0, G, 0, G)
        assert set(range(9)) <= set(np.unique(codes).tolist())
        rows = {i: codes[i] for i in range(G)}
        q = np.arange(G, dtype=np.int32)
        st = query_states(name, k)
        ones = np.ones(G, dtype=bool)
        pm = np.random.default_rng(wc.QUERY_SEED).random(G) < 0.7
        got, exp = counts_check(ctx, X, q, ALL, ones, pkg, rows, st, (name, "all"))
        assert (got.n_sel == G - 1).all()                                        # written by chunk 0 only, for every query
        assert got.n_gt.shape == (G, X.shape[1]) and (got.n_gt + got.n_eq).max(axis=0).min() > 0   # a count for every real column
        assert len({tuple(c) for c in exp[1].T.tolist()}) > X.shape[1] // 2     # the columns differ: their order is checked
        counts_check(ctx, X, q, "reversed", pm, pkg, rows, st, (name, "reversed"))
        counts_check(ctx, X, q, 0x44, ones, pkg, rows, st, (name, 0x44))
        counts_check(ctx, X, q, 1 << N13, ones, pkg, rows, st, (name, "n13"))
        got, exp = counts_check(ctx, X, q, ALL, pm, pkg, rows, st, (name, "random mask"))
        assert np.array_equal(got.n_sel, (pm[None, :] & ~np.eye(G, dtype=bool)).sum(axis=1))
        counts_check(ctx, X, q, ALL, pm, pkg, rows, st, (name, "no ties"), ties=False)
        counts_check(ctx, X, q, 0x44, ones, pkg, rows, st, (name, "0x44, no ties"), ties=False)
        # the raw entry writes its own rows and nothing behind them
        n_sel, n_gt, n_eq = np.full(G + 8, -7, np.int32), np.full((G + 8, X.shape[1]), -7, np.int32), np.full((G + 8, X.shape[1]), -7, np.int32)
        ctx.sample_counts_raw(q, ALL, np.ascontiguousarray(pm, dtype=np.uint8), n_sel, n_gt, n_eq)
        assert np.array_equal(n_gt[:G], exp[1]) and np.array_equal(n_eq[:G], exp[2]) and np.array_equal(n_sel[:G], exp[0])
        assert (n_gt[G:] == -7).all() and (n_eq[G:] == -7).all() and (n_sel[G:] == -7).all()


def test_sample_counts_batches_of_three_rows_by_two_chunks(pkg, monkeypatch):
    """seam_in_group under REO_SAMPLE_COUNTS_BATCH=3: launches of 3 rows x 2 chunks, a short last batch (130 = 43 x 3 + 1)"""
    name, k = "seam_in_group", 0
    X, ctx = open_query(pkg, name, k)
    with ctx:
        assert blocks(ctx, name) == (10, 2)
        rows = code_rows(ctx, np.arange(G))
        q = np.arange(G, dtype=np.int32)
        st = query_states(name, k)
        pm = np.random.default_rng(3).random(G) < 0.7
        whole, _ = counts_check(ctx, X, q, ALL, pm, pkg, rows, st, "unbatched")
        monkeypatch.setenv("REO_SAMPLE_COUNTS_BATCH", "3")                        # (read per call)
        again, _ = counts_check(ctx, X, q, ALL, pm, pkg, rows, st, "batches of 3")
        for f in ("n_sel", "n_gt", "n_eq"):
            assert getattr(again, f).tobytes() == getattr(whole, f).tobytes(), f
        counts_check(ctx, X, q, "reversed", pm, pkg, rows, st, "batches of 3, no ties", ties=False)


def test_sample_counts_two_tiles_by_two_chunks(pkg):
    """seam_in_group, G = 4 200, the dense mask: a row of two 4 096-column tiles meets two chunks, and the first tile's lanes take 64
    partners each (the seventh counter plane); eight queries on either side of column 4 096"""
    name, Gw = "seam_in_group", 4200
    X = wc.int_ties(name, Gw, 77, 0)
    q = np.concatenate([np.arange(4088, 4096), np.arange(4096, 4104)]).astype(np.int32)
    ones = np.ones(Gw, dtype=bool)
    with open_ctx(pkg, X, wc.gid_of(name)) as ctx:
        assert blocks(ctx, name) == (10, 2)
        rows = code_rows(ctx, q)
        st = scc.states(X, q)
        got, exp = counts_check(ctx, X, q, ALL, ones, pkg, rows, st, "dense")
        assert (got.n_sel == Gw - 1).all() and exp[2].max() > 64 and exp[1].max() > 2048
        counts_check(ctx, X, q, "reversed", ones, pkg, rows, st, "reversed", ties=False)


def test_sample_counts_17_plane_layout_beyond_a_chunk(pkg):
    """G = 65 600 (the BIG instantiation), groups of 257 and 8 samples shuffled: 9 + 1 = 10 blocks, two chunks; queries and partner marks
    as tests/test_gpu_sample_counts.py::test_17_plane_layout"""
    Gb, seed = 65600, 61
    rng = np.random.default_rng(seed)
    gid = wc.first_appearance(rng.permutation(np.repeat([0, 1], [257, 8])))
    X = np.asfortranarray(rng.integers(0, 30000, size=(Gb, gid.size)).astype(np.int64))
    q = np.array([65599, 0, 40000], dtype=np.int32)
    pm = np.zeros(Gb, dtype=bool)
    pm[rng.choice(Gb, 1000, replace=False)] = True
    pm[[0, 4095, 4096, 65535, 65536, 65599]] = True
    with open_ctx(pkg, X, gid, pval_reo=0.3) as ctx:
        assert blocks(ctx) == (10, 2) and sorted(np.bincount(gid).tolist()) == [8, 257]
        got, exp = counts_check(ctx, X, q, ALL, pm, pkg)
        assert got.n_sel.tolist() == [int(pm.sum()) - 1, int(pm.sum()) - 1, int(pm.sum()) - int(pm[40000])]
        assert exp[1].sum() > 0 and exp[2].sum() > 0 and len({tuple(c) for c in exp[1].T.tolist()}) > gid.size // 2
        counts_check(ctx, X, q, ALL, pm, pkg, ties=False)


@pytest.mark.parametrize("name", ["seam_in_group", "three_groups"])
def test_pair_counts_whole_block_against_the_oracle(pkg, oracle, name):
    """reo_pair_counts (k1_counts) over all pairs and groups at the same block structures"""
    X, ctx = open_query(pkg, name, 0)
    gid = wc.gid_of(name)
    ng = int(gid.max()) + 1
    with ctx:
        assert blocks(ctx, name)[0] >= 10
        gt, eq = ctx.pair_counts(0, G, 0, G)
        wgt, weq = oracle.pair_counts(np.asarray(X, dtype=np.float64), gid, ng, 0, G, 0, G)
        assert np.array_equal(gt, wgt) and np.array_equal(eq, weq)
        assert gt.max() > (255 if name == "three_groups" else 100) and eq.max() > 32
        strip = ctx.pair_counts(G // 3, G // 3 + 5, 1, G - 1)                      # a rectangle off the origin
        assert np.array_equal(strip[0], wgt[G // 3: G // 3 + 5, 1: G - 1]) and np.array_equal(strip[1], weq[G // 3: G // 3 + 5, 1: G - 1])


# ---- b. reo_sample_tests and reo_sample_calls (built on k_sample_counts)

@pytest.mark.parametrize("name", ["seam_in_group", "mostly_padding"])
def test_sample_tests_and_calls_across_chunks(pkg, monkeypatch, name):
    """all genes: the five integer arrays, the exact tails, and the calls with cut, n_up and n_down of every sample column, byte for byte
    against the host route; then one call in batches of three rows"""
    k = dict(wc.query_cases())[name]
    X, ctx = open_query(pkg, name, k)
    with ctx:
        nblk, nchunks = blocks(ctx, name)
        assert nblk >= 10 and nchunks == (2 if name == "seam_in_group" else 3)
        q = np.arange(G, dtype=np.int32)
        rows = code_rows(ctx, q)
        st = query_states(name, k)
        pm = np.random.default_rng(wc.QUERY_SEED + 1).random(G) < 0.8
        got, exp = st_check(ctx, X, q, pm, pkg, rows, st, f"{name} random mask")
        assert exp["n_above_ctrl"].sum() > 0 and exp["n_below_ctrl"].sum() > 0 and exp["tied"].sum() > 0
        assert exp["rev_up"].sum() > 0 and exp["rev_down"].sum() > 0
        assert int((exp["n_above_ctrl"].astype(np.int64) + exp["n_below_ctrl"]).max()) < 4200
        assert len({tuple(c) for c in exp["u"].T.tolist()}) > X.shape[1] // 2    # the columns differ: their order is checked
        light = ctx.sample_tests(q, pm, counts=False)
        assert light.p_up.tobytes() == got.p_up.tobytes() and light.p_down.tobytes() == got.p_down.tobytes()
        calls, st_light, want, cut = calls_check(ctx, q, pm, 1.0, 0.2, f"{name} calls", light)
        assert calls.calls.shape == (G, X.shape[1]) and (want == 1).any() and (want == -1).any() and 0 < cut.max()
        assert len({tuple(c) for c in want.T.tolist()}) > 3
        calls_check(ctx, q, pm, 0.05, 0.05, f"{name} both thresholds", light)
        monkeypatch.setenv("REO_SAMPLE_CALLS_BATCH", "3")                         # (read per call)
        cc.bitwise(ctx.sample_calls(1.0, 0.2, q, pm), calls)
        monkeypatch.setenv("REO_SAMPLE_TESTS_BATCH", "3")
        st_bitwise(ctx.sample_tests(q, pm), got)


# ---- c. reo_pair_support (k_pair_support)

@pytest.mark.parametrize("name", ["seam_in_group", "three_groups", "mostly_padding"])
def test_pair_support_across_blocks(pkg, monkeypatch, name):
    """a CSR with empty rows and rows of 64, 65 and 150 entries (one, two and three work items): counts per group and the outcome byte of
    every real column; once more with a batch cut inside every long row"""
    gid = wc.gid_of(name)
    X = wc.int_ties(name, G, wc.QUERY_SEED, 0)
    rng = np.random.default_rng(wc.QUERY_SEED + 2)
    csr = make_csr(rng, G, [0, 64, 0, 0, 65, 150, 0, 7, 0], genes=[5, G - 1, 3, 3, 0, 64, 9, G - 1, 77])
    with open_plain(pkg, X, gid) as ctx:
        assert blocks(ctx, name)[0] >= 10
        exp = support_expected(X, gid, int(gid.max()) + 1, *csr)
        ps, _ = support_check(ctx, X, gid, csr, pkg, ties=True, outcomes=True, tag=name, exp=exp)
        assert ps.outcome.shape == (csr[2].size, gid.size) and set(np.unique(ps.outcome).tolist()) == {0, 1, 2}
        assert len({tuple(c) for c in exp[2].T.tolist()}) > gid.size // 2       # the columns differ: their order is checked
        if name == "three_groups":
            assert exp[0][:, wc.group_of_size(name, 300)].max() > 255            # a count that needs its ninth bit
        if name == "mostly_padding":
            assert ps.n_gt.shape[1] == 17 and all(exp[0][:, g].max() > 0 for g in range(17))
        support_check(ctx, X, gid, csr, pkg, ties=False, outcomes=False, tag=name, exp=exp)
        monkeypatch.setenv("REO_PAIR_SUPPORT_BATCH", "50")                         # (read per call)
        again, _ = support_check(ctx, X, gid, csr, pkg, ties=True, outcomes=True, tag=(name, "batch 50"), exp=exp)
        assert again.outcome.tobytes() == ps.outcome.tobytes() and again.n_gt.tobytes() == ps.n_gt.tobytes()


# ---- d. the masked build (k_valid_words, k_counts_masked, k_pairs_masked; mp_threshold_table up to 331 jointly observed samples)

@pytest.mark.parametrize("name,k,kind", [("seam_in_group", 0, "int"), ("full_blocks", 0, "int"), ("three_groups", 1, "float")])
def test_masked_build_across_blocks(pkg, name, k, kind):
    """30 % missing at random plus the special genes: counts (whole and a rectangle off the origin) and the whole class table against the
    restatement, whose thresholds come from oracle.reo_numpy.threshold for every number of jointly observed samples; then the all-ones
    mask against the restatement and, byte for byte, against the plain build.  full_blocks: pairs tied in more than 64 jointly observed
    samples of a group (the second word of the coin stream); three_groups, k = 1: the t-side sums two groups"""
    Gt, seed = wc.G_TABLE, 0x5EED0D00 + k
    gid = wc.gid_of(name)
    ng = int(gid.max()) + 1
    X = wc.int_ties(name, Gt, wc.TABLE_SEED[name], k, pattern=False) if kind == "int" else wc.float_ties(name, Gt, wc.TABLE_SEED[name], k)
    V = wc.random_valid(name, Gt, 7)
    counts = mpc.masked_counts(X, V, gid, ng)
    upper = np.triu(np.ones((Gt, Gt), dtype=bool), 1)
    if name == "full_blocks":
        assert ((counts[1].max(axis=2) > 64) & upper).any()
    n1 = counts[2][:, :, k]
    n2 = counts[2].sum(axis=2) - n1
    assert max(int(n1[upper].max()), int(n2[upper].max())) > 100                 # thresholds well beyond 64 samples are read
    want = check_counts_and_codes(pkg, X, V, gid, seed, ks=(k,), tag=name)
    assert set(range(9)) <= set(np.unique(want).tolist())
    ones = np.ones(X.shape, dtype=bool)
    with open_masked(pkg, X, ones, gid, seed) as ctx:
        assert blocks(ctx, name)[0] >= 10
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(k)
        plain = ctx.get_codes(0, Gt, 0, Gt)
        used = ctx.build_pairs_masked(k, 0.01)
        assert ctx.info()["masked_build"] == 1
        full = ctx.get_codes(0, Gt, 0, Gt)
        assert np.array_equal(full, plain)
        full_counts = mpc.masked_counts(X, ones, gid, ng)
        if kind == "int" and name != "three_groups":
            assert ((full_counts[1].max(axis=2) > 64) & upper).any()             # more than 64 ties of a group: the second coin word
        assert np.array_equal(full, mpc.masked_codes(full_counts, k, 0.01, used, seed))
        assert not np.array_equal(full, want)


# ---- e. permuted tables (k_perm_words, k_pairs_permuted)

PERM_CASES = [("seam_in_group", wc.G_TABLE, "int"), ("full_blocks", wc.G_TABLE, "int"), ("three_groups", wc.G_TABLE, "float"),
              ("seam_in_group", 1100, "ranks")]


def perm_data(name, Gp, kind):
    if kind == "ranks":
        return wc.ranks(name, Gp, 0x5EED0E02)
    return wc.int_ties(name, Gp, wc.TABLE_SEED[name], 0, pattern=False) if kind == "int" else wc.float_ties(name, Gp, wc.TABLE_SEED[name], 0)


@pytest.mark.parametrize("name,Gp,kind", PERM_CASES)
def test_perm_codes_across_blocks(pkg, rel, name, Gp, kind):  # noqa: F811
    """two shuffled rows and the identity row, whole tables: against the relabelled two-group build (check_codes) and, for the tables
    with ties, against the numpy restatement, which holds the coins to the oracle's tie_wins directly; G = 1 100 is tie-free and is
    compared with the relabelled build alone"""
    seed, k = 0x5EED0E00, 0
    gid = wc.gid_of(name)
    X = perm_data(name, Gp, kind)
    rows = check_codes(pkg, rel, X, gid, seed, k=k, n_rows=2)
    obs = (gid == k).astype(np.uint8)
    assert not any(np.array_equal(r, obs) for r in rows)
    aw, live = pnc.pack_words(rows, gid, int(gid.max()) + 1)
    assert aw.shape[1] == wc.LAYOUTS[name][3] and ((aw != 0) & (aw != live[None, :])).all(axis=0).sum() >= aw.shape[1] - 2   # both sides in nearly every block
    with open_perm(pkg, X, gid, seed, build_k=k) as ctx:
        assert blocks(ctx, name)[0] >= 10
        thr = ctx.get_thresholds()
        if int(gid.max()) == 1:                                                  # the identity row of two groups: the resident table
            assert np.array_equal(ctx.perm_codes(obs, k=k), ctx.get_codes(0, Gp, 0, Gp))
        else:                                                                    # (three groups: the rest draws one coin per group there)
            assert np.array_equal(ctx.perm_codes(obs, k=k), rel(seed).codes(X, obs))
        if kind != "ranks":
            m = (int(thr[0, k]), int(thr[1, k]))
            for row in list(rows) + [obs]:
                got = ctx.perm_codes(row, k=k)
                want = pnc.permuted_codes(X, row, m, seed)
                assert np.array_equal(got, want), (name, int((got != want).sum()))
            if name == "full_blocks":
                n_eq = mpc.masked_counts(X, np.ones(X.shape, dtype=bool), (1 - rows[0]).astype(np.int32), 2)[1]
                assert (n_eq.max(axis=2) > 64).sum() > Gp + 100                  # (the diagonal aside) sides with more than 64 ties


@pytest.mark.parametrize("name,kind", [("seam_in_group", "int"), ("full_blocks", "int"), ("three_groups", "float")])
def test_permutation_null_across_blocks(pkg, rel, monkeypatch, name, kind):  # noqa: F811
    """five rows in batches of three (a short last batch): delta1_null, n_up, n_down and se_null bit for bit the relabelled context's pass,
    n_ge the numpy count.  seam_in_group: the last row is shuffled within strata of 16 columns, so that side A has samples in every block"""
    monkeypatch.setenv("REO_PERM_BATCH", "3")
    seed, k, Gp = 0x5EED0E10, 0, wc.G_TABLE
    gid = wc.gid_of(name)
    X = perm_data(name, Gp, kind)
    rows = pkg.permuted_labels(gid, k, 5, seed=4)
    if name == "seam_in_group":
        rows[4] = pkg.permuted_labels(gid, k, 1, seed=5, strata=np.arange(gid.size) // 16)[0]
        aw, live = pnc.pack_words(rows[4:], gid, 2)
        wide = np.array([bin(int(w)).count("1") >= 7 for w in live])             # (the last block of a group has 7 and 2 real slots)
        assert aw.shape[1] == 10 and wide.sum() == 9 and ((aw[0] != 0) & (aw[0] != live))[wide].all()   # both sides in every such block
    pn, info, called = check_null_against_relabelled(pkg, rel, X, gid, seed, k, rows, np.ones(Gp, dtype=bool))
    assert info["perm_batch"] == 3 and info["sample_slots"] == 32 * wc.LAYOUTS[name][3]
    assert len({d.tobytes() for d in pn.delta1_null}) == 5 and pn.n_ge.max() <= 5


# ---- f. contrasts (k1_classify_contrast on the shared count planes)

@pytest.fixture(scope="module")
def contrast_case(pkg, oracle):
    name, Gc, seed = "contrast_groups", wc.G_CONTRAST, 0x5EED0F00
    gid = wc.gid_of(name)
    sizes = wc.sizes_of(name)
    X = wc.planted_ties(name, Gc, wc.QUERY_SEED)
    thr = np.array([[oracle.threshold(int(n), 0.05) for n in sizes], [oracle.threshold(int(gid.size - n), 0.05) for n in sizes]])
    cache = {}
    codes, off = composed_rows(oracle, X, gid, 3, thr, seed, 0, Gc, ORDERED, cache)
    ref0 = np.zeros(Gc, dtype=bool)
    ref0[np.random.default_rng(9).choice(Gc, 120, replace=False)] = True
    return {"name": name, "gid": gid, "X": X, "thr": thr, "codes": codes, "off": off, "nre": cache[0, Gc][0], "ref0": ref0, "seed": seed}


def test_contrasts_every_ordered_contrast_with_counts_above_255(pkg, oracle, contrast_case):
    """groups of 300, 260 and 40 samples, tie-rich Int64: all six ordered contrasts against the composition from the C oracle's pair counts
    and coins, their tallies, and one identify_degs"""
    c, Gc = contrast_case, wc.G_CONTRAST
    name, gid = c["name"], c["gid"]
    big, mid = wc.group_of_size(name, 300), wc.group_of_size(name, 260)
    upper = np.triu(np.ones((Gc, Gc), dtype=bool), 1)
    both = (c["nre"][:, :, big] > 255) & (c["nre"][:, :, mid] > 255) & upper
    assert both.sum() > 100                                                      # the high byte of both counts that a contrast unpacks
    with pkg.Context(device=0, seed=c["seed"]) as ctx:
        ctx.set_matrix(c["X"]); ctx.set_groups(gid, 3)
        assert np.array_equal(ctx.compute_thresholds(0.05), c["thr"])
        for ctrl, treat in ORDERED:
            ctx.build_contrast(ctrl, treat)
            info = ctx.info()
            assert info["contrast_treat"] == treat and info["shared_group_counts"] == 1 and info["has_ties"] == 1
            assert info["sample_slots"] == 32 * 21
            code = c["codes"][ctrl, treat]
            got = ctx.get_codes(0, Gc, 0, Gc)
            assert np.array_equal(got[c["off"]], code[c["off"]]), (ctrl, treat, int((got != code)[c["off"]].sum()))
            assert len(np.unique(code[c["off"]])) >= 5, (ctrl, treat)
            full = np.where(c["off"], code, 255).astype(np.uint8)
            assert np.array_equal(ctx.tally(c["ref0"]), oracle.tally(full, c["ref0"])), (ctrl, treat)
        ctrl, treat = big, mid
        ctx.build_contrast(ctrl, treat)
        full = np.where(c["off"], c["codes"][ctrl, treat], 255).astype(np.uint8)
        assert set(np.unique(full[c["off"]]).tolist()) == set(range(9))
        res, iters, trace = oracle.iterate(full, c["ref0"], 1.0, 0.05, 8, 1)
        assert 1 <= trace[-1][0] <= Gc // 4, trace                               # DEGs at the end: the pass is not hollow
        r, it, tr = ctx.identify_degs(c["ref0"], 1.0, 0.05, 8, 1)
        assert it == iters and tr == trace, (tr, trace)
        _check_result(r, res)


def test_tie_free_contrasts_equal_the_two_group_run_on_the_columns(pkg, oracle):
    """every sample a permutation: the contrast of the 300- and the 260-sample group, both ways, is the two-group run on their columns"""
    name, Gc, seed = "contrast_groups", wc.G_CONTRAST, 0x5EED0F01
    gid = wc.gid_of(name)
    big, mid = wc.group_of_size(name, 300), wc.group_of_size(name, 260)
    X = wc.ranks(name, Gc, wc.QUERY_SEED, effect_group=big)
    off = ~np.eye(Gc, dtype=bool)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, 3); thr = ctx.compute_thresholds(0.05)
        for c, t in ((big, mid), (mid, big)):
            ctx.build_contrast(c, t)
            assert ctx.info()["has_ties"] == 0 and ctx.info()["sample_slots"] == 32 * 21
            got = ctx.get_codes(0, Gc, 0, Gc)
            sel, sub, k = _subset(gid, c, t)
            assert sel.size == 560
            m = [int(thr[0, c]), int(thr[0, t])]
            code = oracle.build_codes(np.asarray(X[:, sel], dtype=np.float64), sub, 2, k, m, seed)
            assert np.array_equal(got[off], code[off]), (c, t)
            assert len(np.unique(got[off])) >= 5
            with pkg.Context(device=0, seed=seed) as two:
                two.set_matrix(np.asfortranarray(X[:, sel])); two.set_groups(sub, 2)
                thr2 = two.compute_thresholds(0.05)
                assert [int(thr2[0, k]), int(thr2[1, k])] == m
                two.build_pairs(k)
                assert np.array_equal(two.get_codes(0, Gc, 0, Gc)[off], got[off]), (c, t)
