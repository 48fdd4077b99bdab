"""The top partners of a gene on the GPU (reo_top_partners; csrc/toppartners.hip): per query gene its best m partner genes, the counts of
"query above partner", N and Gamma.  The expected rows come from the two numpy restatements of tests/top_partners_cases.py -- from_pairs,
the subsequence of the search's oracle, and row_oracle, straight from the values -- and every comparison is exact, field by field; there is
no tolerance anywhere.  The shapes are the smallest at which the kernels can still go wrong: several column tiles and row tiles, a last row
tile that is partly empty, a batch seam, 12 / 15 / 16 position planes with a tile's last column and the last gene, a block seam inside a
group, and a side of 32 768 samples, whose counts set bit 15 of the 16-bit cell."""
import importlib
import os

import numpy as np
import pytest

from query_cases import planted_ranks
import top_pairs_cases as tpc
import top_partners_cases as tprc
import wide_top_pairs_cases as wt

pytestmark = pytest.mark.gpu

FIELDS = ("genes", "partner", "n_gt", "n_eq", "num", "rank_num", "n_found", "side_sizes")


def open_case(pkg, name, cases=tpc, seed=11):
    """matrix and groups of a named case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = cases.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def identical(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in FIELDS) and (x.a, x.b) == (y.a, y.b)


@pytest.mark.parametrize("name", tpc.EQUALITY)
def test_every_row_equals_the_oracle(pkg, name):
    """all genes, m = G - 1: every row whole"""
    exp = tpc.expected(name)
    G = exp.D.size
    full = 2 * exp.sizes[0] * exp.sizes[1]
    if name == "separated":                                                      # asserted from the oracle: Gamma alone orders thousands
        assert (np.abs(exp.num) == full).sum() == 8400
    if name == "level":                                                          # every key is (0, 0): the index alone orders
        assert not exp.num.any() and not exp.rank_num.any()
    ctx, a, b = open_case(pkg, name)
    with ctx:
        tp = ctx.top_partners(m=G - 1, a=a, b=b)
    rows = [tprc.from_pairs(exp, q) for q in range(G)]
    tprc.check_table(tp, rows, G - 1)
    assert np.array_equal(tp.genes, np.arange(G, dtype=np.int32)) and (tp.n_found == G - 1).all()
    assert (tp.a, tp.b) == (a, b) and tuple(int(v) for v in tp.side_sizes) == exp.sizes
    assert np.array_equal(tp.score, np.abs(tp.num) / float(full)) and np.array_equal(tp.direction, np.sign(tp.num).astype(np.int8))
    if name == "level":
        assert all(tp.partner[q].tolist() == [p for p in range(G) if p != q] for q in (0, 50, G - 1))
    # N is antisymmetric and the row of the other gene holds the other orientation
    q, p = 3, int(tp.partner[3, 0])
    at = int(np.flatnonzero(tp.partner[p] == q)[0])
    assert tp.num[p, at] == -tp.num[q, 0] and tp.rank_num[p, at] == tp.rank_num[q, 0]
    assert np.array_equal(tp.n_gt[p, at], np.asarray(exp.sizes) - tp.n_gt[q, 0] - tp.n_eq[q, 0]) and np.array_equal(tp.n_eq[p, at], tp.n_eq[q, 0])


def test_the_library_s_own_search_filtered_per_gene(pkg):
    """float300: top_pairs(all 44 850 pairs) filtered per gene equals top_partners(m = 299); pairs() of all genes at m = 1 starts with
    top_pairs(1)'s pair"""
    name = "float300"
    ctx, a, b = open_case(pkg, name)
    with ctx:
        G = ctx.G
        every = ctx.top_pairs(G * (G - 1) // 2, a=a, b=b)
        assert every.gene_i.size == 44850
        tp = ctx.top_partners(m=G - 1, a=a, b=b)
        best = ctx.top_partners(a=a, b=b)
        one = ctx.top_pairs(1, a=a, b=b)
    listed = tpc.Oracle(every.gene_i, every.gene_j, np.stack([every.n_gt[:, 0], every.n_eq[:, 0], every.n_gt[:, 1], every.n_eq[:, 1]], axis=1),
                        every.num, every.rank_num, None, tuple(int(v) for v in every.side_sizes), None)
    tprc.check_table(tp, [tprc.from_pairs(listed, q) for q in range(G)], G - 1)
    assert best.partner.shape == (G, 1) and np.array_equal(best.partner[:, 0], tp.partner[:, 0]) and np.array_equal(best.num[:, 0], tp.num[:, 0])
    bp, bs = best.best()
    assert np.array_equal(bp, tp.partner[:, 0]) and np.array_equal(bs, tp.score[:, 0])
    pairs = best.pairs()
    assert (pairs.gene_i[0], pairs.gene_j[0]) == (one.gene_i[0], one.gene_j[0]) and pairs.num[0] == one.num[0] and pairs.rank_num[0] == one.rank_num[0]
    assert np.array_equal(pairs.n_gt[0], one.n_gt[0]) and np.array_equal(pairs.n_eq[0], one.n_eq[0]) and (pairs.gene_i < pairs.gene_j).all()
    whole = tp.pairs()                                                           # every pair listed from both its genes: the search's list itself
    assert all(np.array_equal(getattr(whole, f), getattr(every, f)) for f in ("gene_i", "gene_j", "n_gt", "n_eq", "num", "rank_num"))


def test_mask_rows_and_padding(pkg):
    name = "float300"
    X, gid, ng, a, b = tpc.case(name)
    exp = tpc.expected(name)
    G = X.shape[0]
    mask = tpc.half_mask(G)
    inside, outside = np.flatnonzero(mask)[:3], np.flatnonzero(~mask)[:3]
    ctx, a, b = open_case(pkg, name)
    with ctx:
        # query genes inside and outside the mask; repeated and unsorted: independent rows; 9 rows: the last row tile is partly empty
        genes = np.array([inside[2], outside[0], inside[0], outside[2], inside[2], 299, 0, outside[0], inside[1]], dtype=np.int32)
        tp = ctx.top_partners(genes, 7, a=a, b=b, partner_mask=mask)
        tprc.check_table(tp, [tprc.from_pairs(exp, int(q), mask) for q in genes], 7)
        assert mask[tp.partner].all() and (tp.partner != genes[:, None]).all() and np.array_equal(tp.genes, genes)
        assert np.array_equal(tp.partner[0], tp.partner[4]) and np.array_equal(tp.partner[1], tp.partner[7])
        direct = tprc.row_oracle(X, gid, ng, a, b, exp.D, int(genes[1]), mask)   # (D over all genes, whatever the mask)
        assert np.array_equal(tp.partner[1], direct.partner[:7]) and np.array_equal(tp.rank_num[1], direct.rank_num[:7])
        one = ctx.top_partners([int(genes[0])], 7, a=a, b=b, partner_mask=mask)  # n_genes = 1
        assert one.partner.shape == (1, 7) and np.array_equal(one.partner[0], tp.partner[0]) and np.array_equal(one.num[0], tp.num[0])
        # m larger than the eligible partners: three partners, one of them the query itself in row 0
        few = np.zeros(G, dtype=bool)
        few[[5, 17, 250]] = True
        tp = ctx.top_partners([5, 6], 4, a=a, b=b, partner_mask=few)
        tprc.check_table(tp, [tprc.from_pairs(exp, 5, few), tprc.from_pairs(exp, 6, few)], 4)
        assert tp.n_found.tolist() == [2, 3] and tp.partner[0, 2:].tolist() == [-1, -1] and tp.partner[1, 3] == -1
        assert not tp.num[0, 2:].any() and not tp.n_gt[0, 2:].any() and not tp.n_eq[0, 2:].any() and not tp.rank_num[0, 2:].any()
        assert tp.csr()[1].tolist() == [0, 2, 5] and tp.csr()[2].tolist() == tp.partner[0, :2].tolist() + tp.partner[1, :3].tolist()
        # a mask that leaves a row no partner
        only = np.zeros(G, dtype=bool)
        only[9] = True
        tp = ctx.top_partners([9, 10, 9], 2, a=a, b=b, partner_mask=only)
        assert tp.n_found.tolist() == [0, 1, 0] and tp.partner.tolist() == [[-1, -1], [9, -1], [-1, -1]]
        assert not tp.num[[0, 2]].any() and not tp.n_gt[[0, 2]].any() and not tp.rank_num[[0, 2]].any()
        assert tp.best()[0].tolist() == [-1, 9, -1] and tp.best()[1][0] == 0.0
        none = ctx.top_partners([4], 3, a=a, b=b, partner_mask=np.zeros(G, dtype=bool))
        assert none.n_found.tolist() == [0] and none.partner.tolist() == [[-1, -1, -1]] and none.pairs().gene_i.size == 0
        with pytest.raises(pkg.DimensionMismatch, match="partner_mask has shape"):
            ctx.top_partners([4], 3, partner_mask=np.ones(G + 1, dtype=bool))


def test_the_batch_seam(pkg, monkeypatch):
    """REO_TOP_PARTNERS_BATCH=8 against the default on 20 query rows: three batches, the last of them half empty, the same arrays"""
    name = "count_i64"
    exp = tpc.expected(name)
    G = exp.D.size
    genes = np.random.default_rng(3).permutation(G)[:20].astype(np.int32)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        whole = ctx.top_partners(genes, 12, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PARTNERS_BATCH", "8")                        # (read per call)
        split = ctx.top_partners(genes, 12, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PARTNERS_BATCH", "13")                       # padded to 16: a seam inside the second tile pair
        odd = ctx.top_partners(genes, 12, a=a, b=b)
        monkeypatch.delenv("REO_TOP_PARTNERS_BATCH")
    tprc.check_table(whole, [tprc.from_pairs(exp, int(q)) for q in genes], 12)
    assert identical(whole, split) and identical(whole, odd)


@pytest.mark.parametrize("G", [4095, 4096, 32768, 65535])
def test_the_12_15_and_16_plane_chains(pkg, G):
    """the count kernel is compiled per number of position planes.  The moved genes (a tile's last column and the last gene among them)
    and genes 0, 63, 64 and G - 1 as queries, against rows straight from the values with the exact D of the moved case"""
    X, gid, moved = tpc.moved_case(G, 31 + G)
    D = tpc.moved_oracle(X, gid, moved, 8)[5]
    genes = np.unique(np.concatenate([moved, [0, 63, 64, G - 1]])).astype(np.int32)
    assert 63 in moved and G - 1 in moved
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        tp = ctx.top_partners(genes, 8)
    rows = [tprc.row_oracle(X, gid, 2, 0, None, D, int(q)) for q in genes]
    tprc.check_table(tp, rows, 8)
    assert (tp.n_found == 8).all() and not tp.n_eq.any()
    fixed = int(np.flatnonzero(genes == 64)[0])                                  # a fixed gene meets the six moved ones first, then N = 0
    assert set(tp.partner[fixed, :6].tolist()) == set(moved.tolist()) and not tp.num[fixed, 6:].any()


@pytest.mark.parametrize("name", ["seam", "limit"])
def test_wide_sample_axes_and_the_unsigned_cell(pkg, name):
    """seam: a block seam inside a group, five blocks a side.  limit: S_A = 32 768, so the separated genes' counts have bit 15 set -- a
    signed 16-bit cell would read them as negative"""
    X, gid, ng, a, b = wt.case(name)
    exp = wt.expected(name)
    G = X.shape[0]
    genes = np.array([0, 1, 7, G // 2, G - 1], dtype=np.int32)
    ctx, a, b = open_case(pkg, name, cases=wt)
    with ctx:
        assert ctx.info()["sample_slots"] // 32 == wt.blocks(name)
        tp = ctx.top_partners(genes, 6, a=a, b=b)
    tprc.check_table(tp, [tprc.row_oracle(X, gid, ng, a, b, exp.D, int(q)) for q in genes], 6)
    if name == "limit":
        assert exp.sizes == (32768, 32767) and tp.n_gt.max() == 32768 and (tp.n_gt >= 0).all()   # gene G - 1 above a separated gene in all of A
        assert np.abs(tp.num).max() == 2 * 32768 * 32767
    else:
        assert tp.n_eq.any() and min(exp.sizes) > 128


def test_a_call_disturbs_nothing(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    o = tpc.oracle(X, gid, len(lev), 0, None)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        first = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        ctx.top_pairs(50)                                                        # (tie-free data: makes the gene-order planes, and sets its own timers)
        codes, ref, info = ctx.get_codes(0, G, 0, G), ctx.ref_mask(), ctx.info()
        got = ctx.top_partners([0, 299, 17], 5)
        tprc.check_table(got, [tprc.from_pairs(o, q) for q in (0, 299, 17)], 5)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes) and np.array_equal(ctx.ref_mask(), ref)
        after = ctx.info()
        own = ("top_partners_count_us", "top_partners_select_us")                # (its own two timers and nothing else)
        assert all(after[k] == info[k] for k in info if k not in own), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        assert after["top_partners_count_us"] > 0 and after["top_partners_select_us"] > 0
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == first[1:] and np.array_equal(again[0], first[0], equal_nan=True)


def test_every_refusal_has_its_message_and_writes_nothing(pkg, monkeypatch):
    X, gid, ng, a, b = tpc.case("three_0_2")
    G, S = X.shape
    ctx, _, _ = open_case(pkg, "three_0_2")
    with ctx:
        for kw, pattern in ((dict(m=0), "m_want = 0, between 1 and 1024"), (dict(m=1025), "m_want = 1025, between 1 and 1024"),
                            (dict(a=0, b=0), "b == a == 0"), (dict(a=3), "a = 3 is outside the groups \\[0, 3\\)"),
                            (dict(a=0, b=3), "b = 3 is outside the groups"), (dict(genes=[]), "n_genes = 0, between 1 and 2\\^20"),
                            (dict(genes=[0, 5, G]), f"genes\\[2\\] = {G} is outside the genes \\[0, {G}\\) \\(row 2"),
                            (dict(genes=[-1]), "genes\\[0\\] = -1 is outside the genes"),
                            (dict(genes=np.zeros((1 << 16) + 1, dtype=np.int32), m=1024), "n_genes \\* m_want = 65537 x 1024, at most 2\\^26"),
                            (dict(genes=np.zeros((1 << 20) + 1, dtype=np.int32)), "n_genes = 1048577"),
                            (dict(partner_mask=np.full(G, 2, dtype=np.uint8)), "partner_mask\\[0\\] = 2, a byte of the mask is 0 or 1")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                ctx.top_partners(**kw)
            assert e.value.status == pkg._ffi.REO_EINVAL and "reo_top_partners" in e.value.message
        # a refused call writes nothing
        P = pkg._ffi._ptr
        genes = np.array([4, 2], dtype=np.int32)
        partner, counts = np.full((2, 3), -7, dtype=np.int32), np.full((2, 3, 4), -7, dtype=np.int32)
        key, found = np.full((2, 3, 2), -7, dtype=np.int64), np.full(2, -7, dtype=np.int32)
        bad_mask = np.ones(G, dtype=np.uint8)
        bad_mask[G - 1] = 3
        bad_genes = np.array([4, G], dtype=np.int32)
        call = ctx._L.reo_top_partners
        for args, pattern in (((2, 2, P(genes), 2, None, 3, P(partner), P(counts), P(key), P(found)), "b == a"),
                              ((0, 2, P(genes), 2, None, 1025, P(partner), P(counts), P(key), P(found)), "m_want = 1025"),
                              ((0, 2, P(genes), 0, None, 3, P(partner), P(counts), P(key), P(found)), "n_genes = 0"),
                              ((0, 2, None, 2, None, 3, P(partner), P(counts), P(key), P(found)), "must not be null"),
                              ((0, 2, P(genes), 2, None, 3, P(partner), P(counts), None, P(found)), "must not be null"),
                              ((0, 2, P(genes), 2, None, 3, P(partner), P(counts), P(key), None), "must not be null"),
                              ((0, 2, P(bad_genes), 2, None, 3, P(partner), P(counts), P(key), P(found)), "row 1 of the answer"),
                              ((0, 2, P(genes), 2, P(bad_mask), 3, P(partner), P(counts), P(key), P(found)), f"partner_mask\\[{G - 1}\\] = 3")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern):
                pkg._ffi.check(call(ctx._h, *args))
        assert all((x == -7).all() for x in (partner, counts, key, found))
        pkg._ffi.check(call(ctx._h, 0, 2, P(genes), 2, None, 3, P(partner), P(counts), P(key), P(found)))
        exp = tpc.expected("three_0_2")
        want = tprc.table([tprc.from_pairs(exp, 4), tprc.from_pairs(exp, 2)], 3)
        assert np.array_equal(partner, want[0]) and np.array_equal(counts, want[1]) and np.array_equal(key[:, :, 0], want[2])
        assert np.array_equal(key[:, :, 1], want[3]) and np.array_equal(found, want[4])
        ctx.set_valid_mask(np.ones((G, S), dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners compares on the bit planes of the whole matrix.*while a mask is set"):
            ctx.top_partners([4], 3)
        ctx.set_valid_mask(None)
        assert identical(ctx.top_partners([4, 2], 3, a=0, b=2), pkg.TopPartners(genes, want[0], want[1][:, :, 0::2], want[1][:, :, 1::2], want[2], want[3],
                                                                                 want[4], np.asarray(exp.sizes, dtype=np.int64), 0, 2))
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners is not available on a sharded context"):
            ctx.top_partners([4], 3)
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.top_partners([0], 3)
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="no groups"):
            ctx.top_partners([0], 3)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_partners is not available on a reo_create_multi context"):
            ctx.top_partners([0], 3)


def test_run_identify_degs_carries_the_partners_of_the_degs(pkg, tmp_path):
    """the bundled small case: top_partners=3 attaches the TopPartners of the comparison's DEGs against all genes; it equals a direct call,
    and write_extras writes <stem>_<fg_name>_top_partners.tsv, one line per DEG and partner"""
    seed = 0x5EED0001
    R = importlib.import_module(pkg.__name__ + ".reoa")
    golden = os.path.join(os.path.dirname(__file__), "golden")
    prep = R.prepare(os.path.join(golden, "fn_expr.txt"), os.path.join(golden, "fn_meta.txt"), seed=seed)
    args = (prep["data"], prep["sample_groups"], prep["gene_names"], 0.01, 1.0, 0.05, prep["ref"], 128, 5)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    on = pkg.run_identify_degs(*args, seed=seed, device=0, top_partners=3)
    assert set(on.comparisons[0]) == set(plain.comparisons[0]) | {"top_partners"} and "top_partners" not in plain.comparisons[0]
    assert np.array_equal(on.result, plain.result, equal_nan=True) and on.trace == plain.trace
    tp = on.comparisons[0]["top_partners"]
    degs = np.flatnonzero(on.labels != "no change").astype(np.int32)
    assert degs.size > 0 and np.array_equal(tp.genes, degs) and tp.partner.shape == (degs.size, 3) and (tp.n_found == 3).all()
    assert (tp.a, tp.b) == (0, None)
    gid, lev = pkg.encode_groups(prep["sample_groups"])
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev))
        ctx.set_matrix(np.asarray(prep["data"]))
        direct = ctx.top_partners(degs, 3)
        q = int(degs[0])
        D = ctx.rank_shift()
        info = ctx.info()
        none = pkg.hotpath.deg_top_partners(ctx, np.full(len(prep["gene_names"]), "no change", dtype=object), 0, None, 3)["top_partners"]
        assert ctx.info() == info                                                # a comparison without DEGs: an empty object, no library call
    assert identical(tp, direct)
    row = tprc.row_oracle(np.asarray(prep["data"]), gid, len(lev), 0, None, D, q)   # (D is held to its oracle in tests/test_gpu_top_pairs.py)
    assert np.array_equal(tp.partner[0], row.partner[:3]) and np.array_equal(tp.num[0], row.num[:3]) and np.array_equal(tp.n_gt[0], row.counts[:3, 0::2])
    out = R.write_extras("fn_expr", prep, on, str(tmp_path))
    assert [os.path.basename(p) for p in out] == ["fn_expr_group1_group2_top_partners.tsv"]
    lines = open(out[0]).read().split("\n")
    assert lines[0].split("\t") == ["gene", "rank", "partner", "num", "score", "rank_num", "gt_A", "eq_A", "gt_B", "eq_B"] and lines[-1] == ""
    assert len(lines) == 3 * degs.size + 2
    assert lines[1].split("\t")[:4] == [prep["gene_names"][q], "1", prep["gene_names"][int(tp.partner[0, 0])], str(int(tp.num[0, 0]))]
    assert none.genes.size == 0 and none.partner.shape == (0, 3) and none.n_gt.shape == (0, 3, 2) and none.pairs().gene_i.size == 0
    assert none.csr()[1].tolist() == [0] and tuple(int(v) for v in none.side_sizes) == tuple(int(v) for v in tp.side_sizes)
    assert (none.a, none.b) == (0, None) and none.best()[0].size == 0
