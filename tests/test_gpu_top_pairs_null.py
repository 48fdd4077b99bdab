"""The label-permutation null of the best pair score on the GPU (reo_top_pairs_null; csrc/toppairsnull.hip): per label row the largest |N|
over all gene pairs, the pair that attains it and the pairs that reach a few cuts, sixteen rows from one walk over the bit planes.  The
expected values come from the numpy restatement of the definition (tests/top_pairs_null_cases.py) and every comparison is exact.  The
shapes are those of the search's own tests: several column tiles and workgroups, a block seam inside both sides, a side of one sample, a
group on neither side (2-bytes, a live word with holes), data with ties (float300, whose values come closer than the tie band, and the
counts) and without (separated, the moved cases, the planted ranks), and all |N| equal."""
import numpy as np
import pytest

from query_cases import planted_ranks
import top_pairs_cases as tpc
import top_pairs_null_cases as tnc

pytestmark = pytest.mark.gpu


def open_case(pkg, name, seed=11):
    """matrix and groups of a named case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = tpc.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def same(got, exp, tag=None):
    """a TopPairsNull against a Null of the restatement, field by field"""
    assert got.max_num.dtype == np.int64 and got.arg_i.dtype == np.int32 and got.arg_j.dtype == np.int32 and got.n_reach.dtype == np.int64, tag
    assert np.array_equal(got.max_num, exp.max_num), (tag, got.max_num, exp.max_num)
    assert np.array_equal(got.arg_i, exp.arg_i) and np.array_equal(got.arg_j, exp.arg_j), (tag, got.arg_i, got.arg_j, exp.arg_i, exp.arg_j)
    assert got.n_reach.shape == exp.n_reach.shape and np.array_equal(got.n_reach, exp.n_reach), (tag, got.n_reach, exp.n_reach)


def identical(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("max_num", "arg_i", "arg_j", "n_reach", "cuts", "side_sizes")) \
        and (x.a, x.b) == (y.a, y.b)


@pytest.mark.parametrize("name", tnc.NAMES)
def test_every_row_equals_the_restatement(pkg, name):
    """B = 1, 16, 17 and 33 rows: less than a launch group, a full one, a partial second one and a third one; row 0 is the observed
    labelling, on which the maximum is that of the existing search on the same context"""
    exp, rows, cuts = tnc.expected(name), tnc.rows(name), tnc.cuts(name)
    X = tpc.case(name)[0]
    pairs = X.shape[0] * (X.shape[0] - 1) // 2
    ctx, a, b = open_case(pkg, name)
    with ctx:
        if name in ("separated", "count_i64", "count_f32"):                      # the tie-free form of the kernel, and the form with ties
            assert ctx.info()["has_ties"] == (0 if name == "separated" else 1)   # (float300 has values closer than the band: with ties)
        for B in (1, 16, 17, 33):
            got = ctx.top_pairs_null(rows[:B], a=a, b=b, cuts=cuts)
            same(got, tnc.first(exp, B), (name, B))
            assert (got.a, got.b) == (a, b) and np.array_equal(got.cuts, cuts)
            assert tuple(int(v) for v in got.side_sizes) == tpc.expected(name).sizes
            assert (got.n_reach[:, 0] == pairs).all() and not got.n_reach[:, 5].any()
            assert ctx.info()["top_pairs_null_batch"] == B and ctx.info()["top_pairs_null_us"] > 0
        assert got.max_num[0] == abs(int(ctx.top_pairs(1, a=a, b=b).num[0]))
        assert np.array_equal(got.max_score, exp.max_num / float(cuts[4]))
        if name == "level":                                                      # every |N| is 0: the first pair, and every pair reaches cut 0
            assert not got.max_num.any() and not got.arg_i.any() and (got.arg_j == 1).all() and (got.n_reach[:, 0] == 4950).all()
        bare = ctx.top_pairs_null(rows[:17], a=a, b=b)                           # no cuts: no counters
        assert bare.n_reach.shape == (17, 0) and bare.cuts.size == 0 and np.array_equal(bare.max_num, exp.max_num[:17])
        assert np.array_equal(bare.arg_i, exp.arg_i[:17]) and np.array_equal(bare.arg_j, exp.arg_j[:17])


@pytest.mark.parametrize("name", ["float300", "count_i64", "three_0_2"])
def test_the_outputs_do_not_depend_on_position_or_batch(pkg, monkeypatch, name):
    exp, rows, cuts = tnc.expected(name), tnc.rows(name), tnc.cuts(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        plain = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
        same(plain, exp, name)
        back = ctx.top_pairs_null(rows[::-1], a=a, b=b, cuts=cuts)               # a row's outputs do not depend on its place in the batch
        same(back, tnc.Null(exp.max_num[::-1], exp.arg_i[::-1], exp.arg_j[::-1], exp.n_reach[::-1]), (name, "reversed"))
        for batch in (1, 16, 20):                                                # the seam between launches: read per call
            monkeypatch.setenv("REO_TOP_NULL_BATCH", str(batch))
            got = ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts)
            assert identical(got, plain), (name, batch)
            assert ctx.info()["top_pairs_null_batch"] == batch
        monkeypatch.setenv("REO_TOP_NULL_BATCH", "500")                          # it can only lower the batch
        assert identical(ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts), plain) and ctx.info()["top_pairs_null_batch"] == 33
        monkeypatch.delenv("REO_TOP_NULL_BATCH")
        assert identical(ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts), plain) and ctx.info()["top_pairs_null_batch"] == 33


@pytest.mark.parametrize("G", [4095, 4096, 32767, 32768])
def test_the_12_15_and_16_plane_chains(pkg, G):
    """the kernel is compiled per number of position planes: 12 up to 4 095 genes, 15 up to 32 767, 16 above.  The first gene count of each
    and the last one before it, on a case whose expectation needs no G x G arrays (top_pairs_null_cases.moved_expected), under the
    observed labels, the inverted ones and one shuffle."""
    X, gid, genes = tpc.moved_case(G, 31 + G)
    rows = tnc.moved_rows(gid, G)
    want = [tnc.moved_expected(X, rows[p], genes) for p in range(3)]
    cuts = np.array([0, 1, want[0][0], want[0][0] + 1], dtype=np.int64)
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        got = ctx.top_pairs_null(rows, cuts=cuts)
        assert got.max_num[0] == abs(int(ctx.top_pairs(1).num[0]))
    assert [(int(m), int(i), int(j)) for m, i, j in zip(got.max_num, got.arg_i, got.arg_j)] == want
    assert (got.n_reach[:, 0] == G * (G - 1) // 2).all()                         # (more than 2^29 pairs at 32 768 genes: 64-bit counters)
    assert (got.n_reach[:, 1] <= 6 * (G - 1)).all() and (got.n_reach[:, 1] >= 1).all()   # only pairs with a moved gene have N != 0
    assert got.n_reach[0, 2] >= 1 and got.n_reach[0, 3] == 0


def test_gene_mask(pkg):
    name = "float300"
    X, gid, ng, a, b = tpc.case(name)
    G = X.shape[0]
    rows, cuts = tnc.rows(name)[:17], tnc.cuts(name)
    mask = tpc.half_mask(G)
    exp = tnc.restate(X, rows, cuts, mask)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        got = ctx.top_pairs_null(rows, a=a, b=b, gene_mask=mask, cuts=cuts)
        same(got, exp, "half of the genes")
        assert mask[got.arg_i].all() and mask[got.arg_j].all()
        m = int(mask.sum())
        assert (got.n_reach[:, 0] == m * (m - 1) // 2).all()
        assert not identical(got, ctx.top_pairs_null(rows, a=a, b=b, cuts=cuts))
        same(ctx.top_pairs_null(rows, a=a, b=b, gene_mask=np.ones(G, dtype=bool), cuts=cuts), tnc.first(tnc.expected(name), 17), "every gene")
        one = np.zeros(G, dtype=bool)
        one[G - 1] = True
        none = ctx.top_pairs_null(rows, a=a, b=b, gene_mask=one, cuts=cuts)
        assert (none.max_num == -1).all() and (none.arg_i == -1).all() and (none.arg_j == -1).all() and not none.n_reach.any()
        two = one.copy()
        two[3] = True
        pair = ctx.top_pairs_null(rows, a=a, b=b, gene_mask=two, cuts=cuts)
        same(pair, tnc.restate(X, rows, cuts, two), "two genes")
        assert (pair.arg_i == 3).all() and (pair.arg_j == G - 1).all() and (pair.n_reach[:, 0] == 1).all()
        bad = np.ones(G, dtype=np.uint8)
        bad[7] = 2
        with pytest.raises(pkg.DimensionMismatch, match=r"reo_top_pairs_null: gene_mask\[7\] = 2"):
            ctx.top_pairs_null(rows, a=a, b=b, gene_mask=bad)


def test_a_null_disturbs_nothing(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    rows = tnc.shuffled_rows(tnc.observed_row(gid, 0, None), 17, 5)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        first = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        codes, ref, info = ctx.get_codes(0, G, 0, G), ctx.ref_mask(), ctx.info()
        got = ctx.top_pairs_null(rows, cuts=[0, 50])                             # (tie-free data: the gene-order planes are made on demand)
        same(got, tnc.restate(X, rows, [0, 50]), "after a build")
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes) and np.array_equal(ctx.ref_mask(), ref)
        after = ctx.info()
        own = ("planes_on_demand", "top_pairs_null_batch", "top_pairs_null_us")  # (the planes it had made, and its own two entries)
        assert all(after[k] == info[k] for k in info if k not in own), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        assert after["top_pairs_null_batch"] == 17 and after["top_pairs_null_us"] > 0 and info["top_pairs_null_batch"] == 0
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == first[1:] and np.array_equal(again[0], first[0], equal_nan=True)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    X, gid, ng, a, b = tpc.case("three_0_2")
    G, S = X.shape
    rows = np.array(tnc.rows("three_0_2")[:3])
    ctx, _, _ = open_case(pkg, "three_0_2")
    with ctx:
        ok = dict(sides=rows, a=0, b=2)
        far = rows.copy(); far[1, 5] = 7
        part = rows.copy(); part[2, np.flatnonzero(rows[2] == 2)[0]] = 0
        gone = rows.copy(); gone[0, np.flatnonzero(rows[0] == 1)[0]] = 2
        more = rows.copy(); more[1, np.flatnonzero(rows[1] == 0)[0]] = 1
        for kw, pattern in ((dict(ok, b=0), "b == a == 0"), (dict(ok, a=3), "a = 3 is outside the groups \\[0, 3\\)"),
                            (dict(ok, b=3), "b = 3 is outside the groups"), (dict(ok, a=-1), "a = -1 is outside"),
                            (dict(ok, sides=rows[:0]), "n_perm = 0, between 1 and 2\\^20"),
                            (dict(ok, cuts=np.arange(9)), "n_cuts = 9, between 0 and 8"), (dict(ok, cuts=[3, -2]), "cuts\\[1\\] = -2, a cut of \\|N\\| is not negative"),
                            (dict(ok, sides=far), "row 1 of sides holds the byte 7 in column 5"),
                            (dict(ok, sides=part), "row 2 of sides holds the byte 0 in column \\d+, whose sample is on neither side"),
                            (dict(ok, sides=gone), "row 0 of sides holds the byte 2 in column \\d+, whose sample is on one of the sides"),
                            (dict(ok, sides=more), "row 1 of sides has 21 ones and 11 zeros, side A has 20 samples and side B 12"),
                            (dict(ok, b=None), "row 0 of sides holds the byte 2 in column \\d+, whose sample is on one of the sides")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                ctx.top_pairs_null(**kw)
            assert e.value.status == pkg._ffi.REO_EINVAL and "reo_top_pairs_null" in e.value.message
        with pytest.raises(pkg.DimensionMismatch, match="sides has shape"):
            ctx.top_pairs_null(rows[:, :-1], a=0, b=2)
        with pytest.raises(pkg.DimensionMismatch, match="gene_mask has shape"):
            ctx.top_pairs_null(rows, a=0, b=2, gene_mask=np.ones(G + 1, dtype=bool))
        # a refused call writes nothing, and only cuts / n_reach may be null, with n_cuts == 0
        P = pkg._ffi._ptr
        L, h = ctx._L, ctx._h
        mx, gi, gj = np.full(3, -7, dtype=np.int64), np.full(3, -7, dtype=np.int32), np.full(3, -7, dtype=np.int32)
        reach, cuts = np.full((3, 2), -7, dtype=np.int64), np.array([0, 5], dtype=np.int64)
        for args, pattern in (((2, 2, P(rows), 3, None, P(cuts), 2, P(mx), P(gi), P(gj), P(reach)), "b == a"),
                              ((0, 2, None, 3, None, P(cuts), 2, P(mx), P(gi), P(gj), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, None, P(cuts), 2, None, P(gi), P(gj), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, None, P(cuts), 2, P(mx), None, P(gj), P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, None, P(cuts), 2, P(mx), P(gi), None, P(reach)), "must not be null"),
                              ((0, 2, P(rows), 3, None, P(cuts), 2, P(mx), P(gi), P(gj), None), "nor cuts and n_reach with n_cuts = 2"),
                              ((0, 2, P(rows), 3, None, None, 2, P(mx), P(gi), P(gj), P(reach)), "nor cuts and n_reach with n_cuts = 2"),
                              ((0, 2, P(far), 3, None, P(cuts), 2, P(mx), P(gi), P(gj), P(reach)), "holds the byte 7"),
                              ((0, 2, P(rows), (1 << 20) + 1, None, P(cuts), 2, P(mx), P(gi), P(gj), P(reach)), "n_perm = 1048577"),
                              ((0, 2, P(rows), 3, None, P(cuts), -1, P(mx), P(gi), P(gj), P(reach)), "n_cuts = -1")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern):
                pkg._ffi.check(L.reo_top_pairs_null(h, *args))
        assert (mx == -7).all() and (gi == -7).all() and (gj == -7).all() and (reach == -7).all()
        exp = tnc.first(tnc.expected("three_0_2"), 3)
        pkg._ffi.check(L.reo_top_pairs_null(h, 0, 2, P(rows), 3, None, None, 0, P(mx), P(gi), P(gj), None))   # cuts and n_reach are optional
        assert np.array_equal(mx, exp.max_num) and np.array_equal(gi, exp.arg_i) and np.array_equal(gj, exp.arg_j) and (reach == -7).all()
        ctx.set_valid_mask(np.ones((G, S), dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_null compares on the bit planes of the whole matrix.*while a mask is set"):
            ctx.top_pairs_null(**ok)
        ctx.set_valid_mask(None)
        same(ctx.top_pairs_null(**ok), tnc.Null(exp.max_num, exp.arg_i, exp.arg_j, exp.n_reach[:, :0]), "mask cleared")
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_null is not available on a sharded context"):
            ctx.top_pairs_null(**ok)
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.top_pairs_null(np.zeros((1, 0), dtype=np.uint8))
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs_null is not available on a reo_create_multi context"):
            ctx.top_pairs_null(rows, a=0, b=2)


def test_run_identify_degs_carries_the_null(pkg):
    K, B = 20, 17
    today = {"k", "result", "labels", "iters_run", "trace"}
    # two groups: the dict's TopPairsNull equals a direct call with the rows of permuted_sides
    X, gid, ng, a, b = tpc.case("count_i64")
    G = X.shape[0]
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    plain = pkg.run_identify_degs(*args, seed=3, device=0)
    on = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=K, top_pairs_permutations=B, perm_seed=4)
    assert set(plain.comparisons[0]) == today and set(on.comparisons[0]) == today | {"top_pairs", "top_pairs_null"}
    assert set(pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=K).comparisons[0]) == today | {"top_pairs"}
    assert np.array_equal(on.result, plain.result, equal_nan=True) and on.trace == plain.trace
    tp, got = on.comparisons[0]["top_pairs"], on.comparisons[0]["top_pairs_null"]
    rows = pkg.permuted_sides(gid, 0, None, B, seed=4)
    cuts = np.abs(tp.num[[0, 9, 19]])
    ctx, _, _ = open_case(pkg, "count_i64")
    with ctx:
        direct = ctx.top_pairs_null(rows, cuts=cuts)
    assert identical(got, direct) and (got.a, got.b) == (0, None) and got.max_num.size == B
    same(got, tnc.restate(X, rows, cuts), "two groups")
    p = got.p_max(tp)
    assert p.shape == (K,) and (np.diff(p) >= 0).all() and p.min() >= 1.0 / (1 + B) and p.max() <= 1.0
    # three groups, one contrast: the samples of group 1 take no part; strata are honoured
    X, gid, ng, _, _ = tpc.case("three_0_2")
    G = X.shape[0]
    strata = np.arange(gid.size) % 2
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    plain = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)])
    run = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)], top_pairs=K, top_pairs_permutations=B, perm_seed=9, perm_strata=strata)
    assert np.array_equal(run.result, plain.result, equal_nan=True) and run.trace == plain.trace
    tp, got = run.comparisons[0]["top_pairs"], run.comparisons[0]["top_pairs_null"]
    rows = pkg.permuted_sides(gid, 0, 2, B, seed=9, strata=strata)
    assert len(run.comparisons) == 1 and (got.a, got.b) == (0, 2) and (rows[:, gid == 1] == 2).all()
    same(got, tnc.restate(X, rows, np.abs(tp.num[[0, 9, 19]])), "contrast (0, 2)")
    # the reference's comparisons of three groups: group k against every other sample, seed perm_seed + k
    run = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=K, top_pairs_permutations=2, perm_seed=9)
    assert [(cm["top_pairs_null"].a, cm["top_pairs_null"].b) for cm in run.comparisons] == [(0, None), (1, None), (2, None)]
    same(run.comparisons[1]["top_pairs_null"],
         tnc.restate(X, pkg.permuted_sides(gid, 1, None, 2, seed=10), np.abs(run.comparisons[1]["top_pairs"].num[[0, 9, 19]])), "group 1 against the rest")


def test_reoa_writes_a_top_pairs_null_file(pkg, tmp_path):
    (tmp_path / "on").mkdir(); (tmp_path / "off").mkdir()
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "on"), seed=0x5EED0001, device=0, top_pairs=30, top_pairs_permutations=16)
    pkg.reoa(use_testdata="yes", work_dir=str(tmp_path / "off"), seed=0x5EED0001, device=0, top_pairs=30)
    run = df.attrs["run"]
    tp, null = run.comparisons[0]["top_pairs"], run.comparisons[0]["top_pairs_null"]
    assert null.max_num.size == 16 and null.cuts.tolist() == np.abs(tp.num[[0, 9, 29]]).tolist()
    lines = (tmp_path / "on" / "fn_expr_group1_group2_top_pairs_null.tsv").read_text().split("\n")
    assert lines[0].split("\t") == ["gene_i", "gene_j", "direction", "score", "rank_score", "gt_A", "eq_A", "gt_B", "eq_B", "p_max"]
    assert lines[-1] == "" and len(lines) == 32
    p = np.array([float(l.split("\t")[9]) for l in lines[1:-1]])
    assert np.array_equal(p, null.p_max(tp)) and (np.diff(p) >= 0).all() and p.min() >= 1.0 / 17
    pairs = (tmp_path / "on" / "fn_expr_group1_group2_top_pairs.tsv").read_bytes()
    assert pairs == (tmp_path / "off" / "fn_expr_group1_group2_top_pairs.tsv").read_bytes()
    assert [l.split("\t")[:9] for l in lines[:-1]] == [l.split("\t") for l in pairs.decode().split("\n")[:-1]]
    assert not (tmp_path / "off" / "fn_expr_group1_group2_top_pairs_null.tsv").exists()
