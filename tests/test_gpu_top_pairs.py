"""The top-scoring-pair search on the GPU (reo_top_pairs, reo_rank_shift; csrc/toppairs.hip): the n best of all gene pairs, selected on the
device by a radix select that recounts the pairs in every pass.  The expected values come from the numpy restatement of the definition
(tests/top_pairs_cases.py) and every comparison is exact: gene_i, gene_j, the four counts, N and Gamma.  The shapes are the smallest at which
the kernels can still go wrong: several column tiles and workgroups, a block seam inside both sides, a side of one sample, a group that
belongs to neither side, thousands of equal |N|, and all keys equal."""
import numpy as np
import pytest

from query_cases import planted_ranks
import top_pairs_cases as tpc

pytestmark = pytest.mark.gpu

N = 50


def open_case(pkg, name, seed=11):
    """matrix and groups of a named case, nothing else: no thresholds, no class table"""
    X, gid, ng, a, b = tpc.case(name)
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, ng)
    ctx.set_matrix(X)
    return ctx, a, b


def same(tp, exp, n, tag=None):
    """the first n pairs of the oracle, field by field"""
    k = min(n, exp.gene_i.size)
    assert tp.gene_i.dtype == np.int32 and tp.gene_j.dtype == np.int32 and tp.gene_i.size == k, tag
    assert np.array_equal(tp.gene_i, exp.gene_i[:k]) and np.array_equal(tp.gene_j, exp.gene_j[:k]), tag
    assert tp.n_gt.dtype == np.int32 and tp.n_gt.shape == (k, 2) and np.array_equal(tp.n_gt, exp.counts[:k, 0::2]), tag
    assert tp.n_eq.dtype == np.int32 and np.array_equal(tp.n_eq, exp.counts[:k, 1::2]), tag
    assert tp.num.dtype == np.int64 and np.array_equal(tp.num, exp.num[:k]), tag
    assert tp.rank_num.dtype == np.int64 and np.array_equal(tp.rank_num, exp.rank_num[:k]), tag
    assert tuple(int(v) for v in tp.side_sizes) == exp.sizes, tag
    assert (tp.gene_i < tp.gene_j).all(), tag


def identical(x, y):
    return all(np.array_equal(getattr(x, f), getattr(y, f)) for f in ("gene_i", "gene_j", "n_gt", "n_eq", "num", "rank_num", "side_sizes")) \
        and (x.a, x.b) == (y.a, y.b)


@pytest.mark.parametrize("name", tpc.EQUALITY)
def test_the_first_pairs_equal_the_oracle(pkg, name):
    exp = tpc.expected(name)
    full = 2 * exp.sizes[0] * exp.sizes[1]
    if name == "separated":                                                      # asserted from the oracle: Gamma decides, and decides at the cut
        assert (np.abs(exp.num) == full).sum() >= N and exp.rank_num[N - 1] != exp.rank_num[N]
    ctx, a, b = open_case(pkg, name)
    with ctx:
        tp = ctx.top_pairs(N, a=a, b=b)
        same(tp, exp, N, name)
        assert (tp.a, tp.b) == (a, b) and tp.passes >= 1
        assert np.array_equal(tp.direction, np.sign(exp.num[:N]).astype(np.int8))
        assert np.array_equal(tp.score, np.abs(exp.num[:N]) / float(full))
        if name == "level":                                                      # all 4 950 keys are (0, 0): the first pairs in (i, j) order, and all of them
            every = ctx.top_pairs(5000, a=a, b=b)
            assert every.gene_i.size == 4950
            same(every, exp, 5000, "level, every pair")
        if name == "float300":                                                   # a longer list crosses many equal |N|
            same(ctx.top_pairs(3000, a=a, b=b), exp, 3000, "float300, n = 3000")


@pytest.mark.parametrize("name", tpc.EQUALITY)
def test_rank_shift_equals_the_oracle(pkg, name):
    exp = tpc.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        D = ctx.rank_shift(a=a, b=b)
        assert D.dtype == np.int64 and D.shape == exp.D.shape and np.array_equal(D, exp.D), name


@pytest.mark.parametrize("G", [4095, 4096, 32767, 32768])
def test_the_15_and_16_plane_chains(pkg, monkeypatch, G):
    """the pair kernel is compiled per number of position planes: 12 up to 4 095 genes, 15 up to 32 767, 16 above.  The first gene count of
    each and the last one before it, on a case whose oracle needs no G x G arrays (top_pairs_cases.moved_case)."""
    X, gid, genes = tpc.moved_case(G, 31 + G)
    gi, gj, counts, num, gam, D = tpc.moved_oracle(X, gid, genes, N)
    with pkg.Context(device=0, seed=11) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        assert np.array_equal(ctx.rank_shift(), D)
        tp = ctx.top_pairs(N)
        monkeypatch.setenv("REO_TOP_PAIRS_CAP", str(N))
        tight = ctx.top_pairs(N)
    assert np.array_equal(tp.gene_i, gi) and np.array_equal(tp.gene_j, gj)
    assert np.array_equal(tp.n_gt, counts[:, 0::2]) and not tp.n_eq.any()
    assert np.array_equal(tp.num, num) and np.array_equal(tp.rank_num, gam)
    assert identical(tp, tight) and tight.passes >= tp.passes


@pytest.mark.parametrize("name", ["separated", "level"])
def test_the_result_does_not_depend_on_the_capacity(pkg, monkeypatch, name):
    exp = tpc.expected(name)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        wide = ctx.top_pairs(N, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PAIRS_CAP", str(N))                           # (read per call)
        tight = ctx.top_pairs(N, a=a, b=b)
        monkeypatch.setenv("REO_TOP_PAIRS_CAP", "3")                              # never below n
        floor = ctx.top_pairs(N, a=a, b=b)
        monkeypatch.delenv("REO_TOP_PAIRS_CAP")
    same(tight, exp, N, name)
    assert identical(wide, tight) and identical(floor, tight)
    assert tight.passes > wide.passes and floor.passes == tight.passes


def test_gene_mask(pkg):
    name = "float300"
    X, gid, ng, a, b = tpc.case(name)
    mask = tpc.half_mask(X.shape[0])
    assert 100 < mask.sum() < 200
    exp = tpc.oracle(X, gid, ng, a, b, mask)
    ctx, a, b = open_case(pkg, name)
    with ctx:
        tp = ctx.top_pairs(N, a=a, b=b, gene_mask=mask)
        same(tp, exp, N, "half of the genes")
        assert mask[tp.gene_i].all() and mask[tp.gene_j].all()
        assert not identical(tp, ctx.top_pairs(N, a=a, b=b))
        same(ctx.top_pairs(N, a=a, b=b, gene_mask=np.ones(X.shape[0], dtype=bool)), tpc.expected(name), N, "every gene")
        one = np.zeros(X.shape[0], dtype=bool)
        one[X.shape[0] - 1] = True
        none = ctx.top_pairs(N, a=a, b=b, gene_mask=one)
        assert none.gene_i.size == 0 and none.num.size == 0 and none.n_gt.shape == (0, 2)
        two = one.copy()
        two[3] = True
        pair = ctx.top_pairs(N, a=a, b=b, gene_mask=two)
        assert pair.gene_i.tolist() == [3] and pair.gene_j.tolist() == [X.shape[0] - 1]
        bad = np.ones(X.shape[0], dtype=np.uint8)
        bad[7] = 2
        with pytest.raises(pkg.DimensionMismatch, match=r"gene_mask\[7\] = 2"):
            ctx.top_pairs(N, a=a, b=b, gene_mask=bad)


@pytest.mark.parametrize("name", ["count_i64", "three_0_2", "three_1_rest"])
def test_pair_support_counts_the_listed_pairs_alike(pkg, name):
    ctx, a, b = open_case(pkg, name)
    with ctx:
        tp = ctx.top_pairs(N, a=a, b=b)
        ps = ctx.pair_support(tp.csr(), outcomes=True)
        rest = [g for g in range(ps.n_gt.shape[1]) if g != a] if b is None else [b]
        assert np.array_equal(ps.n_gt[:, a], tp.n_gt[:, 0]) and np.array_equal(ps.n_eq[:, a], tp.n_eq[:, 0])
        assert np.array_equal(ps.n_gt[:, rest].sum(axis=1), tp.n_gt[:, 1]) and np.array_equal(ps.n_eq[:, rest].sum(axis=1), tp.n_eq[:, 1])
        votes = tp.votes(ps)
        assert votes.shape == (ctx.S,) and votes.dtype == np.int32
        k = tp.disjoint(5)
        assert k.size == 5 and len(set(tp.gene_i[k].tolist()) | set(tp.gene_j[k].tolist())) == 10


def test_a_search_disturbs_nothing(pkg):
    G, S, seed = 300, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 100, seed)
    exp = tpc.oracle(X, gid, len(lev), 0, None)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        first = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        codes, ref, info = ctx.get_codes(0, G, 0, G), ctx.ref_mask(), ctx.info()
        tp = ctx.top_pairs(N)                                                    # (tie-free data: the gene-order planes are made on demand)
        same(tp, exp, N, "after a build")
        assert np.array_equal(ctx.rank_shift(), exp.D)
        assert np.array_equal(ctx.get_codes(0, G, 0, G), codes) and np.array_equal(ctx.ref_mask(), ref)
        after = ctx.info()
        own = ("planes_on_demand", "top_pairs_hist_us", "top_pairs_emit_us")     # (the planes it had made, and its own two timers)
        assert all(after[k] == info[k] for k in info if k not in own), {k: (info[k], after[k]) for k in info if after[k] != info[k]}
        assert after["top_pairs_hist_us"] > 0 and after["top_pairs_emit_us"] > 0
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == first[1:] and np.array_equal(again[0], first[0], equal_nan=True)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    X, gid, ng, a, b = tpc.case("three_0_2")
    G, S = X.shape
    ctx, _, _ = open_case(pkg, "three_0_2")
    with ctx:
        for kw, pattern in ((dict(n=0), "n_want = 0, between 1 and 2\\^20"), (dict(n=(1 << 20) + 1), "n_want = 1048577"),
                            (dict(n=5, a=0, b=0), "b == a == 0"), (dict(n=5, a=3), "a = 3 is outside the groups \\[0, 3\\)"),
                            (dict(n=5, a=0, b=3), "b = 3 is outside the groups"), (dict(n=5, a=-1), "a = -1 is outside")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                ctx.top_pairs(**kw)
            assert e.value.status == pkg._ffi.REO_EINVAL and "reo_top_pairs" in e.value.message
        with pytest.raises(pkg.DimensionMismatch, match="reo_rank_shift: b == a == 1"):
            ctx.rank_shift(a=1, b=1)
        with pytest.raises(pkg.DimensionMismatch, match="gene_mask has shape"):
            ctx.top_pairs(5, gene_mask=np.ones(G + 1, dtype=bool))
        # a refused call writes nothing
        P = pkg._ffi._ptr
        gi, gj = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
        counts, key, found = np.full((4, 4), -7, dtype=np.int32), np.full((4, 2), -7, dtype=np.int64), np.full(1, -7, dtype=np.int64)
        with pytest.raises(pkg.DimensionMismatch, match="b == a"):
            pkg._ffi.check(ctx._L.reo_top_pairs(ctx._h, 2, 2, None, 4, P(gi), P(gj), P(counts), P(key), P(found), None))
        with pytest.raises(pkg.DimensionMismatch, match="must not be null"):
            pkg._ffi.check(ctx._L.reo_top_pairs(ctx._h, 0, 2, None, 4, P(gi), None, P(counts), P(key), P(found), None))
        assert (gi == -7).all() and (gj == -7).all() and (counts == -7).all() and (key == -7).all() and found[0] == -7
        pkg._ffi.check(ctx._L.reo_top_pairs(ctx._h, 0, 2, None, 4, P(gi), P(gj), P(counts), P(key), P(found), None))   # passes_run is optional
        exp = tpc.expected("three_0_2")
        assert found[0] == 4 and np.array_equal(gi, exp.gene_i[:4]) and np.array_equal(key[:, 0], exp.num[:4])
        ctx.set_valid_mask(np.ones((G, S), dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs compares on the bit planes of the whole matrix.*while a mask is set"):
            ctx.top_pairs(5)
        with pytest.raises(pkg.DimensionMismatch, match="reo_rank_shift compares on the bit planes"):
            ctx.rank_shift()
        ctx.set_valid_mask(None)
        same(ctx.top_pairs(5, a=0, b=2), exp, 5, "mask cleared")
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs is not available on a sharded context"):
            ctx.top_pairs(5)
        with pytest.raises(pkg.DimensionMismatch, match="reo_rank_shift is not available on a sharded context"):
            ctx.rank_shift()
    with pkg.Context(device=0, seed=1) as ctx:                                   # no matrix, no groups
        with pytest.raises(pkg.DimensionMismatch, match="no expression matrix"):
            ctx.top_pairs(5)
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="no groups"):
            ctx.top_pairs(5)
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_top_pairs is not available on a reo_create_multi context"):
            ctx.top_pairs(5)
        with pytest.raises(pkg.DimensionMismatch, match="reo_rank_shift is not available on a reo_create_multi context"):
            ctx.rank_shift()


def test_run_identify_degs_carries_the_search(pkg):
    K = 20
    today = {"k", "result", "labels", "iters_run", "trace"}
    # two groups: the dict's TopPairs equals a direct call
    X, gid, ng, a, b = tpc.case("count_i64")
    G = X.shape[0]
    names = [f"g{i}" for i in range(G)]
    args = (X, gid.tolist(), names, 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    plain = pkg.run_identify_degs(*args, seed=3, device=0)
    on = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=K)
    assert set(plain.comparisons[0]) == today and set(on.comparisons[0]) == today | {"top_pairs"}
    assert np.array_equal(on.result, plain.result, equal_nan=True) and on.trace == plain.trace
    ctx, _, _ = open_case(pkg, "count_i64")
    with ctx:
        direct = ctx.top_pairs(K)
    got = on.comparisons[0]["top_pairs"]
    assert identical(got, direct) and (got.a, got.b) == (0, None)
    same(got, tpc.expected("count_i64"), K, "two groups")
    # three groups, one contrast: a and b are the contrast's groups
    X, gid, ng, _, _ = tpc.case("three_0_2")
    G = X.shape[0]
    args = (X, gid.tolist(), [f"g{i}" for i in range(G)], 0.01, 1.0, 0.05, np.ones(G, dtype=bool), 3, 1)
    run = pkg.run_identify_degs(*args, seed=3, device=0, contrasts=[(0, 2)], top_pairs=K)
    got = run.comparisons[0]["top_pairs"]
    assert len(run.comparisons) == 1 and (got.a, got.b) == (0, 2)
    same(got, tpc.expected("three_0_2"), K, "contrast (0, 2)")
    # the reference's comparisons of three groups: group k against every other sample
    run = pkg.run_identify_degs(*args, seed=3, device=0, top_pairs=K)
    assert [(cm["top_pairs"].a, cm["top_pairs"].b) for cm in run.comparisons] == [(0, None), (1, None), (2, None)]
    same(run.comparisons[1]["top_pairs"], tpc.expected("three_1_rest"), K, "group 1 against the rest")


def test_reoa_writes_a_top_pairs_file(pkg, tmp_path):
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path), seed=0x5EED0001, device=0, top_pairs=30)
    run = df.attrs["run"]
    tp = run.comparisons[0]["top_pairs"]
    lines = (tmp_path / "fn_expr_group1_group2_top_pairs.tsv").read_text().split("\n")
    assert lines[0].split("\t") == ["gene_i", "gene_j", "direction", "score", "rank_score", "gt_A", "eq_A", "gt_B", "eq_B"]
    assert lines[-1] == "" and len(lines) == tp.gene_i.size + 2 and tp.gene_i.size == 30
    want = [run.gene_names[int(tp.gene_i[0])], run.gene_names[int(tp.gene_j[0])], str(int(tp.direction[0])), repr(float(tp.score[0])),
            repr(float(tp.rank_score[0]))] + [str(int(v)) for v in (tp.n_gt[0, 0], tp.n_eq[0, 0], tp.n_gt[0, 1], tp.n_eq[0, 1])]
    assert lines[1].split("\t") == want
    assert (np.diff(tp.score) <= 0).all()
