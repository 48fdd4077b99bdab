"""The core path -- pair kernel, class table, K2, the passes -- at 18 position planes (131 072 genes and more), held to the oracle.

The whole-table oracle cannot follow there (its table at 131 584 genes is 17 GB), so the reference is the thin one of
tests/big_plane_cases.py: strips of 32 columns or rows of the class table from the oracle's counts and tie coins, their tallies, and
the oracle's own pass arithmetic over tallies (tests/test_big_plane_cases_cpu.py holds each piece to the whole-table oracle at a few
hundred genes).  Every two-group case has 16 interleaved samples and pval_reo = 0.1 (thresholds 7 of 8: all nine classes occur).

Where the lines of the table are: a row is Gp / 2 bytes with Gp the gene count padded to 1024 (132 096 at 131 584 genes: 66 048 bytes), so
byte offsets pass 2^32 in row 65 027 and 2^33 in row 130 055 -- there the uint32 word index of the row scans passes 2^31.  The row strips
sit on those rows, and on 65 264 / 130 544, where the lines would be if rows were G / 2 bytes."""
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

import big_plane_cases as bp
from test_gpu_parity import P_ATOL, STAT_RTOL, _check_result   # (_check_result: tallies equal, p / padj within P_ATOL, statistics within STAT_RTOL)

pytestmark = pytest.mark.gpu

G18 = 131584            # 128.5 x 1024: 18 planes, a padded last chunk of 1024 genes
SEED = 0x5EED0B18
THREADS = 8             # the strips of the reference are independent: ctypes and numpy release the interpreter lock


def _pool_map(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


def _line_rows(G):
    """rows in which the byte offset of the class table passes 2^32 and 2^33 (the second: the uint32 word index passes 2^31)"""
    row_bytes = (G + 1023) // 1024 * 1024 // 2
    return (1 << 32) // row_bytes, (1 << 33) // row_bytes


def _p_error(res, exp):
    return float(np.abs(res[:, :2] - exp[:, :2]).max())


def _stat_error(res, exp):
    """largest relative error of the statistics where they are not next to zero (there _check_result's absolute 1e-9 decides)"""
    d, e = np.abs(res[:, 11:] - exp[:, 11:]), np.abs(exp[:, 11:])
    big_enough = e > 1e-2
    return float((d[big_enough] / e[big_enough]).max()) if big_enough.any() else 0.0


def _open(pkg, X, gid, ngroups, seed=SEED):
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_matrix(X)
    ctx.set_groups(gid, ngroups)
    thr = ctx.compute_thresholds(bp.PVAL_REO)
    return ctx, thr


@pytest.fixture(scope="module")
def big(request, pkg, oracle):
    """One context per matrix of tests/big_plane_cases.py at 131 584 genes with its class table built, and the four column strips of the
    reference set from the oracle; shared by the table, K2 and pass cases (pytest runs a matrix's cases together)."""
    name = request.param
    recipe, has_ties = bp.MATRICES[name]
    gid = bp.labels()
    X = recipe(G18, SEED)
    Xf = np.asfortranarray(X.astype(np.float64))
    ctx, thr = _open(pkg, X, gid, 2)
    assert thr.tolist() == [[7, 7], [7, 7]] and np.array_equal(thr, bp.thresholds(oracle, gid, 2))
    ctx.build_pairs(0)
    runs = bp.ref_runs(G18)
    strips = dict(zip(runs, _pool_map(lambda j0: bp.expected_codes(oracle, Xf, gid, thr, SEED, 0, G18, j0, j0 + bp.STRIP), runs)))
    for c in strips.values():
        c.setflags(write=False)
    ns = SimpleNamespace(name=name, has_ties=has_ties, X=X, Xf=Xf, gid=gid, thr=thr, ctx=ctx, strips=strips, ref0=bp.ref_set(G18), rows=None)
    yield ns
    ctx.close()
    pkg._ffi.trim_memory()   # (an 8.7 GB class table went back to the block cache: return it to the driver)


def _row_strips(oracle, b):
    """{i0: n x G codes} of the row strips, from the oracle, once per matrix"""
    if b.rows is None:
        r32, r33 = _line_rows(G18)
        assert (r32, r33) == (65027, 130055)
        spans = [(0, 32), (r32 - 16, 32), (65264, 32), (r33 - 16, 32), (130544, 32), (G18 - 64, 64)]
        codes = _pool_map(lambda s: bp.expected_codes(oracle, b.Xf, b.gid, b.thr, SEED, s[0], s[0] + s[1], 0, G18), spans)
        b.rows = {s[0]: c for s, c in zip(spans, codes)}
    return b.rows


ALL = pytest.mark.parametrize("big", ["free", "counts", "band"], indirect=True)



@ALL
def test_class_table_columns_blocks_and_mirror(big, oracle):
    """(a) k1w_pairs<18, TIES> with the generated 18-plane count loop, the big plane layout, the table's writes past 4 and 8 GiB: whole
    columns of the class table (every row of it, every chunk's first and last genes among the columns) against the oracle."""
    ctx, G = big.ctx, G18
    info = ctx.info()
    assert info["transform_in_lds"] == 3 and info["has_ties"] == big.has_ties and info["Gp"] == 132096
    assert info["table_bytes"] > (8 << 30)
    for j0, exp in big.strips.items():
        bp.check_codes(ctx.get_codes(0, G, j0, j0 + bp.STRIP), exp, 0, j0, f"{big.name} columns {j0}")
    if big.name == "counts":   # all nine classes are there to be got wrong
        seen = sum(np.bincount(c[c < 9], minlength=9) for c in big.strips.values())
        assert (seen > 0).all(), seen
    rng = np.random.default_rng(SEED)
    blocks = [(int(a), int(b)) for a, b in rng.integers(0, G - 40, size=(16, 2))]
    for (i0, j0), exp in zip(blocks, _pool_map(lambda ij: bp.expected_codes(oracle, big.Xf, big.gid, big.thr, SEED, ij[0], ij[0] + 40, ij[1], ij[1] + 40), blocks)):
        bp.check_codes(ctx.get_codes(i0, i0 + 40, j0, j0 + 40), exp, i0, j0, f"{big.name} block")
    # both halves of half-height items (rows 0-15 and 16-31 of the tile), 64 of their 256 columns: tests/big_plane_cases.HALF_ITEMS
    for (i0, j0), exp in zip(bp.HALF_ITEMS, _pool_map(lambda ij: bp.expected_codes(oracle, big.Xf, big.gid, big.thr, SEED, ij[0], ij[0] + 32, ij[1], ij[1] + 64), bp.HALF_ITEMS)):
        bp.check_codes(ctx.get_codes(i0, i0 + 32, j0, j0 + 64), exp, i0, j0, f"{big.name} half-height item")
    for (a, b) in [(0, G - 256), (G - 256, G - 256), (131000, 65400)]:
        bp.check_mirror(ctx.get_codes(a, a + 256, b, b + 256), ctx.get_codes(b, b + 256, a, a + 256), a, b, big.name)


@ALL
def test_class_table_rows_at_the_offset_lines(big, oracle):
    """(a) whole rows of the class table against the oracle: the first rows, the rows where the table's byte offsets pass 2^32 and 2^33,
    and the last 64 rows (the last i-tiles, whose only chunk is the padded last one)."""
    for i0, exp in _row_strips(oracle, big).items():
        bp.check_codes(big.ctx.get_codes(i0, i0 + exp.shape[0], 0, G18), exp, i0, 0, f"{big.name} rows {i0}")


@ALL
def test_k2_scans_a_table_past_4_gib(big, oracle):
    """(b) K2 (tally_rows: one wave per row, the whole row) on an 8.7 GB table: the tallies over the reference set against the oracle's
    strips; the tallies over ALL genes -- a scan of every word of the row -- against the oracle for the genes of the column strips
    (through the mirror rule) and of the row strips (directly: rows on both sides of the 2^32 and 2^33 byte lines); exact identities."""
    ctx, G = big.ctx, G18
    bp.check_tally(ctx.tally(big.ref0), bp.ref_set_tally(big.strips), what=f"{big.name} tally(ref0)")
    full = ctx.tally(np.ones(G, dtype=bool))
    for j0, c in big.strips.items():
        rows = np.arange(j0, j0 + bp.STRIP)
        bp.check_tally(full[rows], bp.column_histogram(c), rows, f"{big.name} tally(ones) at columns {j0}")
    for i0, c in _row_strips(oracle, big).items():
        rows = np.arange(i0, i0 + c.shape[0])
        bp.check_tally(full[rows], bp.strip_tally(c), rows, f"{big.name} tally(ones) at rows {i0}")
    assert np.array_equal(full.sum(axis=1), np.full(G, G - 1)) and full.min() >= 0
    tot = full.sum(axis=0, dtype=np.int64)
    assert np.array_equal(tot, tot[::-1])                      # sum_i cont[i, c] == sum_i cont[i, 8 - c]
    m = np.random.default_rng(SEED + 1).random(G) < 0.3
    assert np.array_equal(ctx.tally(m).astype(np.int64) + ctx.tally(~m), full)


@pytest.mark.parametrize("n_iter", [1, 6])
@pytest.mark.parametrize("big", ["free", "counts"], indirect=True)
def test_passes_at_18_planes(big, oracle, n_iter):
    """(c) identify_degs on the 18-plane table against the oracle's iteration (tests/big_plane_cases.reference_run: the loop of
    oracle_iterate, every pass by oracle_iter_stats): passes, trace and tallies equal, p / padj and the statistics within the project's
    tolerances.  One pass: the reference takes its tallies from the oracle's strips, nothing of the device's is in it.  Six passes: the
    reference takes each pass's tallies from the device's full scan, ctx.tally, which test_k2_scans_a_table_past_4_gib holds to the
    oracle; the run itself comes by them through k2_tally's delta form and the light passes."""
    ctx, G = big.ctx, G18
    got = ctx.identify_degs(big.ref0, 1.0, 0.05, n_iter, 3)
    mask = ctx.ref_mask()                                          # (reo_tally drops the run's mask: first)
    if n_iter == 1:
        strip_cont = bp.ref_set_tally(big.strips)

        def tally_fn(ref):
            assert np.array_equal(ref != 0, big.ref0)
            return strip_cont
        assert np.array_equal(mask, big.ref0)
    else:
        tally_fn = ctx.tally
    exp = bp.reference_run(tally_fn, G, big.ref0, 1.0, 0.05, n_iter, 3)
    print(big.name, n_iter, "passes", got[1], "trace", got[2], "reference", exp[1], exp[2])
    print("largest error of p / padj", _p_error(got[0], exp[0]), "of", P_ATOL, "; of the statistics, relative", _stat_error(got[0], exp[0]), "of", STAT_RTOL)
    bp.check_run(got, exp, _check_result, f"{big.name} n_iter {n_iter}")
    assert _p_error(got[0], exp[0]) <= P_ATOL
    bp.check_tally(ctx.tally(mask), got[0][:, 2:11].astype(np.int32), what=f"{big.name} tally(ref_mask)")
    assert got[1] == n_iter or abs(int(mask.sum()) - got[2][-1][1]) < 3
    if n_iter == 6:
        assert got[1] >= 3 and got[2][-1][0] > 0, got[2]           # passes whose reference set moves by a few genes, and DEGs to move it


@pytest.mark.parametrize("kind", ["tie_rich", "tie_free"])
def test_three_groups_recounted_at_18_planes(pkg, oracle, monkeypatch, kind):
    """(d) k1w_pairs_multi<18, TIES>: three groups, 9 samples, each comparison recounted by the wave form (REO_SHARE_GROUP_COUNTS=0; the
    shared planes would be (C + 1) Gp^2 2 bytes = 138 GB here and stay out).  Sampled blocks against the oracle: first and last columns,
    across 65 536 and 131 072, the diagonal, the padded tail."""
    monkeypatch.setenv("REO_SHARE_GROUP_COUNTS", "0")
    G, S, C = G18, 9, 3
    gid = bp.labels(S, C)
    assert gid.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2]
    X = np.random.default_rng(1).integers(0, 1000, size=(G, S)) if kind == "tie_rich" else bp.free(G, SEED, S, gid)
    Xf = np.asfortranarray(X.astype(np.float64))
    blocks = [(0, G - 64, 64), (G - 64, 0, 64), (0, 0, 48), (65504, 65504, 64), (100, 65500, 64), (131040, 131040, 64), (200, 131040, 64),
              (131050, 65510, 48), (G - 48, G - 48, 48), (G - 33, 17, 32), (131072, G - 64, 64)]
    with pkg.Context(device=0, seed=SEED) as ctx:
        ctx.set_matrix(X); ctx.set_groups(gid, C)
        thr = ctx.compute_thresholds(bp.PVAL_REO)
        assert np.array_equal(thr, bp.thresholds(oracle, gid, C))
        for k in (1, 0):
            ctx.build_pairs(k)
            info = ctx.info()
            assert info["shared_group_counts"] == 0 and info["has_ties"] == (1 if kind == "tie_rich" else 0) and info["transform_in_lds"] == 3
            exps = _pool_map(lambda b: bp.expected_codes(oracle, Xf, gid, thr, SEED, b[0], b[0] + b[2], b[1], b[1] + b[2], C, k), blocks)
            for (i0, j0, n), exp in zip(blocks, exps):
                bp.check_codes(ctx.get_codes(i0, i0 + n, j0, j0 + n), exp, i0, j0, f"{kind} k {k}")
    pkg._ffi.trim_memory()


@pytest.mark.parametrize("G,name", [(131071, "counts"), (131072, "free")])
def test_the_plane_boundary(pkg, oracle, G, name):
    """(e) 131 071 genes: the last count with 17 planes -- positions up to 131 070, and in `counts` the top value's tie group ends at
    position 131 071 = 2^17 - 1.  131 072: the first count with 18.  Sampled blocks of codes and of raw counts against the oracle: the
    first and last genes, both sides of 65 536."""
    recipe, has_ties = bp.MATRICES[name]
    gid = bp.labels()
    X = recipe(G, SEED)
    Xf = np.asfortranarray(X.astype(np.float64))
    blocks = [(0, G - 64, 64), (G - 64, 0, 64), (0, 0, 48), (65504, 65504, 64), (100, 65500, 64), (65500, 100, 64), (G - 48, G - 48, 48),
              (G - 33, 17, 32), (65536, G - 64, 64), (G - 64, 65472, 64)]
    ctx, thr = _open(pkg, X, gid, 2)
    with ctx:
        for (i0, j0, n) in blocks[:6]:
            gt, eq = ctx.pair_counts(i0, i0 + n, j0, j0 + n)
            egt, eeq = oracle.pair_counts(Xf, gid, 2, i0, i0 + n, j0, j0 + n)
            assert np.array_equal(gt, egt) and np.array_equal(eq, eeq), (G, i0, j0)
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["transform_in_lds"] == 3 and info["has_ties"] == has_ties and info["Gp"] == 131072
        exps = _pool_map(lambda b: bp.expected_codes(oracle, Xf, gid, thr, SEED, b[0], b[0] + b[2], b[1], b[1] + b[2]), blocks)
        for (i0, j0, n), exp in zip(blocks, exps):
            bp.check_codes(ctx.get_codes(i0, i0 + n, j0, j0 + n), exp, i0, j0, f"G {G}")
        bp.check_mirror(ctx.get_codes(0, 256, G - 256, G), ctx.get_codes(G - 256, G, 0, 256), 0, G - 256, f"G {G}")
    pkg._ffi.trim_memory()


def test_merge_rank_with_more_than_48_kb_of_splitters(pkg, oracle):
    """(f) 196 700 genes: 193 sort chunks, a splitter table of 193 x 32 x 8 = 49 408 bytes -- the first geometry at which launch_full_pass
    raises k3_merge_rank's dynamic LDS limit.  A 19.4 GB class table (8 samples, tie-free); tallies over the reference set against the
    oracle's strips, the run of three passes against the oracle's iteration over the device's scans."""
    G, S = 196700, 8
    assert (G + 1023) // 1024 * 32 * 8 == 49408 > 48 * 1024 >= (196608 + 1023) // 1024 * 32 * 8
    gid = bp.labels(S)
    X = bp.free(G, SEED, S, gid)
    Xf = np.asfortranarray(X.astype(np.float64))
    ref0 = bp.ref_set(G)
    ctx, thr = _open(pkg, X, gid, 2)
    with ctx:
        ctx.build_pairs(0)
        info = ctx.info()
        assert info["transform_in_lds"] == 3 and info["has_ties"] == 0 and info["table_bytes"] > 19 * 10 ** 9
        runs = bp.ref_runs(G)
        strips = dict(zip(runs, _pool_map(lambda j0: bp.expected_codes(oracle, Xf, gid, thr, SEED, 0, G, j0, j0 + bp.STRIP), runs)))
        for j0, exp in strips.items():
            bp.check_codes(ctx.get_codes(0, G, j0, j0 + bp.STRIP), exp, 0, j0, f"columns {j0}")
        bp.check_tally(ctx.tally(ref0), bp.ref_set_tally(strips), what="tally(ref0)")
        full = ctx.tally(np.ones(G, dtype=bool))
        for j0, c in strips.items():
            rows = np.arange(j0, j0 + bp.STRIP)
            bp.check_tally(full[rows], bp.column_histogram(c), rows, f"tally(ones) at columns {j0}")
        assert np.array_equal(full.sum(axis=1), np.full(G, G - 1))
        got = ctx.identify_degs(ref0, 1.0, 0.05, 3, 3)
        mask = ctx.ref_mask()
        exp = bp.reference_run(ctx.tally, G, ref0, 1.0, 0.05, 3, 3)
        print("passes", got[1], "trace", got[2], "reference", exp[1], exp[2])
        print("largest error of p / padj", _p_error(got[0], exp[0]), "of", P_ATOL, "; of the statistics, relative", _stat_error(got[0], exp[0]), "of", STAT_RTOL)
        bp.check_run(got, exp, _check_result, "196700")
        bp.check_tally(ctx.tally(mask), got[0][:, 2:11].astype(np.int32), what="tally(ref_mask)")
        # the first pass once more with nothing of the device's in the reference: its tallies from the oracle's strips
        one = ctx.identify_degs(ref0, 1.0, 0.05, 1, 3)
        bp.check_run(one, bp.reference_run(lambda ref: bp.ref_set_tally(strips), G, ref0, 1.0, 0.05, 1, 3), _check_result, "196700, one pass")
    pkg._ffi.trim_memory()   # (a 19.4 GB class table went back to the block cache: return it to the driver)
