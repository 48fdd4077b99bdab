"""The top-scoring-pair search (reo_top_pairs, reo_rank_shift), the parts that need no GPU: the ABI, the key, the tile rule, the digit pick,
the pass loop and the host argument checks of csrc/top_pairs.h under the sanitizers, the pass loop against the numpy oracle of
tests/top_pairs_cases.py, and the Python helpers (the TopPairs algebra, top_pairs_plan, the TSV writer, the top_pairs=None defaults)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import top_pairs_cases as tpc
import wide_top_pairs_cases as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    L = pkg._ffi.lib()
    for s, nargs in (("reo_rank_shift", 4), ("reo_top_pairs", 11)):               # (ctx, a, b, D) and the eleven parameters of the search
        m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, m.group(1)
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == nargs
        assert hasattr(L, s)
    assert L.reo_version() >= 1300
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    assert "2 delta + eq_A / S_A - eq_B / S_B" in header and "2 delta + eq_A / S_A - eq_B / S_B" in pkg.TopPairs.__doc__
    p = inspect.signature(pkg.Context.top_pairs).parameters
    assert list(p) == ["self", "n", "a", "b", "gene_mask"] and p["a"].default == 0 and p["b"].default is None and p["gene_mask"].default is None
    p = inspect.signature(pkg.Context.rank_shift).parameters
    assert list(p) == ["self", "a", "b"] and p["a"].default == 0 and p["b"].default is None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_pairs") / "top_pairs_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "top_pairs_driver.cpp")])
    return exe


def test_key_tiles_digit_pick_pass_loop_and_argument_checks_under_sanitizers(driver):
    """tests/top_pairs_driver.cpp: every argument check with its message; key packing and digits; the tile rule enumerated for G in {1, 2,
    63, 64, 65, 300}; tp_pick_digit on hand-made histograms; tp_select against a full sort.  AddressSanitizer and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 6000
    tiles = {int(l.split()[1]): (int(l.split()[2]), int(l.split()[3])) for l in lines if l.startswith("tiles ")}
    assert sorted(tiles) == [1, 2, 63, 64, 65, 300]
    assert tiles[64] == (8, 32) and tiles[65][0] == 17                            # one column tile: 8 row tiles; 65 genes: a second tile for column 64
    assert tiles[300][0] < tiles[300][1] / 2                                      # less than half of the launched waves walk anything


def run_select(driver, name, n, cap, gene_mask=None):
    cases = wt if name in wt.DEEP else tpc                                       # (deep_gamma, limit: tests/wide_top_pairs_cases.py)
    X, gid, ng, a, b = cases.case(name)
    exp = cases.expected(name) if gene_mask is None else tpc.oracle(X, gid, ng, a, b, gene_mask)
    G = X.shape[0]
    n_max = 2 * exp.sizes[0] * exp.sizes[1]
    g_max = int(exp.D.max() - exp.D.min())
    text = f"{G} {n} {cap} {n_max} {g_max} {exp.gene_i.size}\n" + tpc.key_lines(exp, G)
    run = subprocess.run([driver, "select"], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    passes, cand = int(lines[0].split()[1]), int(lines[1].split()[1])
    got = np.array([l.split() for l in lines[2:]], dtype=np.int64).reshape(-1, 2)
    k = min(n, exp.gene_i.size)
    assert got.shape[0] == k and np.array_equal(got[:, 0], exp.gene_i[:k]) and np.array_equal(got[:, 1], exp.gene_j[:k]), (name, n, cap)
    return passes, cand


@pytest.mark.parametrize("name", tpc.EQUALITY + list(wt.DEEP))
def test_the_pass_loop_selects_the_oracles_order_at_any_capacity(driver, name):
    """the library's own pass loop, a host histogram in place of the kernel: the oracle's first 50 pairs, at the default capacity and at
    capacity = n; the tight buffer needs more passes wherever more than 50 keys share the first digit's bin.  deep_gamma and limit: Gamma
    at and above 2^32, whose upper bits tp_pack puts into TpKey.hi, decides among hundreds of pairs at |N| = 2 S_A S_B, and at the
    limit |N| has the top bit of its field set"""
    exp = wt.expected(name) if name in wt.DEEP else tpc.expected(name)
    assert np.array_equal(exp.N, -exp.N.T)                                        # N is antisymmetric
    p_default, c_default = run_select(driver, name, 50, 0)
    p_tight, c_tight = run_select(driver, name, 50, 50)
    assert 1 <= p_default <= p_tight <= 10 and 50 <= c_tight <= c_default <= exp.gene_i.size
    G = (wt if name in wt.DEEP else tpc).case(name)[0].shape[0]                   # the numpy restatement of the loop counts the same
    assert wt.select_passes(exp, G, 50, wt.default_capacity(50)) == (p_default, c_default) and wt.select_passes(exp, G, 50, 50) == (p_tight, c_tight)
    if name in ("separated", "level") or name in wt.DEEP:
        assert p_tight > p_default
    if name in wt.DEEP:                                                          # the tight run refines through digits of Gamma that lie in TpKey.hi
        head = exp.rank_num[:50]
        assert np.unique(head >> 32).size >= 2 and (np.abs(exp.num[:51]) == 2 * exp.sizes[0] * exp.sizes[1]).all() and p_tight >= 4
        if name == "limit":
            assert abs(int(exp.num[0])) >> 30 == 1 and int(head.max()) >> 37 == 1
    if name == "level":
        assert run_select(driver, name, 5000, 0)[1] == 4950                       # fewer pairs than wanted: all of them


def test_the_cases_are_what_the_gpu_tests_say_they_are():
    e = tpc.expected("count_i64")
    a = np.abs(e.num)
    assert np.unique(a).size == 90 and (a == a[49]).sum() == 10                   # 90 distinct |N|, ten pairs share the cut's
    e = tpc.expected("rank130")
    a = np.abs(e.num)
    assert e.sizes == (1, 20) and a[49] == 32 and (a == 32).sum() == 47
    e = tpc.expected("separated")
    a = np.abs(e.num)
    full = 2 * e.sizes[0] * e.sizes[1]
    assert (a == full).sum() == 8400 and a.size == 19900                          # Gamma decides among 8 400 pairs
    assert e.rank_num[49] != e.rank_num[50] and a[50] == full                     # no two pairs share (|N|, Gamma) at the cut
    e = tpc.expected("level")
    assert not e.num.any() and not e.rank_num.any() and not e.D.any() and e.gene_i.size == 4950
    iu, ju = np.triu_indices(100, 1)
    assert np.array_equal(e.gene_i, iu) and np.array_equal(e.gene_j, ju)
    e = tpc.expected("three_0_2")
    assert e.sizes == (20, 12)                                                   # group 1 belongs to neither side
    assert tpc.expected("three_1_rest").sizes == (33, 32)
    # tie-free data: the score is Geman's |gt_A / S_A - gt_B / S_B| and Gamma / (2 S_A S_B) Tan's |mean_A(r_i - r_j) - mean_B(r_i - r_j)|
    X, gid, _, _, _ = tpc.case("separated")
    e = tpc.expected("separated")
    sa, sb = e.sizes
    c = e.counts[:200].astype(np.float64)
    assert np.allclose(np.abs(e.num[:200]) / (2.0 * sa * sb), np.abs(c[:, 0] / sa - c[:, 2] / sb), rtol=0, atol=1e-12)
    r = np.argsort(np.argsort(X, axis=0), axis=0).astype(np.float64)
    d = r[e.gene_i[:200]] - r[e.gene_j[:200]]
    tan = np.abs(d[:, gid == 0].mean(axis=1) - d[:, gid == 1].mean(axis=1))
    assert np.allclose(e.rank_num[:200] / (2.0 * sa * sb), tan, rtol=0, atol=1e-9)


def test_the_oracle_of_the_large_cases_is_the_full_oracle_at_a_small_size():
    """moved_case / moved_oracle serve the gene counts whose G x G oracle would be too large; at G = 200 both oracles exist"""
    X, gid, genes = tpc.moved_case(200, 21)
    assert genes[0] == 63 and genes[-1] == 199 and len(set(genes.tolist())) == 6
    full = tpc.oracle(X, gid, 2, 0, None)
    gi, gj, counts, num, gam, D = tpc.moved_oracle(X, gid, genes, 50)
    assert np.array_equal(D, full.D)
    assert np.array_equal(gi, full.gene_i[:50]) and np.array_equal(gj, full.gene_j[:50]) and np.array_equal(counts, full.counts[:50])
    assert np.array_equal(num, full.num[:50]) and np.array_equal(gam, full.rank_num[:50])
    assert (np.abs(full.num) > 0).sum() < 6 * 200                                # only pairs with a moved gene have N != 0


def hand_made(pkg):
    return pkg.TopPairs(gene_i=np.array([2, 0, 2, 1, 5], dtype=np.int32), gene_j=np.array([7, 2, 3, 4, 6], dtype=np.int32),
                        n_gt=np.array([[4, 0], [0, 5], [3, 1], [1, 2], [2, 2]], dtype=np.int32),
                        n_eq=np.array([[0, 0], [0, 0], [1, 0], [0, 1], [0, 1]], dtype=np.int32),
                        num=np.array([40, -40, 27, -10, 0], dtype=np.int64), rank_num=np.array([90, 70, 5, 5, 0], dtype=np.int64),
                        side_sizes=np.array([4, 5], dtype=np.int64), a=0, b=None, passes=2)


def test_top_pairs_algebra_on_a_hand_made_list(pkg):
    tp = hand_made(pkg)
    assert pkg.TopPairs._fields == ("gene_i", "gene_j", "n_gt", "n_eq", "num", "rank_num", "side_sizes", "a", "b", "passes")
    assert tp.score.dtype == np.float64 and np.array_equal(tp.score, np.array([1.0, 1.0, 27 / 40, 10 / 40, 0.0]))
    assert np.array_equal(tp.rank_score, np.array([90, 70, 5, 5, 0]) / 40.0)
    assert tp.direction.dtype == np.int8 and tp.direction.tolist() == [1, -1, 1, -1, 0]
    # num is what the counts give: w = 2 gt + eq - S per side
    w = 2 * tp.n_gt.astype(np.int64) + tp.n_eq - tp.side_sizes[None, :]
    assert np.array_equal(w[:, 0] * 5 - w[:, 1] * 4, tp.num)
    # greedy k-TSP: (2, 7); (0, 2) and (2, 3) reuse gene 2; (1, 4); (5, 6)
    assert tp.disjoint(1).tolist() == [0] and tp.disjoint(2).tolist() == [0, 3] and tp.disjoint(3).tolist() == [0, 3, 4]
    assert tp.disjoint(10).tolist() == [0, 3, 4] and tp.disjoint(0).tolist() == [] and tp.disjoint(2).dtype == np.int64
    genes, rowptr, partner = tp.csr()
    assert genes.dtype == np.int32 and rowptr.dtype == np.int64 and partner.dtype == np.int32
    assert genes.tolist() == [2, 0, 2, 1, 5] and rowptr.tolist() == [0, 1, 2, 3, 4, 5] and partner.tolist() == [7, 2, 3, 4, 6]
    # votes: outcome 2 = gene_i above gene_j; three samples
    outcome = np.array([[2, 0, 1], [0, 2, 1], [2, 2, 0], [0, 0, 2], [2, 0, 1]], dtype=np.uint8)
    z = np.zeros((5, 2), dtype=np.int32)
    sup = pkg.PairSupport(genes, rowptr, partner, None, z, z, outcome, np.array([4, 5], dtype=np.int64))
    v = tp.votes(sup)
    # sample 0: +1 +1 +1 +1 (0) = 4; sample 1: -1 -1 +1 +1 = 0; sample 2: 0 0 -1 -1 = -2
    assert v.dtype == np.int32 and v.tolist() == [4, 0, -2]
    with pytest.raises(pkg.DimensionMismatch, match="outcomes=True"):
        tp.votes(sup._replace(outcome=None))
    with pytest.raises(pkg.DimensionMismatch, match="lists 4 pairs"):
        tp.votes(sup._replace(outcome=outcome[:4]))
    empty = pkg.TopPairs(np.zeros(0, np.int32), np.zeros(0, np.int32), z[:0], z[:0], np.zeros(0, np.int64), np.zeros(0, np.int64),
                         np.array([4, 5], dtype=np.int64), 0, 1, 1)
    assert empty.score.size == 0 and empty.disjoint(3).size == 0 and empty.csr()[1].tolist() == [0]


def test_write_top_pairs_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E", "f", "g", "h"]
    path = tmp_path / "t.tsv"
    pkg.write_top_pairs_tsv(str(path), names, hand_made(pkg))
    assert path.read_bytes() == (b"gene_i\tgene_j\tdirection\tscore\trank_score\tgt_A\teq_A\tgt_B\teq_B\n"
                                 b"geneC\th\t1\t1.0\t2.25\t4\t0\t0\t0\n"
                                 b"A1BG\tgeneC\t-1\t1.0\t1.75\t0\t0\t5\t0\n"
                                 b"geneC\td\t1\t0.675\t0.125\t3\t1\t1\t0\n"
                                 b"TP53\tE\t-1\t0.25\t0.125\t1\t0\t2\t1\n"
                                 b"f\tg\t0\t0.0\t0.0\t2\t0\t2\t1\n")
    z = np.zeros((0, 2), dtype=np.int32)
    empty = pkg.TopPairs(np.zeros(0, np.int32), np.zeros(0, np.int32), z, z, np.zeros(0, np.int64), np.zeros(0, np.int64),
                         np.array([3, 3], dtype=np.int64), 0, None, 1)
    pkg.write_top_pairs_tsv(str(path), names, empty)
    assert path.read_bytes() == b"gene_i\tgene_j\tdirection\tscore\trank_score\tgt_A\teq_A\tgt_B\teq_B\n"


def test_top_pairs_defaults_to_none_and_is_keyword_only(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["top_pairs"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert {"TopPairs", "write_top_pairs_tsv"} <= set(pkg.__all__)
    # the plans that existing callers use keep their signatures
    assert list(inspect.signature(pkg.hotpath.perm_plan).parameters) == ["permutations", "contrasts", "masked", "shard"]
    assert list(inspect.signature(pkg.hotpath.missing_plan).parameters) == ["data", "missing", "valid", "shard", "contrasts", "sample_scores",
                                                                             "sample_tests", "sample_calls", "pair_support"]
    assert list(inspect.signature(pkg.hotpath.top_pairs_plan).parameters) == ["top_pairs", "masked", "shard"]


def test_top_pairs_plan_refuses_before_any_context(pkg, tmp_path):
    """No GPU here: opening a context would raise a ReoError that is no DimensionMismatch, and reoa would first miss its files"""
    plan = pkg.hotpath.top_pairs_plan
    assert plan(None) is None and plan(None, masked=True, shard=(0, 4)) is None   # nothing asked: nothing refused
    assert plan(1) is None and plan(1 << 20) is None and plan(np.int64(20)) is None
    for bad in (0, -3, (1 << 20) + 1, 2.5, "20", True):
        with pytest.raises(pkg.DimensionMismatch, match="top_pairs = .*between 1 and 2\\^20"):
            plan(bad)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs: .*validity mask"):
        plan(20, masked=True)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs: .*no sharded form \\(shard = \\(1, 2\\)\\)"):
        plan(20, shard=(1, 2))
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    X[0, 0] = np.nan
    args = (X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs: .*validity mask"):
        pkg.run_identify_degs(*args, missing="pairwise", top_pairs=20)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs: .*validity mask"):
        pkg.run_identify_degs(np.nan_to_num(X), *args[1:], valid=np.ones((6, 4), bool), top_pairs=20)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs: .*no sharded form"):
        pkg.run_identify_degs(np.nan_to_num(X), *args[1:], shard=(0, 2), top_pairs=20)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs = 0"):
        pkg.run_identify_degs(np.nan_to_num(X), *args[1:], top_pairs=0)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs = 0"):
        pkg.identify_degs_cells(np.nan_to_num(X), ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, top_pairs=0)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs = -1"):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), top_pairs=-1)
    assert os.listdir(tmp_path) == []
