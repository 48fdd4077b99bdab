"""Leave-one-out cross-validation of the k-TSP selection (reo_top_pairs_loo), the parts that need no GPU: the ABI, the shared header
csrc/top_pairs_loo.h under the sanitizers (tests/top_pairs_loo_driver.cpp), the bound that makes the candidate route exact -- the candidate
restatement of tests/top_pairs_loo_cases.py against the all-pairs one --, the TopPairsLoo algebra on hand-made arrays, the plan function and
the two writers."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import top_pairs_cases as tpc
import top_pairs_loo_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    s = "reo_top_pairs_loo"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m and len(m.group(1).split(",")) == 12, m and m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 12
    assert hasattr(L, s) and L.reo_version() >= 1500
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    p = inspect.signature(pkg.Context.top_pairs_loo).parameters
    assert list(p) == ["self", "kmax", "a", "b", "gene_mask"]
    assert p["a"].default == 0 and p["b"].default is None and p["gene_mask"].default is None
    assert pkg.TopPairsLoo._fields == ("gene_i", "gene_j", "num", "rank_num", "outcome", "side", "side_sizes", "a", "b", "cut", "n_candidates")
    for method in ("votes", "predictions", "errors", "error_rate", "best_k", "pair_frequency"):
        assert callable(getattr(pkg.TopPairsLoo, method))
    assert {"TopPairsLoo", "write_top_pairs_cv_tsv", "write_top_pairs_loo_tsv"} <= set(pkg.__all__)
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        q = inspect.signature(fn).parameters["top_pairs_loo"]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY, fn
    csrc = os.path.join(ROOT, "rankcompv3.jl_amd", "csrc")
    unit = open(os.path.join(csrc, "Makefile")).read()
    assert "toppairsloo.o" in unit and re.search(r"^toppairsloo\.o:.*top_pairs_loo\.h", unit, flags=re.M)
    shared = open(os.path.join(csrc, "top_pairs_loo.h")).read()
    assert "hip_runtime" not in shared and "blocks at most two" in shared       # plain C++, and the argument of the bound is written down


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_pairs_loo") / "top_pairs_loo_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "top_pairs_loo_driver.cpp")])
    return exe


def test_fold_arithmetic_rules_and_argument_checks_under_sanitizers(driver):
    """tests/top_pairs_loo_driver.cpp: the fold's N and D against a recount without the sample, the order against the packed key of the
    search, the cut, the walk, the capacity rule and every argument check with its message.  AddressSanitizer and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 5000


# case -> (cut T, candidates) at kmax = 5: small bands except where thousands of pairs share the top score or every score is 0
BANDS = {"float300": (1414, 130), "count_i64": (440, 422), "separated": (1914, 8400), "three_0_2": (156, 540), "three_1_rest": (1234, 259),
         "level": (0, 4950)}


@pytest.mark.parametrize("kmax", [1, 5])
@pytest.mark.parametrize("name", lc.CASES)
def test_the_candidates_hold_every_pick_of_every_fold(name, kmax):
    """the bound, pinned: the greedy walk over the pairs with full-data |N| >= T equals the greedy walk over all pairs, in every fold"""
    every, band = lc.expected(name, kmax), lc.expected_candidates(name, kmax)
    assert lc.same(every, band), name
    X, gid, ng, a, b = tpc.case(name)
    side = lc.sides_of(gid, ng, a, b)
    assert np.array_equal(every.side, side) and int((side != 2).sum()) == sum(tpc.expected(name).sizes)
    assert (every.gene_i[side == 2] == -1).all() and (every.gene_i[side != 2] >= 0).all()   # these cases have kmax disjoint pairs in every fold
    if kmax == 5 and name in BANDS:
        assert (band.cut, band.n_candidates) == BANDS[name]
    for s in np.flatnonzero(side != 2):                                          # a fold's picks are disjoint and ordered by the fold's own key
        genes = np.concatenate([every.gene_i[s], every.gene_j[s]])
        assert np.unique(genes).size == 2 * kmax
        assert (np.diff(np.abs(every.num[s])) <= 0).all()


def test_the_restatement_is_the_definition_on_one_fold():
    """fold 0 of count_i64 by hand: drop the column, two groups, the oracle of the search"""
    X, gid, ng, a, b = tpc.case("count_i64")
    exp = lc.expected("count_i64", 5)
    cols = np.arange(1, X.shape[1])
    o = tpc.oracle(np.asfortranarray(X[:, cols]), gid[cols], 2, 0, None)
    at = lc.greedy(o, 5)
    assert np.array_equal(exp.gene_i[0], o.gene_i[at]) and np.array_equal(exp.gene_j[0], o.gene_j[at])
    assert np.array_equal(exp.num[0], o.num[at]) and np.array_equal(exp.rank_num[0], o.rank_num[at])
    assert np.array_equal(exp.outcome[0], np.sign(X[o.gene_i[at], 0] - X[o.gene_j[at], 0]).astype(np.int8))   # (integers: ties by equality)
    assert (lc.expected("count_i64", 5).outcome == 0).any()                       # the count cases have tied held-out samples among the picks


def hand_made(pkg):
    """five samples (A A B B neither), kmax 3"""
    gi = np.array([[2, 0, 5], [2, 0, 5], [2, 1, -1], [0, 2, 5], [-1, -1, -1]], dtype=np.int32)
    gj = np.array([[7, 3, 6], [7, 3, 6], [7, 4, -1], [3, 7, 6], [-1, -1, -1]], dtype=np.int32)
    num = np.array([[40, -30, 20], [40, -30, 20], [35, 30, 0], [-38, 36, 0], [0, 0, 0]], dtype=np.int64)
    out = np.array([[1, 1, 0], [-1, 0, 1], [-1, 1, 0], [-1, -1, 1], [0, 0, 0]], dtype=np.int8)
    return pkg.TopPairsLoo(gi, gj, num, np.abs(num) * 3, out, np.array([1, 1, 0, 0, 2], dtype=np.int8), np.array([2, 2], dtype=np.int64), 0, 1, 12, 77)


def test_the_algebra_on_hand_made_arrays(pkg):
    loo = hand_made(pkg)
    v = loo.votes()
    # sign(num) * outcome: [1 -1 0] [-1 0 1] [-1 1 0] [1 -1 0] [0 0 0], summed along k
    assert v.dtype == np.int32 and v.tolist() == [[1, 0, 0], [-1, -1, 0], [-1, 0, 0], [1, 0, 0], [0, 0, 0]]
    assert loo.predictions(1).dtype == np.int8 and loo.predictions(1).tolist() == [1, -1, -1, 1, 0]
    assert loo.predictions(2).tolist() == [0, -1, 0, 0, 0]                        # tied votes are undecided; the sample of neither side stays 0
    e = loo.errors()
    assert e["n_folds"].tolist() == [4, 4, 4] and e["n_wrong"].tolist() == [2, 1, 0] and e["n_undecided"].tolist() == [0, 3, 4]
    assert all(x.dtype == np.int64 for x in e.values())
    assert np.array_equal(loo.error_rate(), np.array([0.5, 1.0, 1.0])) and loo.error_rate(1) == 0.5 and loo.error_rate(3) == 1.0
    assert loo.best_k() == 1 and loo.best_k(odd=False) == 1
    level = loo._replace(outcome=np.zeros_like(loo.outcome))                      # equal rates everywhere: the smallest k
    assert level.error_rate().tolist() == [1.0, 1.0, 1.0] and level.best_k() == 1 and level.best_k(odd=False) == 1
    late = loo._replace(num=np.array([[40, 30, 20]] * 5, dtype=np.int64),
                        outcome=np.array([[0, 1, 1], [0, 1, 1], [0, -1, -1], [0, -1, -1], [0, 0, 0]], dtype=np.int8))
    assert late.error_rate().tolist() == [1.0, 0.0, 0.0] and late.best_k(odd=False) == 2 and late.best_k() == 3   # odd k only: 3, not 2
    fi, fj, fc = loo.pair_frequency(1)
    assert (fi.tolist(), fj.tolist(), fc.tolist()) == ([2, 0], [7, 3], [3, 1]) and fc.dtype == np.int64 and fi.dtype == np.int32
    fi, fj, fc = loo.pair_frequency(3)                                           # count descending, then (i, j); the -1 rows are no pairs
    assert (fi.tolist(), fj.tolist(), fc.tolist()) == ([2, 0, 5, 1], [7, 3, 6, 4], [4, 3, 3, 1])
    none = loo._replace(gene_i=np.full((5, 3), -1, np.int32), gene_j=np.full((5, 3), -1, np.int32))
    assert [x.size for x in none.pair_frequency(2)] == [0, 0, 0]
    for bad in (0, 4):
        with pytest.raises(pkg.DimensionMismatch, match="between 1 and kmax = 3"):
            loo.predictions(bad)
        with pytest.raises(pkg.DimensionMismatch, match="between 1 and kmax = 3"):
            loo.pair_frequency(bad)
        with pytest.raises(pkg.DimensionMismatch, match="between 1 and kmax = 3"):
            loo.error_rate(bad)


def test_the_plan_refuses_before_a_context_is_opened(pkg, tmp_path):
    plan = pkg.hotpath.top_pairs_loo_plan
    assert plan(None) is None and plan(1) is None and plan(np.int64(64)) is None and plan(None, masked=True, shard=(0, 2)) is None
    for bad in (0, -1, 65, 2.5, "3", True):
        with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo = .*between 1 and 64"):
            plan(bad)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo: .*validity mask"):
        plan(3, masked=True)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo: the search has no sharded form"):
        plan(3, shard=(1, 2))
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    args = (X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo = 65"):       # before any context is opened: there is no GPU here
        pkg.run_identify_degs(*args, top_pairs_loo=65)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo: .*validity mask"):
        pkg.run_identify_degs(*args, top_pairs_loo=3, valid=np.ones((6, 4), dtype=bool))
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo: .*validity mask"):
        pkg.run_identify_degs(*args, top_pairs_loo=3, missing="pairwise")
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo: the search has no sharded form"):
        pkg.run_identify_degs(*args, top_pairs_loo=3, shard=(0, 2))
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo = 0"):
        pkg.identify_degs_cells(X, ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, top_pairs_loo=0)
    with pytest.raises(pkg.DimensionMismatch, match="top_pairs_loo = 0"):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), top_pairs_loo=0)
    assert os.listdir(tmp_path) == []


def test_the_two_writers_byte_for_byte(pkg, tmp_path):
    loo = hand_made(pkg)
    cv, folds = tmp_path / "cv.tsv", tmp_path / "loo.tsv"
    pkg.write_top_pairs_cv_tsv(str(cv), loo)
    assert cv.read_bytes() == b"k\tn_folds\tn_wrong\tn_undecided\terror\n1\t4\t2\t0\t0.5\n2\t4\t1\t3\t1.0\n3\t4\t0\t4\t1.0\n"
    pkg.write_top_pairs_loo_tsv(str(folds), ["s1", "s2", "s3", "s4", "s5"], loo)
    assert folds.read_bytes() == (b"sample\tside\tvotes_1\tvotes_2\tvotes_3\n"
                                  b"s1\tA\t1\t0\t0\ns2\tA\t-1\t-1\t0\ns3\tB\t-1\t0\t0\ns4\tB\t1\t0\t0\n")
