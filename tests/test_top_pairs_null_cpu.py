"""The label-permutation null of the best pair score (reo_top_pairs_null), the parts that need no GPU: the ABI, the shared header
csrc/top_pairs_null.h under the sanitizers (tests/top_pairs_null_driver.cpp), the restatement of tests/top_pairs_null_cases.py against the
oracle of the search, permuted_sides, and the TopPairsNull algebra on hand-made numbers."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import top_pairs_cases as tpc
import top_pairs_null_cases as tnc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    s = "reo_top_pairs_null"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m and len(m.group(1).split(",")) == 12, m and m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 12
    assert hasattr(L, s) and L.reo_version() >= 1400
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    assert "NOT a tie-break" in header
    p = inspect.signature(pkg.Context.top_pairs_null).parameters
    assert list(p) == ["self", "sides", "a", "b", "gene_mask", "cuts"]
    assert p["a"].default == 0 and p["b"].default is None and p["gene_mask"].default is None and p["cuts"].default is None
    assert pkg.TopPairsNull._fields == ("max_num", "arg_i", "arg_j", "n_reach", "cuts", "side_sizes", "a", "b")
    assert {"TopPairsNull", "permuted_sides", "write_top_pairs_null_tsv"} <= set(pkg.__all__)
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        q = inspect.signature(fn).parameters["top_pairs_permutations"]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY, fn
    unit = open(os.path.join(ROOT, "rankcompv3.jl_amd", "csrc", "Makefile")).read()
    assert "toppairsnull.o" in unit


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_pairs_null") / "top_pairs_null_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "top_pairs_null_driver.cpp")])
    return exe


def test_words_key_batch_rule_and_argument_checks_under_sanitizers(driver):
    """tests/top_pairs_null_driver.cpp: every argument check with its message; the A-word and the live word of rows that hold a 2; key pack,
    unpack and order; the batch rule.  AddressSanitizer and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 4000


@pytest.mark.parametrize("name", ["count_i64", "rank130", "three_0_2", "three_1_rest", "level"])
def test_the_restatement_agrees_with_the_oracle_of_the_search(name):
    """per row, the restatement's maximum is |N| of the first pair of top_pairs_cases.oracle on the relabelled groups; on the observed row
    that is the oracle of the case itself"""
    X, gid, ng, a, b = tpc.case(name)
    rows, exp = tnc.rows(name), tnc.expected(name)
    assert np.array_equal(rows[0], tnc.observed_row(gid, a, b)) and (rows[:, rows[0] == 2] == 2).all()
    assert (rows == 1).sum(axis=1).tolist() == [int((gid == a).sum())] * tnc.B_MAX
    assert exp.max_num[0] == abs(int(tpc.expected(name).num[0]))
    for p in (0, 1, 16, 32):
        o = tpc.oracle(X, tnc.relabel(rows[p]), 3, 0, 1)
        assert exp.max_num[p] == abs(int(o.num[0])), (name, p)
        top = np.abs(o.num) == exp.max_num[p]                                    # the first (i, j) among the pairs at the maximum
        assert (exp.arg_i[p], exp.arg_j[p]) == min(zip(o.gene_i[top].tolist(), o.gene_j[top].tolist())), (name, p)
    c = tnc.cuts(name)
    pairs = X.shape[0] * (X.shape[0] - 1) // 2
    assert (exp.n_reach[:, 0] == pairs).all() and not exp.n_reach[:, 5].any() and exp.n_reach[0, 3] >= 1
    assert c[3] == exp.max_num[0] and c[4] == 2 * tpc.expected(name).sizes[0] * tpc.expected(name).sizes[1]
    if name == "level":
        assert not exp.max_num.any() and not exp.arg_i.any() and (exp.arg_j == 1).all()
        assert c.tolist() == [0, 1, 0, 0, 288, 289] and (exp.n_reach[:, [0, 2, 3]] == 4950).all() and not exp.n_reach[:, [1, 4, 5]].any()


def test_the_restatement_with_a_mask_and_without_pairs():
    X, gid, ng, a, b = tpc.case("count_i64")
    rows = tnc.rows("count_i64")[:2]
    one = np.zeros(X.shape[0], dtype=bool)
    one[5] = True
    none = tnc.restate(X, rows, [0], one)
    assert none.max_num.tolist() == [-1, -1] and none.arg_i.tolist() == [-1, -1] and not none.n_reach.any()
    two = one.copy()
    two[9] = True
    pair = tnc.restate(X, rows, [0], two)
    assert pair.arg_i.tolist() == [5, 5] and pair.arg_j.tolist() == [9, 9] and pair.n_reach[:, 0].tolist() == [1, 1]
    n = tnc.abs_num(X, rows[1])[0]
    assert pair.max_num[1] == n[5, 9] == n[9, 5]


def test_moved_expected_is_the_full_restatement_at_a_small_size():
    X, gid, genes = tpc.moved_case(200, 21)
    rows = tnc.moved_rows(gid, 3)
    assert rows.shape == (3, 9) and (rows == 1).sum(axis=1).tolist() == [5, 5, 5] and len({r.tobytes() for r in rows}) == 3
    assert (rows[1] != rows[0]).sum() == 8                                       # four samples of either side changed places
    full = tnc.restate(X, rows)
    for p in range(3):
        assert tnc.moved_expected(X, rows[p], genes) == (int(full.max_num[p]), int(full.arg_i[p]), int(full.arg_j[p]))


def test_permuted_sides(pkg):
    gid = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 1, 0, 2, 1, 0])
    rows = pkg.permuted_sides(gid, 0, 2, 40, seed=5)
    assert rows.dtype == np.uint8 and rows.shape == (40, 16)
    obs = np.where(gid == 0, 1, np.where(gid == 2, 0, 2))
    assert ((rows == 2) == (obs == 2)[None, :]).all()                            # the samples of group 1 take no part, in every row
    assert ((rows == 1).sum(axis=1) == 6).all() and ((rows == 0).sum(axis=1) == 4).all()
    assert len({r.tobytes() for r in rows}) == 40 and not (rows == obs[None, :]).all(axis=1).any()
    assert np.array_equal(rows, pkg.permuted_sides(gid, 0, 2, 40, seed=5)) and not np.array_equal(rows, pkg.permuted_sides(gid, 0, 2, 40, seed=6))
    with_obs = pkg.permuted_sides(gid, 0, 2, 40, seed=5, include_observed=True)
    assert np.array_equal(with_obs[0], obs) and np.array_equal(with_obs[1:], rows[:39])
    rest = pkg.permuted_sides(gid, 1, None, 10, seed=1)                          # b None: every other sample is side B, no 2 anywhere
    assert not (rest == 2).any() and ((rest == 1).sum(axis=1) == 6).all()
    strata = np.array(list("xxyyxxyyxxyyxxyy"))
    st = pkg.permuted_sides(gid, 0, 2, 8, seed=2, strata=strata)
    for v in "xy":
        assert ((st[:, strata == v] == 1).sum(axis=1) == (obs[strata == v] == 1).sum()).all()
        assert ((st[:, strata == v] == 2) == (obs[strata == v] == 2)[None, :]).all()
    with pytest.raises(ValueError, match="fewer than 7 distinct arrangements"):
        pkg.permuted_sides(np.array([0, 1, 1, 2, 2]), 0, 1, 7)                   # one 1 among three samples: two arrangements besides the observed
    assert pkg.permuted_sides(np.array([0, 1, 1, 2, 2]), 0, 1, 2).shape == (2, 5)
    with pytest.raises(ValueError, match="nothing to permute"):
        pkg.permuted_sides(gid, 3, None, 4)
    with pytest.raises(ValueError, match="b == a"):
        pkg.permuted_sides(gid, 1, 1, 4)
    with pytest.raises(ValueError, match="strata has 3 labels"):
        pkg.permuted_sides(gid, 0, 2, 4, strata=[1, 2, 3])
    # permuted_labels itself is unchanged: one side against the rest, bytes 0 / 1
    assert np.array_equal(pkg.permuted_labels(gid, 1, 10, seed=1), rest)


def hand_made(pkg):
    return pkg.TopPairsNull(max_num=np.array([40, 12, 27, 30, 27, 8, 40], dtype=np.int64), arg_i=np.zeros(7, np.int32), arg_j=np.ones(7, np.int32),
                            n_reach=np.array([[1, 3], [0, 0], [0, 2], [0, 4], [0, 1], [0, 0], [2, 4]], dtype=np.int64),
                            cuts=np.array([40, 27], dtype=np.int64), side_sizes=np.array([4, 5], dtype=np.int64), a=0, b=None)


def test_p_max_and_expected_reach_on_hand_made_numbers(pkg):
    null = hand_made(pkg)
    assert null.max_score.dtype == np.float64 and np.array_equal(null.max_score, np.array([40, 12, 27, 30, 27, 8, 40]) / 40.0)
    z = np.zeros((4, 2), dtype=np.int32)
    tp = pkg.TopPairs(np.array([2, 0, 2, 1], np.int32), np.array([7, 2, 3, 4], np.int32), z, z, np.array([40, -30, 27, -5], dtype=np.int64),
                      np.zeros(4, np.int64), np.array([4, 5], dtype=np.int64), 0, None, 1)
    # max_num >= 40: two; >= 30: three; >= 27: five; >= 5: all seven
    assert np.array_equal(null.p_max(tp), np.array([3, 4, 6, 8]) / 8.0)
    assert (np.diff(null.p_max(tp)) >= 0).all()
    assert np.array_equal(null.expected_reach(), np.array([3 / 7, 14 / 7]))
    empty = tp._replace(gene_i=tp.gene_i[:0], gene_j=tp.gene_j[:0], num=tp.num[:0])
    assert null.p_max(empty).shape == (0,)
    none = pkg.TopPairsNull(np.array([-1, -1], np.int64), np.full(2, -1, np.int32), np.full(2, -1, np.int32), np.zeros((2, 0), np.int64),
                            np.zeros(0, np.int64), np.array([4, 5], dtype=np.int64), 0, 1)
    assert none.expected_reach().shape == (0,) and np.array_equal(none.p_max(tp), np.full(4, 1 / 3))


def test_the_plan_and_the_cuts_of_a_run(pkg, tmp_path):
    plan = pkg.hotpath.top_pairs_null_plan
    assert plan(None, None) is None and plan(20, None) is None and plan(20, 17) is None and plan(5, np.int64(1 << 20)) is None
    with pytest.raises(ValueError, match="top_pairs_permutations needs top_pairs"):
        plan(None, 17)
    for bad in (0, -1, (1 << 20) + 1, 2.5, "17", True):
        with pytest.raises(ValueError, match="top_pairs_permutations = .*between 1 and 2\\^20"):
            plan(20, bad)
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    args = (X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)
    with pytest.raises(ValueError, match="top_pairs_permutations needs top_pairs"):     # before any context is opened: there is no GPU here
        pkg.run_identify_degs(*args, top_pairs_permutations=10)
    with pytest.raises(ValueError, match="top_pairs_permutations needs top_pairs"):
        pkg.identify_degs_cells(X, ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, top_pairs_permutations=10)
    with pytest.raises(ValueError, match="top_pairs_permutations needs top_pairs"):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), top_pairs_permutations=10)
    assert os.listdir(tmp_path) == []
    z = np.zeros((150, 2), dtype=np.int32)
    num = np.arange(300, 150, -1, dtype=np.int64) * np.where(np.arange(150) % 2, -1, 1)
    tp = pkg.TopPairs(np.zeros(150, np.int32), np.ones(150, np.int32), z, z, num, np.zeros(150, np.int64), np.array([4, 5], dtype=np.int64), 0, None, 1)
    cuts = pkg.hotpath.top_pairs_null_cuts
    assert cuts(tp).tolist() == [300, 291, 201, 151] and cuts(tp).dtype == np.int64   # entries 1, 10, 100 and K
    short = tp._replace(num=num[:10])
    assert cuts(short).tolist() == [300, 291] and cuts(tp._replace(num=num[:1])).tolist() == [300] and cuts(tp._replace(num=num[:0])).size == 0


def test_write_top_pairs_null_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E", "f", "g", "h"]
    tp = pkg.TopPairs(gene_i=np.array([2, 0], dtype=np.int32), gene_j=np.array([7, 2], dtype=np.int32),
                      n_gt=np.array([[4, 0], [0, 4]], dtype=np.int32), n_eq=np.array([[0, 0], [0, 1]], dtype=np.int32),
                      num=np.array([40, -30], dtype=np.int64), rank_num=np.array([90, 70], dtype=np.int64),
                      side_sizes=np.array([4, 5], dtype=np.int64), a=0, b=None, passes=2)
    path = tmp_path / "t.tsv"
    pkg.write_top_pairs_null_tsv(str(path), names, tp, hand_made(pkg))
    assert path.read_bytes() == (b"gene_i\tgene_j\tdirection\tscore\trank_score\tgt_A\teq_A\tgt_B\teq_B\tp_max\n"
                                 b"geneC\th\t1\t1.0\t2.25\t4\t0\t0\t0\t0.375\n"
                                 b"A1BG\tgeneC\t-1\t0.75\t1.75\t0\t0\t4\t1\t0.5\n")
