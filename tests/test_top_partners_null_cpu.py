"""The label-permutation null of a gene's best partner score (reo_top_partners_null), the parts that need no GPU: the ABI, the shared header
csrc/top_partners_null.h under the sanitizers (tests/top_partners_null_driver.cpp), the restatement of tests/top_partners_null_cases.py
against that of the global null (identity I1), the condition that keeps the partner tie-break from being tested on nothing, the
TopPartnersNull algebra on hand-made arrays, the plan function and the writer."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import top_pairs_cases as tpc
import top_pairs_null_cases as tnc
import top_partners_null_cases as pnc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    s = "reo_top_partners_null"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    # ctx, a, b, sides, n_perm, genes, n_genes, partner_mask, cuts, max_n, arg_p, n_reach: the twelve of the declaration
    assert m and len(m.group(1).split(",")) == 12, m and m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 12
    assert hasattr(L, s) and L.reo_version() >= 1700
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    p = inspect.signature(pkg.Context.top_partners_null).parameters
    assert list(p) == ["self", "sides", "genes", "a", "b", "partner_mask", "cuts"]
    assert p["genes"].default is None and p["a"].default == 0 and p["b"].default is None and p["partner_mask"].default is None and p["cuts"].default is None
    assert pkg.TopPartnersNull._fields == ("genes", "max_num", "arg_partner", "n_reach", "cuts", "side_sizes", "a", "b")
    for method in ("p_row", "p_max", "expected_reach", "overall"):
        assert callable(getattr(pkg.TopPartnersNull, method))
    assert isinstance(pkg.TopPartnersNull.max_score, property)
    assert {"TopPartnersNull", "write_top_partners_null_tsv"} <= set(pkg.__all__)
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        q = inspect.signature(fn).parameters["top_partners_permutations"]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY, fn
    csrc = os.path.join(ROOT, "rankcompv3.jl_amd", "csrc")
    unit = open(os.path.join(csrc, "Makefile")).read()
    assert "toppartnersnull.o" in unit and re.search(r"^toppartnersnull\.o:.*top_partners_null\.h", unit, flags=re.M)
    shared = open(os.path.join(csrc, "top_partners_null.h")).read()
    assert "hip_runtime" not in shared and '#include "top_pairs_null.h"' in shared and '#include "top_partners.h"' in shared
    assert "NOT a tie-break" in shared and "single-step" in header


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_partners_null") / "top_partners_null_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "top_partners_null_driver.cpp")])
    return exe


def test_key_batch_rule_and_argument_checks_under_sanitizers(driver):
    """tests/top_partners_null_driver.cpp: every argument check with its message; key pack, unpack and order; eligibility, the cut word and
    the padded rows; the batch rule.  AddressSanitizer and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 10000


@pytest.mark.parametrize("name", pnc.NAMES)
def test_all_rows_together_are_the_global_null(name):
    """I1 on the restatements: with every gene as a query, the maximum over the rows is the global null's, and the smallest
    (min(q, p), max(q, p)) over the rows that attain it is its pair -- for all 33 label rows"""
    exp, glob = pnc.expected(name), tnc.expected(name)
    G = tpc.case(name)[0].shape[0]
    assert exp.max_num.shape == (pnc.B_MAX, G) and exp.arg_partner.shape == (pnc.B_MAX, G) and exp.n_reach.shape == (pnc.B_MAX, G)
    want = [(int(m), int(i), int(j)) for m, i, j in zip(glob.max_num, glob.arg_i, glob.arg_j)]
    assert pnc.overall(exp.max_num, exp.arg_partner, np.arange(G)) == want
    assert (exp.arg_partner != np.arange(G)[None, :]).all() and (exp.arg_partner >= 0).all() and (exp.max_num >= 0).all()
    c = pnc.cuts(name)
    assert (exp.n_reach[:, 0::5] == G - 1).all() and not exp.n_reach[:, 4::5].any()   # cut 0: every partner; 2 S_A S_B + 1: none
    assert (exp.n_reach[0, 3::5] >= 1).all() and np.array_equal(c[3::5], exp.max_num[0, 3::5])   # the observed maximum reaches itself
    if name == "level":                                                          # every |N| is 0: partner 1 for gene 0, partner 0 otherwise
        assert not exp.max_num.any() and (exp.arg_partner[:, 0] == 1).all() and not exp.arg_partner[:, 1:].any()


@pytest.mark.parametrize("name", pnc.NAMES)
def test_the_smallest_partner_rule_is_exercised(name):
    """every named case has (label row, gene) cells whose maximum more than one partner attains: there "the smallest p" decides"""
    exp = pnc.expected(name)
    cells = exp.max_num.size
    print(name, "cells with several partners at the maximum:", exp.n_multi, "of", cells)
    assert 1 <= exp.n_multi <= cells


def test_the_restatement_with_a_mask_a_query_list_and_no_partner():
    name = "count_i64"
    X = tpc.case(name)[0]
    G = X.shape[0]
    rows = tnc.rows(name)[:3]
    q = pnc.seam_queries(G)
    assert q.tolist() == [0, 63, 64, G - 1, 5, 5, 64]
    part = pnc.restate(X, rows, q, pnc.cuts(name)[q])
    full = pnc.select(pnc.expected(name), 3, q)
    assert all(np.array_equal(u, v) for u, v in zip(part[:3], full[:3]))         # a list of queries selects columns: rows are decided alone
    assert np.array_equal(part.max_num[:, 4], part.max_num[:, 5]) and np.array_equal(part.arg_partner[:, 1 + 1], part.arg_partner[:, 6])
    one = np.zeros(G, dtype=bool)
    one[5] = True
    alone = pnc.restate(X, rows, [5, 9], [0, 0], one)
    assert alone.max_num[:, 0].tolist() == [-1] * 3 and alone.arg_partner[:, 0].tolist() == [-1] * 3 and not alone.n_reach[:, 0].any()
    n = tnc.abs_num(X, rows[1])[0]
    assert (alone.arg_partner[:, 1] == 5).all() and alone.max_num[1, 1] == n[9, 5] == n[5, 9] and (alone.n_reach[:, 1] == 1).all()
    bare = pnc.restate(X, rows, [5, 9])
    assert bare.n_reach.shape == (3, 0)
    for m in (None, tpc.half_mask(G), one):                                      # the O(G S) restatement on data with ties
        c = pnc.cuts(name)[q]
        slow, fast = pnc.restate(X, rows, q, c, m), pnc.query_restate(X, rows, q, c, m)
        assert all(np.array_equal(u, v) for u, v in zip(slow[:3], fast[:3])) and slow.n_multi == fast.n_multi
    Xf = tpc.case("count_f32")[0]
    assert Xf.dtype == np.float32
    slow, fast = pnc.restate(Xf, tnc.rows("count_f32")[:2], q), pnc.query_restate(Xf, tnc.rows("count_f32")[:2], q)
    assert all(np.array_equal(u, v) for u, v in zip(slow[:3], fast[:3]))


def test_moved_restate_is_the_full_restatement_at_a_small_size():
    X, gid, genes = tpc.moved_case(200, 21)
    rows = tnc.moved_rows(gid, 3)
    q = np.array(list(genes) + [0, 64, 198], dtype=np.int32)
    cuts = np.arange(q.size, dtype=np.int64)
    full, fast = pnc.restate(X, rows, q, cuts), pnc.moved_restate(X, rows, q, cuts)
    assert all(np.array_equal(u, v) for u, v in zip(full[:3], fast[:3])) and full.n_multi == fast.n_multi
    assert (fast.max_num[:, :len(genes)] > 0).all()                              # a moved gene has partners at N != 0 under every row
    assert not fast.max_num[:, len(genes)].any() and (fast.arg_partner[:, len(genes)] == 1).all()   # gene 0 lies below every gene everywhere


def hand_made(pkg):
    """B = 4 label rows, Q = 3 query genes (5, 2, 9)"""
    return pkg.TopPartnersNull(genes=np.array([5, 2, 9], dtype=np.int32),
                               max_num=np.array([[40, 10, 8], [12, 30, 8], [27, 10, 40], [30, 5, 0]], dtype=np.int64),
                               arg_partner=np.array([[2, 5, 0], [9, 9, 1], [2, 0, 5], [0, 1, 2]], dtype=np.int32),
                               n_reach=np.array([[1, 3, 0], [0, 4, 0], [0, 3, 1], [1, 2, 0]], dtype=np.int32),
                               cuts=np.array([30, 5, 40], dtype=np.int64), side_sizes=np.array([4, 5], dtype=np.int64), a=0, b=None)


def hand_made_partners(pkg):
    """the TopPartners of the same three genes, m = 2; the last row found one partner only"""
    z = np.zeros((3, 2, 2), dtype=np.int32)
    return pkg.TopPartners(genes=np.array([5, 2, 9], dtype=np.int32), partner=np.array([[2, 7], [9, 0], [5, -1]], dtype=np.int32), n_gt=z, n_eq=z,
                           num=np.array([[40, -27], [-30, 10], [8, 0]], dtype=np.int64), rank_num=np.zeros((3, 2), np.int64),
                           n_found=np.array([2, 2, 1], dtype=np.int32), side_sizes=np.array([4, 5], dtype=np.int64), a=0, b=None)


def test_the_algebra_on_hand_made_arrays(pkg):
    null, tp = hand_made(pkg), hand_made_partners(pkg)
    assert null.max_score.dtype == np.float64 and np.array_equal(null.max_score, null.max_num / 40.0)
    # gene 5: max 40 12 27 30 -- >= 40: one, >= 27: three.  gene 2: 10 30 10 5 -- >= 30: one, >= 10: three.  gene 9: 8 8 40 0 -- >= 8: three
    assert np.array_equal(null.p_row(tp), np.array([[2, 4], [2, 4], [4, 5]]) / 5.0)
    assert null.p_row(tp)[2, 1] == 1.0                                           # a padded cell
    # the maximum over the rows: 40 30 40 30 -- >= 40: two, >= 30: four, >= 27: four, >= 10: four, >= 8: four
    assert np.array_equal(null.p_max(tp), np.array([[3, 5], [5, 5], [5, 5]]) / 5.0)
    assert (null.p_max(tp) >= null.p_row(tp)).all() and (np.diff(null.p_row(tp), axis=1) >= 0).all()
    assert np.array_equal(null.expected_reach(), np.array([2, 12, 1]) / 4.0)
    top, gi, gj = null.overall()
    # row 0: 40 by gene 5 with 2 -> (2, 5).  row 1: 30 by gene 2 with 9 -> (2, 9).  row 2: 40 by gene 9 with 5 -> (5, 9).  row 3: (0, 5)
    assert top.tolist() == [40, 30, 40, 30] and gi.tolist() == [2, 2, 5, 0] and gj.tolist() == [5, 9, 9, 5]
    assert top.dtype == np.int64 and gi.dtype == np.int32 and gj.dtype == np.int32
    assert [tuple(t) for t in zip(top.tolist(), gi.tolist(), gj.tolist())] == pnc.overall(null.max_num, null.arg_partner, null.genes)
    tie = null._replace(max_num=np.array([[40, 40, 40]], dtype=np.int64), arg_partner=np.array([[7, 9, 1]], dtype=np.int32), n_reach=null.n_reach[:1])
    assert [v.tolist() for v in tie.overall()] == [[40], [1], [9]]               # (5, 7), (2, 9), (1, 9): the smallest pair among equals
    with pytest.raises(ValueError, match="other query genes"):
        null.p_row(tp._replace(genes=np.array([5, 2, 8], dtype=np.int32)))
    with pytest.raises(ValueError, match="other query genes"):
        null.p_max(tp._replace(genes=tp.genes[:2], partner=tp.partner[:2], num=tp.num[:2], n_found=tp.n_found[:2]))
    none = pkg.TopPartnersNull(np.array([3], np.int32), np.full((2, 1), -1, np.int64), np.full((2, 1), -1, np.int32), np.zeros((2, 0), np.int32),
                               np.zeros(0, np.int64), np.array([4, 5], dtype=np.int64), 0, 1)
    assert none.expected_reach().shape == (0,) and [v.tolist() for v in none.overall()] == [[-1, -1], [-1, -1], [-1, -1]]
    empty = pkg.TopPartnersNull(np.zeros(0, np.int32), np.zeros((2, 0), np.int64), np.zeros((2, 0), np.int32), np.zeros((2, 0), np.int32),
                                np.zeros(0, np.int64), np.array([4, 5], dtype=np.int64), 0, 1)
    assert [v.tolist() for v in empty.overall()] == [[-1, -1], [-1, -1], [-1, -1]] and empty.max_score.shape == (2, 0)


def test_the_plan_and_the_cuts_of_a_run(pkg, tmp_path):
    plan = pkg.hotpath.top_partners_null_plan
    assert plan(None, None) is None and plan(3, None) is None and plan(3, 17) is None and plan(5, np.int64(1 << 20)) is None
    with pytest.raises(ValueError, match="top_partners_permutations needs top_partners"):
        plan(None, 17)
    for bad in (0, -1, (1 << 20) + 1, 2.5, "17", True):
        with pytest.raises(ValueError, match="top_partners_permutations = .*between 1 and 2\\^20"):
            plan(3, bad)
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    args = (X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)
    with pytest.raises(ValueError, match="top_partners_permutations needs top_partners"):   # before any context is opened: there is no GPU here
        pkg.run_identify_degs(*args, top_partners_permutations=10)
    with pytest.raises(ValueError, match="top_partners_permutations needs top_partners"):
        pkg.identify_degs_cells(X, ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, top_partners_permutations=10)
    with pytest.raises(ValueError, match="top_partners_permutations needs top_partners"):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), top_partners_permutations=10)
    assert os.listdir(tmp_path) == []
    cuts = pkg.hotpath.top_partners_null_cuts
    tp = hand_made_partners(pkg)
    assert cuts(tp).tolist() == [27, 10, 8] and cuts(tp).dtype == np.int64      # |num| of each row's last found partner
    assert cuts(tp._replace(n_found=np.array([1, 0, 1], dtype=np.int32))).tolist() == [40, 0, 8]


def test_write_top_partners_null_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "b", "TP53", "d", "e", "geneF", "g", "h", "i", "J9"]
    tp = hand_made_partners(pkg)
    tp = tp._replace(n_gt=np.array([[[4, 0], [1, 3]], [[0, 4], [2, 1]], [[3, 2], [0, 0]]], dtype=np.int32),
                     n_eq=np.array([[[0, 0], [0, 1]], [[0, 1], [1, 0]], [[0, 0], [0, 0]]], dtype=np.int32),
                     rank_num=np.array([[90, 70], [60, 50], [5, 0]], dtype=np.int64))
    path, plain = tmp_path / "null.tsv", tmp_path / "plain.tsv"
    pkg.write_top_partners_null_tsv(str(path), names, tp, hand_made(pkg))
    pkg.write_top_partners_tsv(str(plain), names, tp)
    assert path.read_bytes() == (b"gene\trank\tpartner\tnum\tscore\trank_num\tgt_A\teq_A\tgt_B\teq_B\tp_row\n"
                                 b"geneF\t1\tTP53\t40\t1.0\t90\t4\t0\t0\t0\t0.4\n"
                                 b"geneF\t2\th\t-27\t0.675\t70\t1\t0\t3\t1\t0.8\n"
                                 b"TP53\t1\tJ9\t-30\t0.75\t60\t0\t0\t4\t1\t0.4\n"
                                 b"TP53\t2\tA1BG\t10\t0.25\t50\t2\t1\t1\t0\t0.8\n"
                                 b"J9\t1\tgeneF\t8\t0.2\t5\t3\t0\t2\t0\t0.8\n")
    got, base = path.read_text().split("\n"), plain.read_text().split("\n")
    assert [l.split("\t")[:10] for l in got[:-1]] == [l.split("\t") for l in base[:-1]]   # the columns of write_top_partners_tsv, then p_row
