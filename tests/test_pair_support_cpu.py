"""Pair support (reo_pair_support), the parts that need no GPU: the ABI, the work items, batches, byte expansion and host argument checks of
csrc/pair_support.h under the sanitizers, and the Python helpers (the PairSupport algebra, the TSV writer, the pair_support=False defaults,
the refusal of pair_support=True without pairs)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declaration hold , and ;)
    s = "reo_pair_support"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m, s
    assert len(m.group(1).split(",")) == 8, m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 8
    assert hasattr(L, s)
    assert L.reo_version() >= 800
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer


def test_items_batches_bytes_and_argument_checks_under_sanitizers(tmp_path):
    """tests/pair_support_driver.cpp: pair_support_check_args, every check with its message; ps_build_items for rows of 0, 1, 63, 64, 65, 128
    and 129 entries, empty rows between full ones and batch cuts inside a row; ps_batch_entries; ps_outcome_byte / ps_outcome_expand, which
    the kernel of csrc/pairsupport.hip evaluates.  AddressSanitizer and UBSan stay silent."""
    exe = str(tmp_path / "pair_support_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "pair_support_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 200 * 32 + 450
    # a row of n entries is ceil(n / 64) work items
    assert [l.split()[1:] for l in lines[:-1]] == [["0", "0"], ["1", "1"], ["63", "1"], ["64", "1"], ["65", "2"], ["128", "2"], ["129", "3"]]


def hand_made(pkg, ties=True):
    n_eq = np.array([[0, 1], [1, 0], [0, 0]], dtype=np.int32) if ties else None
    return pkg.PairSupport(genes=np.array([5, 2], dtype=np.int32), rowptr=np.array([0, 2, 3], dtype=np.int64),
                           partner=np.array([7, 1, 9], dtype=np.int32), code=np.array([2, 6, 2], dtype=np.uint8),
                           n_gt=np.array([[4, 0], [1, 5], [2, 3]], dtype=np.int32), n_eq=n_eq, outcome=None,
                           group_sizes=np.array([4, 6], dtype=np.int64))


def test_pair_support_algebra_on_hand_made_counts(pkg):
    ps = hand_made(pkg)
    assert ps.n_lt.tolist() == [[0, 5], [2, 1], [2, 3]] and ps.n_lt.dtype == np.int32
    assert ps.frac_gt.dtype == np.float64 and np.array_equal(ps.frac_gt, np.array([[1.0, 0.0], [0.25, 5 / 6], [0.5, 0.5]]))
    assert np.array_equal(ps.delta(), np.array([1.0, 0.25 - 5 / 6, 0.0])) and np.array_equal(ps.delta(0), ps.delta())
    assert np.array_equal(ps.delta(1), -ps.delta(0))                             # two groups: the other side is the other group
    part, gt, eq = ps.row(0)
    assert part.tolist() == [7, 1] and gt.tolist() == [[4, 0], [1, 5]] and eq.tolist() == [[0, 1], [1, 0]]
    assert ps.row(1)[0].tolist() == [9]
    with pytest.raises(pkg.DimensionMismatch):
        ps.delta(2)
    no_ties = hand_made(pkg, ties=False)
    assert no_ties.row(0)[2] is None and np.array_equal(no_ties.delta(), ps.delta())
    with pytest.raises(pkg.DimensionMismatch, match="ties=True"):
        no_ties.n_lt
    # three groups: group k against ALL other samples, what reo_build_pairs(k) compares
    p3 = pkg.PairSupport(np.array([0], dtype=np.int32), np.array([0, 1], dtype=np.int64), np.array([1], dtype=np.int32), None,
                         np.array([[2, 3, 0]], dtype=np.int32), None, None, np.array([2, 3, 5], dtype=np.int64))
    assert p3.delta(0).tolist() == [1.0 - 3 / 8] and p3.delta(1).tolist() == [1.0 - 2 / 7] and p3.delta(2).tolist() == [0.0 - 5 / 5]


def test_top_breaks_equal_deltas_by_gene_then_partner(pkg):
    ps = pkg.PairSupport(genes=np.array([3, 1, 3], dtype=np.int32), rowptr=np.array([0, 2, 3, 5], dtype=np.int64),
                         partner=np.array([9, 4, 8, 4, 2], dtype=np.int32), code=None,
                         n_gt=np.array([[2, 0], [0, 2], [2, 0], [1, 1], [0, 2]], dtype=np.int32), n_eq=None, outcome=None,
                         group_sizes=np.array([2, 2], dtype=np.int64))
    assert ps.delta().tolist() == [1.0, -1.0, 1.0, 0.0, -1.0]
    # |delta| = 1 for (3, 9), (3, 4), (1, 8), (3, 2): ascending (gene, partner); the sign plays no part
    assert ps.top(10).tolist() == [2, 4, 1, 0, 3]
    assert ps.top(3).tolist() == [2, 4, 1] and ps.top(0).tolist() == [] and ps.top(3, k=1).tolist() == [2, 4, 1]
    ps2 = ps._replace(n_gt=np.array([[2, 0], [0, 2], [1, 0], [1, 1], [0, 2]], dtype=np.int32))
    assert ps2.top(2).tolist() == [4, 1] and ps2.top(5).tolist() == [4, 1, 0, 2, 3]   # a larger |delta| goes first whatever its gene


def test_write_pair_support_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E", "f", "g", "h", "i", "j"]
    path = tmp_path / "s.tsv"
    pkg.write_pair_support_tsv(str(path), names, ["ctl", "trt 1"], hand_made(pkg))
    assert path.read_bytes() == (b"gene\tpartner\tclass\tctl_gt\tctl_eq\ttrt 1_gt\ttrt 1_eq\n"
                                 b"f\th\tn13\t4\t0\t0\t1\n"
                                 b"f\tTP53\tn31\t1\t1\t5\t0\n"
                                 b"geneC\tj\tn13\t2\t0\t3\t0\n")
    p3 = pkg.PairSupport(np.array([4, 0, 4], dtype=np.int32), np.array([0, 1, 1, 2], dtype=np.int64), np.array([1, 3], dtype=np.int32),
                         np.array([8, 0], dtype=np.uint8), np.array([[2, 3, 0], [7, 8, 9]], dtype=np.int32),
                         np.array([[0, 0, 5], [1, 0, 0]], dtype=np.int32), None, np.array([2, 3, 5], dtype=np.int64))
    pkg.write_pair_support_tsv(str(path), names, ["a", "b", "c"], p3)
    assert path.read_bytes() == (b"gene\tpartner\tclass\ta_gt\ta_eq\tb_gt\tb_eq\tc_gt\tc_eq\n"
                                 b"E\tTP53\tn33\t2\t0\t3\t0\t0\t5\n"
                                 b"E\td\tn11\t7\t1\t8\t0\t9\t0\n")
    z = np.zeros((0, 2), dtype=np.int32)
    empty = pkg.PairSupport(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint8), z, z, None,
                            np.array([3, 3], dtype=np.int64))
    pkg.write_pair_support_tsv(str(path), names, ["a", "b"], empty)
    assert path.read_bytes() == b"gene\tpartner\tclass\ta_gt\ta_eq\tb_gt\tb_eq\n"
    with pytest.raises(pkg.DimensionMismatch):
        pkg.write_pair_support_tsv(str(path), names, ["ctl", "trt"], hand_made(pkg, ties=False))


def test_pair_support_defaults_to_false_and_is_keyword_only(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["pair_support"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert {"PairSupport", "write_pair_support_tsv", "PairList"} <= set(pkg.__all__)
    assert pkg.PairList._fields == ("genes", "rowptr", "partner", "code")       # PairList stays as it is
    assert pkg.PairSupport._fields == ("genes", "rowptr", "partner", "code", "n_gt", "n_eq", "outcome", "group_sizes")
    p = inspect.signature(pkg.Context.pair_support).parameters
    assert list(p) == ["self", "pairs", "ties", "outcomes"] and p["ties"].default is True and p["outcomes"].default is False


def test_pair_support_without_pairs_is_refused_before_any_context(pkg, tmp_path):
    """No GPU here: opening a context would raise a ReoError that is no DimensionMismatch, and reoa would first miss its files"""
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    msg = "pair_support=True needs `pairs`"
    with pytest.raises(pkg.DimensionMismatch, match=msg):
        pkg.run_identify_degs(X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1, pair_support=True)
    with pytest.raises(pkg.DimensionMismatch, match=msg):
        pkg.identify_degs_cells(X, ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, pair_support=True)
    with pytest.raises(pkg.DimensionMismatch, match=msg):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), pair_support=True)
    assert os.listdir(tmp_path) == []
