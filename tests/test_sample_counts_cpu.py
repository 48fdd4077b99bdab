"""Sample counts (reo_sample_counts), the parts that need no GPU: the ABI, the vertical counters, the slot map and the host argument checks of
csrc/sample_counts.h under the sanitizers, and the Python helpers (the score algebra, the TSV writer, the sample_scores=False defaults)."""
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
    s = "reo_sample_counts"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m, s
    assert len(m.group(1).split(",")) == 8, m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 8
    assert hasattr(L, s)
    assert L.reo_version() >= 700
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header)                    # no new stage timer


def test_counters_slot_map_and_argument_checks_under_sanitizers(tmp_path):
    """tests/sample_counts_driver.cpp: sc_counter_add / sc_counter_planes / sc_counter_expand of csrc/sample_counts.h, which the kernel of
    csrc/samplecounts.hip evaluates, against per-bit integer counting for 1, 2, 63, 64, 65 and 127 additions; sc_slot_map for interleaved
    labels and groups of 1, 31, 32 and 33 samples; sample_counts_check_args, every check with its message.  AddressSanitizer and UBSan stay
    silent."""
    exe = str(tmp_path / "sample_counts_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sample_counts_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 6 * 3 * 64
    assert [l.split()[1:] for l in lines[:-1]] == [["1", "1"], ["2", "2"], ["63", "6"], ["64", "7"], ["65", "7"], ["127", "7"]]


def hand_made(pkg):
    g = np.array([5, 2], dtype=np.int32)
    c13 = pkg.SampleCounts(g, np.array([4, 0], dtype=np.int32), np.array([[4, 1, 0], [0, 0, 0]], dtype=np.int32),
                           np.array([[0, 1, 0], [0, 0, 0]], dtype=np.int32))
    c31 = pkg.SampleCounts(g, np.array([3, 2], dtype=np.int32), np.array([[0, 1, 3], [2, 0, 1]], dtype=np.int32),
                           np.array([[1, 0, 0], [0, 0, 1]], dtype=np.int32))
    return c13, c31


def test_score_algebra_on_hand_made_counts(pkg):
    c13, c31 = hand_made(pkg)
    assert c13.n_lt.tolist() == [[0, 2, 4], [0, 0, 0]] and c31.n_lt.tolist() == [[2, 2, 0], [0, 2, 0]] and c13.n_lt.dtype == np.int32
    sc = pkg._ffi.sample_scores_from(c13, c31)
    assert isinstance(sc, pkg.SampleScores) and sc.genes.tolist() == [5, 2]
    assert sc.n_pairs.tolist() == [7, 2]
    assert sc.treat_like.tolist() == [[6, 3, 0], [0, 2, 0]]                       # gt(n13) + lt(n31)
    assert sc.ctrl_like.tolist() == [[0, 3, 7], [2, 0, 1]]                        # lt(n13) + gt(n31)
    assert sc.tied.tolist() == [[1, 1, 0], [0, 0, 1]]
    assert sc.net.tolist() == [[6, 0, -7], [-2, 2, -1]] and sc.net.dtype == np.int32 and sc.net.shape == (2, 3)
    assert np.array_equal(sc.treat_like + sc.ctrl_like + sc.tied, np.broadcast_to(sc.n_pairs[:, None], (2, 3)))
    no_ties = pkg.SampleCounts(c13.genes, c13.n_sel, c13.n_gt, None)
    with pytest.raises(pkg.DimensionMismatch):
        no_ties.n_lt


def test_write_sample_scores_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E", "f"]
    sc = pkg._ffi.sample_scores_from(*hand_made(pkg))
    path = tmp_path / "s.tsv"
    pkg.write_sample_scores_tsv(str(path), names, ["ctl_1", "trt 1", "x"], sc)
    assert path.read_bytes() == (b"gene\tn_pairs\tctl_1\ttrt 1\tx\n"
                                 b"f\t7\t6\t0\t-7\n"
                                 b"geneC\t2\t-2\t2\t-1\n")
    z = np.zeros((0, 2), dtype=np.int32)
    pkg.write_sample_scores_tsv(str(path), names, ["a", "b"], pkg.SampleScores(np.zeros(0, np.int32), np.zeros(0, np.int32), z, z, z))
    assert path.read_bytes() == b"gene\tn_pairs\ta\tb\n"


def test_sample_scores_default_to_false(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["sample_scores"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert {"SampleCounts", "SampleScores", "write_sample_scores_tsv"} <= set(pkg.__all__)
    assert callable(pkg.Context.sample_counts) and callable(pkg.Context.sample_scores)
    p = inspect.signature(pkg.Context.sample_counts).parameters
    assert list(p) == ["self", "genes", "classes", "partner_mask", "ties"] and p["partner_mask"].default is None and p["ties"].default is True


def test_numpy_restatement_of_the_comparators():
    """tests/sample_counts_cases.py on values whose states are known by hand"""
    import sample_counts_cases as sc
    x = np.array([1.0, 1.05, 1.1000001, 0.0, np.inf, np.inf, -np.inf, -np.inf])
    gt, eq = sc.sample_states(x, 0)
    assert eq.tolist() == [True, True, False, False, False, False, False, False] and gt.tolist() == [False, False, False, True, False, False, True, True]
    gt, eq = sc.sample_states(x, 5)                                              # +Inf, index 5: above the equal infinity with the smaller index
    assert not eq.any() and gt.tolist() == [True, True, True, True, True, False, True, True]
    gt, eq = sc.sample_states(x, 4)
    assert not eq.any() and gt.tolist() == [True, True, True, True, False, False, True, True]
    gt, eq = sc.sample_states(x, 7)                                              # -Inf, index 7: above the -Inf of index 6 only
    assert not eq.any() and gt.tolist() == [False] * 6 + [True, False]
    xi = np.array([3, 3, 2, 4], dtype=np.int64)
    gt, eq = sc.sample_states(xi, 1)
    assert eq.tolist() == [True, True, False, False] and gt.tolist() == [False, False, True, False]
    import float32_cases as fc
    rng = np.random.default_rng(3)
    p = None
    while p is None:
        p = fc._flip_pair(rng)
    xf = np.array([p[0], p[1]], dtype=np.float32)                                # Float32 says "not tied", Float64 "tied"
    assert not sc.sample_states(xf, 0)[1][1] and sc.sample_states(xf.astype(np.float64), 0)[1][1]
    row = np.array([255, 2, 6, 4, 2], dtype=np.uint8)
    assert sc.selection(row, 0x44, [1, 1, 1, 1, 0]).tolist() == [False, True, True, False, False]
