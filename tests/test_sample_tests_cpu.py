"""Sample tests (reo_sample_tests), the parts that need no GPU: the ABI, the arithmetic and the host argument checks of csrc/sample_tests.h
under the sanitizers against exact tails, and the Python helpers (the two-sided value, Benjamini-Hochberg per column, the calls, the TSV
writer, the sample_tests=False defaults)."""
import inspect
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np

import sample_tests_cases as stc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declaration hold , and ;)
    s = "reo_sample_tests"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m, s
    assert len(m.group(1).split(",")) == 11, m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 11
    assert hasattr(L, s)
    assert L.reo_version() >= 1000
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer


def test_exact_tails_against_enumeration():
    """the oracle of every other test here: the integer tails against a plain sum of C(K, x) C(N - K, n - x) / C(N, n) as fractions"""
    rng = np.random.default_rng(4)
    tables = [(0, 0, 0, 0), (3, 2, 0, 0), (0, 5, 5, 0), (5, 0, 0, 5), (1, 1, 1, 1), (7, 5, 9, 2)]
    tables += [tuple(int(v) for v in rng.integers(0, 9, size=4)) for _ in range(200)]
    for a, b, u, d in tables:
        N, K, n = a + b + u + d, a + u, u + d
        up, down, total = stc.exact_tails(a, b, u, d)
        if n == 0:
            assert (up, down, total) == (1, 1, 1)
            continue
        pmf = {x: Fraction(math.comb(K, x) * math.comb(N - K, n - x), math.comb(N, n)) for x in range(max(0, n - (N - K)), min(n, K) + 1)}
        assert sum(pmf.values()) == 1
        assert Fraction(up, total) == sum(v for x, v in pmf.items() if x >= u), (a, b, u, d)
        assert Fraction(down, total) == sum(v for x, v in pmf.items() if x <= u), (a, b, u, d)
    assert stc.exact_tails(0, 3, 3, 0)[0::2] == (1, math.comb(6, 3))              # the rarest table: 1 / C(2 J, J)
    assert stc.rel_err(0.25, 1, 4) == 0.0 and stc.rel_err(0.5, 1, 4) == 1.0
    assert stc.below_two_to(1, 2 ** 901, -900) and not stc.below_two_to(1, 2 ** 900, -900)
    assert stc.tolerance(12) < stc.tolerance(13) == stc.tolerance(70) < stc.tolerance(126) == stc.tolerance(300) < stc.tolerance(4199)


def test_tails_table_and_argument_checks_under_sanitizers(tmp_path):
    """tests/sample_tests_driver.cpp: sample_tests_check_args (every check with its message), st_batch_rows, st_table and st_tails of
    csrc/sample_tests.h, which the kernel of csrc/sampletests.hip evaluates; every read of the log-factorial table is checked to lie at an
    index <= N <= 2 (G - 1), and the table has exactly that many entries.  AddressSanitizer and UBSan stay silent.  The printed tails of
    the degenerate tables and of the seeded grid are compared with the exact ones: per background size the largest relative error is printed
    and asserted against 4 x MEASURED_REL_ERR (tests/sample_tests_cases.py); exact values below 2^-900 must come out below 2^-890."""
    exe = str(tmp_path / "sample_tests_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sample_tests_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 1500
    worst, cells, underflows = {}, {}, 0
    for line in lines[:-1]:
        f = line.split()
        assert f[0] == "tail" and len(f) == 8, line
        size, (a, b, u, d) = int(f[1]), (int(v) for v in f[2:6])
        assert a + b <= size
        got = float.fromhex(f[6]), float.fromhex(f[7])
        up, down, total = stc.exact_tails(a, b, u, d)
        if u + d == 0:
            assert got == (1.0, 1.0), line                                       # an empty J, all tied
        for g, num in zip(got, (up, down)):
            kind, v = stc.judge(g, num, total)
            if kind == "underflow":
                assert v, line
                underflows += 1
            else:
                worst[size] = max(worst.get(size, 0.0), v)
                assert v <= stc.tolerance(size), (line, v)
        cells[size] = cells.get(size, 0) + 1
    print("largest relative error by background size:", {k: f"{v:.3e}" for k, v in worst.items()}, "cells", cells, "underflows", underflows)
    assert sorted(worst) == [12, 70, 300, 4200] and min(cells.values()) > 150 and underflows >= 4
    for size, v in worst.items():                                                # the constants are the measured figures, not a guess
        assert v <= stc.MEASURED_REL_ERR[size] * stc.MARGIN


def hand_made(pkg):
    """3 genes x 4 samples; p-values far from every threshold used below (0.05 and 0.2): the nearest lies 0.01 away, the tolerance of
    the arithmetic is below 1e-10"""
    p_up = np.array([[1e-6, 0.5, 0.999, 0.04], [0.6, 0.001, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]])
    p_down = np.array([[0.9999, 0.6, 1e-5, 0.97], [0.5, 0.9995, 0.5, 0.5], [0.5, 0.5, 0.5, 0.5]])
    z = np.zeros((3, 4), dtype=np.int32)
    return pkg.SampleTests(np.array([5, 2, 9], dtype=np.int32), np.array([3, 4, 0], dtype=np.int32), np.array([2, 1, 0], dtype=np.int32), z, z, z, p_up, p_down)


def test_pval_and_calls_on_hand_made_values(pkg):
    st = hand_made(pkg)
    assert np.array_equal(st.pval, [[2e-6, 1.0, 2e-5, 0.08], [1.0, 0.002, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]])
    padj = st.padj()
    assert np.allclose(padj, [[6e-6, 1.0, 6e-5, 0.24], [1.0, 0.006, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0]], rtol=1e-12, atol=0)
    for thr in (0.05, 0.2, 1.0):                                                 # no value within the arithmetic's tolerance of a threshold
        near = np.concatenate([st.pval.ravel(), padj.ravel()])
        near = near[near != 1.0]
        assert (np.abs(near - thr) > 0.009).all()
    c = st.calls(0.2, 0.05)
    assert c.dtype == np.int8 and c.tolist() == [[1, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 0]]
    assert st.calls(0.05, 1.0).tolist() == [[1, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 0]]   # pval 0.08 misses 0.05
    assert st.calls(0.2, 1.0).tolist() == [[1, 0, -1, 1], [0, 1, 0, 0], [0, 0, 0, 0]]    # ... and passes 0.2 when padj (0.24) may be anything
    assert st.calls(1.0, 1.0).tolist() == [[1, 1, -1, 1], [-1, 1, 0, 0], [0, 0, 0, 0]]  # equal tails call nothing
    none = pkg.SampleTests(st.genes, st.n_above_ctrl, st.n_below_ctrl, None, None, None, st.p_up, st.p_down)   # counts=False
    assert np.array_equal(none.calls(0.2, 0.05), c)


def test_padj_against_the_oracles_bh_on_random_columns(pkg):
    from oracle import reo_numpy
    rng = np.random.default_rng(12)
    for rows, cols in ((1, 3), (2, 2), (17, 5), (200, 7)):
        p_up = rng.random((rows, cols)) ** 3
        p_up[rng.random((rows, cols)) < 0.1] = 0.5                               # equal values: the stable order matters
        p_down = np.minimum(1.0, 1.0 - p_up + rng.random((rows, cols)) * 0.01)
        z = np.zeros(rows, dtype=np.int32)
        st = pkg.SampleTests(z, z, z, None, None, None, p_up, p_down)
        got = st.padj()
        assert got.shape == (rows, cols) and got.dtype == np.float64
        for s in range(cols):
            assert np.array_equal(got[:, s], reo_numpy.bh(st.pval[:, s])), (rows, s)
    assert np.array_equal(pkg._ffi.bh_columns(np.zeros((0, 3))), np.zeros((0, 3)))


def test_write_sample_calls_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E", "f", "g7", "h", "i", "j"]
    st = hand_made(pkg)
    path = tmp_path / "c.tsv"
    pkg.write_sample_calls_tsv(str(path), names, ["ctl_1", "trt 1", "x", "y"], st.genes, st.calls(0.2, 0.05))
    assert path.read_bytes() == (b"gene\tctl_1\ttrt 1\tx\ty\n"
                                 b"geneC\t0\t1\t0\t0\n"
                                 b"f\t1\t0\t-1\t0\n")                            # ascending gene order (2, 5); gene 9 has no call
    pkg.write_sample_calls_tsv(str(path), names, ["a", "b"], np.zeros(0, np.int32), np.zeros((0, 2), dtype=np.int8))
    assert path.read_bytes() == b"gene\ta\tb\n"
    pkg.write_sample_calls_tsv(str(path), names, ["a", "b"], np.array([1, 0], np.int32), np.zeros((2, 2), dtype=np.int8))
    assert path.read_bytes() == b"gene\ta\tb\n"                                   # genes without a call: the header alone


def test_the_three_options_default_to_false(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["sample_tests"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert {"SampleTests", "write_sample_calls_tsv"} <= set(pkg.__all__)
    assert callable(pkg.Context.sample_tests) and callable(pkg.Context.sample_tests_raw)
    p = inspect.signature(pkg.Context.sample_tests).parameters
    assert list(p) == ["self", "genes", "partner_mask", "counts"]
    assert p["genes"].default is None and p["partner_mask"].default is None and p["counts"].default is True
    assert pkg.SampleTests._fields == ("genes", "n_above_ctrl", "n_below_ctrl", "rev_up", "rev_down", "tied", "p_up", "p_down")
    assert isinstance(pkg.SampleTests.pval, property)
