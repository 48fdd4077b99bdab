"""Sample calls (reo_sample_calls), the parts that need no GPU: the ABI, the arithmetic and the host argument checks of
csrc/sample_calls.h under the sanitizers, the whole rule (rank, histogram, cut, call) on seeded columns against SampleTests.calls, and the
sample_calls=False defaults."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np

import sample_calls_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declaration hold , and ;)
    s = "reo_sample_calls"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m, s
    assert len(m.group(1).split(",")) == 10, m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 10
    assert hasattr(L, s)
    assert L.reo_version() >= 1100
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    shared = open(os.path.join(ROOT, "rankcompv3.jl_amd", "csrc", "sample_calls.h")).read()
    assert int(re.search(r"constexpr int kCallBins = (\d+);", shared).group(1)) == pkg._ffi.CALL_BINS   # the mirror of the tile size


def test_rule_words_cuts_and_argument_checks_under_sanitizers(pkg, tmp_path):
    """tests/sample_calls_driver.cpp: sample_calls_check_args (every check with its message, and their order), the batch and memory
    arithmetic, call_bh_rank against a plain search over a grid that holds every rounding boundary at n = 200, the word's pack and unpack,
    call_cut on hand-made histograms.  AddressSanitizer and UBSan stay silent.  The whole rule on the printed columns (all equal, all 0,
    all 1, the boundary columns, random^3 with ties; n in {1, 2, 17, 200, 5000}) equals SampleTests.calls and the count of padj <= padj_deg
    for the sixteen threshold pairs: an equality, both sides evaluate p * (n / r)."""
    exe = str(tmp_path / "sample_calls_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sample_calls_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 5000
    columns, seen, it = {}, set(), iter(lines[:-1])
    sign = {"+": 1, "-": -1, "0": 0}
    sizes, called, cuts_met = set(), 0, set()
    for line in it:
        f = line.split()
        if f[0] == "column":
            cid, n = int(f[1]), int(f[2])
            rows = [next(it).split() for _ in range(n)]
            assert all(r[0] == "p" and len(r) == 3 for r in rows)
            up = np.array([[float.fromhex(r[1])] for r in rows])
            down = np.array([[float.fromhex(r[2])] for r in rows])
            z = np.zeros(n, dtype=np.int32)
            columns[cid] = pkg.SampleTests(z, z, z, None, None, None, up, down)
            sizes.add(n)
            continue
        assert f[0] == "calls" and len(f) == 8, line[:80]
        cid, a, b = int(f[1]), float.fromhex(f[2]), float.fromhex(f[3])
        st = columns[cid]
        calls, cut, n_up, n_down = cc.expected(st, a, b)
        got = np.array([sign[ch] for ch in f[7]], dtype=np.int8)
        assert got.shape == (st.p_up.shape[0],) and np.array_equal(got, calls[:, 0]), (cid, a, b, np.flatnonzero(got != calls[:, 0])[:5])
        assert (int(f[4]), int(f[5]), int(f[6])) == (int(cut[0]), int(n_up[0]), int(n_down[0])), (cid, a, b, f[4:7], cut, n_up, n_down)
        seen.add((cid, a, b))
        called += int(n_up[0]) + int(n_down[0])
        cuts_met.add((st.p_up.shape[0], int(cut[0])))
    assert sizes == {1, 2, 17, 200, 5000} and len(columns) == 30
    assert len(seen) == 30 * 16 and {(a, b) for _, a, b in seen} == {(a, b) for a in cc.THRESHOLDS for b in cc.THRESHOLDS}
    assert called > 10000
    assert any(0 < k < n for n, k in cuts_met) and any(k == n for n, k in cuts_met) and any(k == 0 for n, k in cuts_met)   # cuts inside, at either end


def test_the_three_options_default_to_false(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["sample_calls"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert {"SampleCalls", "SampleTests", "write_sample_calls_tsv"} <= set(pkg.__all__)
    assert callable(pkg.Context.sample_calls) and callable(pkg.Context.sample_calls_raw)
    p = inspect.signature(pkg.Context.sample_calls).parameters
    assert list(p) == ["self", "pval_deg", "padj_deg", "genes", "partner_mask"]
    assert p["genes"].default is None and p["partner_mask"].default is None
    assert pkg.SampleCalls._fields == ("genes", "calls", "cut", "n_up", "n_down") == cc.FIELDS
    assert pkg._ffi.CALL_BINS >= 1024 and pkg._ffi.CALL_BINS % 256 == 0


def test_write_extras_writes_one_calls_file_from_the_device_calls(pkg, tmp_path):
    """write_extras (reoa's writer of the optional files) on hand-made comparison dicts: "sample_calls" alone and together with
    "sample_tests" give one file, from the SampleCalls; "sample_tests" alone gives today's file; neither gives none"""
    from types import SimpleNamespace
    names, samples = ["A1BG", "TP53", "geneC"], ["s1", "s2"]
    prep = {"g_name": ["g1", "g2"], "gene_names": names, "sample_names": samples}
    genes = np.arange(3, dtype=np.int32)
    z = np.zeros(2, dtype=np.int32)
    dev = pkg.SampleCalls(genes, np.array([[1, 0], [0, 0], [0, -1]], dtype=np.int8), z, z, z)
    p_up = np.array([[1e-9, 0.5], [0.5, 0.5], [1e-9, 0.5]])
    host = pkg.SampleTests(genes, z[:1].repeat(3), z[:1].repeat(3), None, None, None, p_up, 1.0 - p_up)
    from_dev = b"gene\ts1\ts2\nA1BG\t1\t0\ngeneC\t0\t-1\n"
    from_host = b"gene\ts1\ts2\nA1BG\t1\t0\ngeneC\t1\t0\n"
    for i, (cm, want) in enumerate((({"sample_calls": dev}, from_dev), ({"sample_calls": dev, "sample_tests": host}, from_dev),
                                    ({"sample_tests": host}, from_host), ({}, None))):
        d = tmp_path / str(i)
        d.mkdir()
        run = SimpleNamespace(comparisons=[dict(cm, k=0)], levels=["g1", "g2"])
        out = sys.modules[pkg.__name__ + ".reoa"].write_extras("stem", prep, run, str(d), 1.0, 0.05)   # (pkg.reoa is the function)
        files = sorted(p.name for p in d.iterdir())
        if want is None:
            assert out == [] and files == []
        else:
            assert len(out) == 1 and len(files) == 1 and files[0].endswith("_sample_calls.tsv"), files
            assert (d / files[0]).read_bytes() == want
