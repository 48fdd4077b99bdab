"""Pair lists (reo_get_ref_mask, reo_pair_list), the parts that need no GPU: the ABI, the selected-pair word and the host argument checks of
csrc/pair_list.h under the sanitizers, and the Python helpers (class selections, the TSV writer, the pairs=None defaults)."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"reo_get_ref_mask": 3, "reo_pair_list": 9}    # arguments of each entry


def test_header_declares_and_library_exports_the_two_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    L = pkg._ffi.lib()
    for s, nargs in ENTRIES.items():
        assert s in header
        m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == nargs
        assert hasattr(L, s), s
    assert L.reo_version() >= 600


def test_select_word_and_argument_checks_under_sanitizers(tmp_path):
    """tests/pair_list_driver.cpp: pair_select_word / pair_valid_word / pair_code_at of csrc/pair_list.h, which both kernels of
    csrc/pairlist.hip evaluate, against a per-bit decode: all 511 class masks, G = 33, 64, 65, 127 (last-word tails), the diagonal in the
    first, a middle and the last bit of a word -- and pair_list_check_args, every check with its message.  AddressSanitizer and UBSan
    stay silent."""
    exe = str(tmp_path / "pair_list_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "pair_list_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 4 * 5 * 511 * 8
    assert [l.split()[1] for l in lines[:-1]] == ["33", "64", "65", "127"]
    assert all(int(l.split()[2]) > 0 for l in lines[:-1])


def test_class_selection_parsing(pkg):
    cm = pkg._ffi.class_mask
    assert tuple(pkg.HEADER[2:11]) == pkg._ffi.CLASS_NAMES
    assert cm("reversed") == 0x44 == cm(["n13", "n31"]) == cm([2, 6]) == cm(0x44) == cm(("n13", 6))
    assert cm("n11") == 1 and cm("n33") == 0x100 and cm(["n22"]) == 0x10
    assert cm(pkg.HEADER[2:11]) == 0x1FF == cm(range(9)) == cm(0x1FF)
    assert cm(np.int64(5)) == 5 and cm([np.int32(8)]) == 0x100
    assert cm(["reversed", "n22"]) == 0x54
    assert cm(c for c in ("n12",)) == 2                                          # any iterable
    for bad in (0, 0x200, -1, [], "n14", "pval", ["n11", 9], [-1], None, True, [1.5], [True]):
        with pytest.raises(pkg.DimensionMismatch):
            cm(bad)


def test_write_pairs_tsv_byte_for_byte(pkg, tmp_path):
    names = ["A1BG", "TP53", "geneC", "d", "E"]
    pl = pkg.PairList(genes=np.array([3, 0, 3], dtype=np.int32), rowptr=np.array([0, 2, 2, 5], dtype=np.int64),
                      partner=np.array([1, 4, 0, 1, 2], dtype=np.int32), code=np.array([2, 6, 6, 2, 4], dtype=np.uint8))
    path = tmp_path / "p.tsv"
    pkg.write_pairs_tsv(str(path), names, pl)
    assert path.read_bytes() == (b"gene\tpartner\tclass\n"
                                 b"d\tTP53\tn13\n" b"d\tE\tn31\n"
                                 b"d\tA1BG\tn31\n" b"d\tTP53\tn13\n" b"d\tgeneC\tn22\n")
    part, code = pl.row(2)
    assert part.tolist() == [0, 1, 2] and code.tolist() == [6, 2, 4] and pl.row(1)[0].size == 0


def test_pairs_default_to_none(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["pairs"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert "PairList" in pkg.__all__ and "write_pairs_tsv" in pkg.__all__
    assert callable(pkg.Context.ref_mask) and callable(pkg.Context.pair_list)
