"""Row-major host matrices (reo_set_matrix_rm_*), the parts that need no GPU: the ABI, the routing of _ffi.host_matrix_entry and the
host-side row readers of csrc/upload_rows.h under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RM = ["reo_set_matrix_rm_f64", "reo_set_matrix_rm_i64", "reo_set_matrix_rm_f32", "reo_set_matrix_rm_i32"]
NATIVE = {"f64": np.float64, "i64": np.int64, "f32": np.float32, "i32": np.int32}


def test_header_declares_and_library_exports_the_row_major_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    L = pkg._ffi.lib()
    for s in RM:
        assert re.search(r"int32_t\s+" + s + r"\s*\(reo_ctx \*ctx, const \w+\s*\*X, int64_t G, int64_t S, int64_t ld\);", header), s
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES
        assert hasattr(L, s)
    assert "LAYOUT." in header
    assert L.reo_version() >= 300


@pytest.mark.parametrize("name", sorted(NATIVE))
def test_c_contiguous_native_arrays_are_handed_over_in_place(pkg, name, monkeypatch):
    monkeypatch.setenv("REO_ROWMAJOR", "1")
    G, S = 7, 5
    X = np.arange(G * S).reshape(G, S).astype(NATIVE[name])
    assert X.flags.c_contiguous
    sym, A, ld = pkg._ffi.host_matrix_entry(X)
    assert sym == "reo_set_matrix_rm_" + name
    assert A.ctypes.data == X.ctypes.data and np.shares_memory(A, X) and A.shape == (G, S)
    assert ld == S
    # a column slice of a wider C-ordered array: the pitch is the wide array's row, no copy
    wide = np.arange(G * 23).reshape(G, 23).astype(NATIVE[name])
    V = wide[:, 5:5 + S]
    sym, A, ld = pkg._ffi.host_matrix_entry(V)
    assert sym == "reo_set_matrix_rm_" + name and ld == wide.shape[1]
    assert A.ctypes.data == V.ctypes.data and np.shares_memory(A, wide)


def _same_route(pkg, X):
    a, b = pkg._ffi.host_matrix_entry(X), pkg._ffi.matrix_entry(X)
    assert a[0] == b[0] and a[2] == b[2] and not a[0].startswith("reo_set_matrix_rm_")
    assert a[1].shape == b[1].shape and a[1].dtype == b[1].dtype and a[1].strides == b[1].strides and np.array_equal(a[1], b[1])
    return a, b


@pytest.mark.parametrize("name", sorted(NATIVE))
def test_column_major_arrays_keep_their_route(pkg, name, monkeypatch):
    monkeypatch.setenv("REO_ROWMAJOR", "1")
    G, S = 7, 5
    F = np.asfortranarray(np.arange(G * S).reshape(G, S).astype(NATIVE[name]))
    a, _ = _same_route(pkg, F)
    assert a[1].ctypes.data == F.ctypes.data and a[2] == G                      # in place, as before
    tall = np.asfortranarray(np.arange((G + 6) * S).reshape(G + 6, S).astype(NATIVE[name]))
    V = tall[2:2 + G, :]                                                        # a row slice of a taller F-ordered array: ld = G + 6
    a, _ = _same_route(pkg, V)
    assert a[1].ctypes.data == V.ctypes.data and a[2] == G + 6


@pytest.mark.parametrize("dtype,want", [(np.int16, "i64"), (np.uint8, "i64"), (np.bool_, "i64"), (np.float16, "f64")])
def test_other_dtypes_are_cast_in_c_order(pkg, dtype, want, monkeypatch):
    monkeypatch.setenv("REO_ROWMAJOR", "1")
    G, S = 6, 4
    X = (np.arange(G * S).reshape(G, S) % 3).astype(dtype)
    sym, A, ld = pkg._ffi.host_matrix_entry(X)
    assert sym == "reo_set_matrix_rm_" + want and A.dtype == NATIVE[want]
    assert A.flags.c_contiguous and ld == S and np.array_equal(A, X.astype(NATIVE[want]))
    # the same values F-ordered: matrix_entry's column-major cast
    _same_route(pkg, np.asfortranarray(X))


def test_other_strides_go_through_matrix_entry(pkg, monkeypatch):
    monkeypatch.setenv("REO_ROWMAJOR", "1")
    X = np.arange(12 * 10, dtype=np.int64).reshape(12, 10)
    _same_route(pkg, X[::2, ::2])
    _same_route(pkg, np.broadcast_to(np.arange(10, dtype=np.float64), (12, 10)))            # zero stride along the genes
    _same_route(pkg, np.broadcast_to(np.arange(12, dtype=np.float64)[:, None], (12, 10)))   # ... along the samples
    _same_route(pkg, X.astype(np.int16)[:, 2:7])                                            # not a native dtype, not contiguous
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.host_matrix_entry(np.arange(5.0))
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.host_matrix_entry(np.zeros((2, 3, 4)))


@pytest.mark.parametrize("switch", ["0", None])
def test_switch_restores_the_column_major_copy(pkg, monkeypatch, switch):
    """REO_ROWMAJOR=0, and the variable unset (the route is opt-in): matrix_entry's answer for everything"""
    if switch is None: monkeypatch.delenv("REO_ROWMAJOR", raising=False)
    else: monkeypatch.setenv("REO_ROWMAJOR", switch)
    G, S = 7, 5
    wide = np.arange(G * 23, dtype=np.float32).reshape(G, 23)
    for X in (np.arange(G * S, dtype=np.int64).reshape(G, S), wide[:, 5:5 + S], np.ones((G, S), dtype=np.int16),
              np.asfortranarray(np.ones((G, S), dtype=np.int32)), np.arange(G * S, dtype=np.float64).reshape(G, S)[::2, ::2]):
        _same_route(pkg, X)
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.host_matrix_entry(np.arange(5.0))
    monkeypatch.setenv("REO_ROWMAJOR", "1")                                     # read per call
    assert pkg._ffi.host_matrix_entry(np.zeros((G, S)))[0] == "reo_set_matrix_rm_f64"


def test_row_readers_equal_the_column_readers_under_sanitizers(tmp_path):
    """tests/upload_rows_driver.cpp: narrow_rows / narrow_rows_f64 / pack_rows of csrc/upload_rows.h against a copy of the column
    readers, every narrow type, G in {1, 2, 63, 257}, chunks at both ends of a row of a source with ld > S, 1 / 3 / 7 row shares, and
    the verdicts at the 16- and 32-bit limits, one past them, -0.0, NaN, +-Inf, 2^53 and values float32 does not hold -- built with
    AddressSanitizer and UBSan, buffers at their exact sizes.  The digest pins images and verdicts."""
    exe = str(tmp_path / "upload_rows_driver")
    # -static-libasan / -static-libubsan: ASan's shared runtime checks at start-up that it comes first in the list of loaded libraries
    # and aborts if LD_PRELOAD names any other library; the static runtime makes no such check, and the program needs no LD_PRELOAD.
    # This needs gcc's static sanitizer archives (libasan.a, libubsan.a) next to the shared ones.  -fno-sanitize-recover: a UBSan
    # finding ends the program with a failure status instead of a line on stderr only.
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "upload_rows_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]                                  # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok 780 baa908d5f181998b", lines[-1]
    verdict = {}
    for l in lines[:-1]:
        t, which, v = l.split()
        verdict.setdefault((t, int(which)), []).append(v)
    # per special value: 3 places x 2 thread counts.  Int64 specials: 32767 32768 -32768 -32769 2^31-1 2^31 -2^31 -2^31-1 2^53
    per = 6
    i16 = [v[0] for v in zip(*[iter(verdict[("i64", 0)])] * per)]
    i32 = [v[0] for v in zip(*[iter(verdict[("i64", 1)])] * per)]
    assert all(len(set(g)) == 1 for g in zip(*[iter(verdict[("i64", 0)])] * per))
    assert i16 == ["fits", "wider", "fits", "wider", "wider", "wider", "wider", "wider", "wider"]
    assert i32 == ["fits", "fits", "fits", "fits", "fits", "wider", "fits", "wider", "wider"]
    # Float64 specials: the same eight limits, -0.0, NaN, +Inf, -Inf, 2^53, 0.1, 2^24 + 1, 0.5
    f16 = [v[0] for v in zip(*[iter(verdict[("f64", 0)])] * per)]
    f32i = [v[0] for v in zip(*[iter(verdict[("f64", 1)])] * per)]
    f32 = [v[0] for v in zip(*[iter(verdict[("f64", 2)])] * per)]
    assert f16 == ["fits", "wider", "fits", "wider"] + ["wider"] * 12
    assert f32i == ["fits"] * 5 + ["wider", "fits", "wider"] + ["wider"] * 5 + ["wider", "fits", "wider"]
    # as float32: 2^31 - 1 and -2^31 - 1 and 2^24 + 1 need more mantissa, 0.1 too; -0.0 and +-Inf convert back to the same bits
    # (they pass this reader -- the ranking's own rules see them on the device), NaN never equals itself
    assert f32 == ["fits"] * 4 + ["wider", "fits", "fits", "wider", "fits", "wider", "fits", "fits", "fits", "wider", "wider", "fits"]
