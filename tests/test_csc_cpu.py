"""Sparse host matrices (reo_set_matrix_csc_*), the parts that need no GPU: the ABI, the routing of _ffi.csc_entry, the sparse input of
run_identify_degs and the host readers of csrc/upload_csc.h under the sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSC = ["reo_set_matrix_csc_f64", "reo_set_matrix_csc_i64", "reo_set_matrix_csc_f32", "reo_set_matrix_csc_i32"]
NATIVE = {"f64": np.float64, "i64": np.int64, "f32": np.float32, "i32": np.int32}
CTYPE = {"f64": "double", "i64": "int64_t", "f32": "float", "i32": "int32_t"}


def test_header_declares_and_library_exports_the_csc_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    L = pkg._ffi.lib()
    for s in CSC:
        want = (r"int32_t\s+" + s + r"\s*\(reo_ctx \*ctx, int64_t G, int64_t S, const int64_t \*colptr, const int32_t \*rowidx, const "
                + CTYPE[s[-3:]] + r"\s*\*val\);")
        assert re.search(want, header), s
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES
        assert len(pkg._ffi.SIGNATURES[s][1]) == 6
        assert hasattr(L, s)
    assert "SPARSE." in header
    assert L.reo_version() >= 400


def _thin(G, S, dtype, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 50, size=(G, S)) * (rng.random((G, S)) < 0.3)
    return X.astype(dtype)


def _redensify(colptr, rowidx, val, G, S):
    D = np.zeros((G, S), dtype=val.dtype)
    for s in range(S):
        sl = slice(colptr[s], colptr[s + 1])
        assert np.all(np.diff(rowidx[sl]) > 0)                                  # strictly increasing inside a column
        D[rowidx[sl], s] = val[sl]
    return D


@pytest.mark.parametrize("name", sorted(NATIVE))
def test_canonical_csc_is_handed_over_without_copying_the_values(pkg, name):
    G, S = 9, 6
    X = _thin(G, S, NATIVE[name])
    M = sp.csc_matrix(X)
    assert M.has_canonical_format and M.indices.dtype == np.int32
    sym, colptr, rowidx, val, g, s = pkg._ffi.csc_entry(M)
    assert sym == "reo_set_matrix_csc_" + name and (g, s) == (G, S)
    assert np.shares_memory(val, M.data) and val.ctypes.data == M.data.ctypes.data
    assert np.shares_memory(rowidx, M.indices)                                  # int32 already: no copy either
    assert colptr.dtype == np.int64 and rowidx.dtype == np.int32 and val.dtype == NATIVE[name]
    assert colptr[0] == 0 and colptr[-1] == M.nnz == rowidx.size == val.size and colptr.size == S + 1
    assert np.array_equal(_redensify(colptr, rowidx, val, G, S), X)


@pytest.mark.parametrize("make", [sp.csr_matrix, sp.coo_matrix, sp.csc_matrix])
def test_csr_and_coo_go_through_tocsc(pkg, make):
    G, S = 11, 7
    X = _thin(G, S, np.int64, seed=5)
    M = make(X)
    sym, colptr, rowidx, val, g, s = pkg._ffi.csc_entry(M)
    assert sym == "reo_set_matrix_csc_i64" and (g, s) == (G, S)
    assert np.array_equal(_redensify(colptr, rowidx, val, G, S), X)
    assert np.array_equal(M.toarray(), X)


def test_int64_indices_are_narrowed_and_values_keep_their_place(pkg):
    G, S = 9, 6
    X = _thin(G, S, np.float64)
    M = sp.csc_matrix(X)
    M64 = M.copy()                                                              # (the constructor would narrow the indices again)
    M64.indices = M64.indices.astype(np.int64)
    M64.indptr = M64.indptr.astype(np.int64)
    assert M64.indices.dtype == np.int64
    sym, colptr, rowidx, val, _, _ = pkg._ffi.csc_entry(M64)
    assert rowidx.dtype == np.int32 and colptr.dtype == np.int64 and np.shares_memory(val, M64.data)
    assert np.array_equal(_redensify(colptr, rowidx, val, G, S), X)


@pytest.mark.parametrize("dtype,want", [(np.int16, "i64"), (np.bool_, "i64"), (np.float16, "f64")])
def test_other_value_dtypes_are_cast(pkg, dtype, want):
    G, S = 8, 5
    X = _thin(G, S, np.int64) % 3
    M = sp.csc_matrix(X)
    # (built from the three arrays: the constructor keeps a value dtype it would not choose itself)
    Md = sp.csc_matrix((M.data.astype(dtype), M.indices, M.indptr), shape=(G, S))
    if Md.dtype != np.dtype(dtype):
        Md.data = M.data.astype(dtype)
    sym, colptr, rowidx, val, _, _ = pkg._ffi.csc_entry(Md)
    assert sym == "reo_set_matrix_csc_" + want and val.dtype == NATIVE[want]
    assert np.array_equal(_redensify(colptr, rowidx, val, G, S), X.astype(dtype).astype(NATIVE[want]))


@pytest.mark.parametrize("fault", ["unsorted", "duplicates"])
def test_non_canonical_csc_is_copied_and_the_caller_keeps_its_arrays(pkg, fault):
    G, S = 6, 3
    if fault == "unsorted":
        data = np.array([1.0, 2.0, 3.0, 4.0, 5.0]); indices = np.array([4, 1, 0, 5, 2], dtype=np.int32); indptr = np.array([0, 2, 2, 5], dtype=np.int32)
    else:
        data = np.array([1.0, 2.0, 3.0, 4.0, 5.0]); indices = np.array([1, 1, 0, 2, 2], dtype=np.int32); indptr = np.array([0, 2, 2, 5], dtype=np.int32)
    M = sp.csc_matrix((data, indices, indptr), shape=(G, S))
    assert np.shares_memory(M.data, data) and not M.has_canonical_format
    before = (M.data.tobytes(), M.indices.tobytes(), M.indptr.tobytes())
    dense = M.toarray()                                                         # (duplicates add up)
    sym, colptr, rowidx, val, g, s = pkg._ffi.csc_entry(M)
    assert sym == "reo_set_matrix_csc_f64"
    assert np.array_equal(_redensify(colptr, rowidx, val, G, S), dense)
    assert (M.data.tobytes(), M.indices.tobytes(), M.indptr.tobytes()) == before
    assert not np.shares_memory(val, M.data)


def test_is_sparse_keeps_arrays_on_their_route(pkg):
    assert pkg._ffi.is_sparse(sp.csr_matrix(np.eye(3)))
    assert not pkg._ffi.is_sparse(np.eye(3)) and not pkg._ffi.is_sparse([[1, 2], [3, 4]])


def test_sparse_data_fails_like_dense_data_without_a_gpu(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    M = sp.csr_matrix(_thin(12, 4, np.int64))
    names = list("abcdefghijkl")
    with pytest.raises(pkg.ReoError) as e:
        pkg.run_identify_degs(M, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(12, bool), 2, 1)
    assert e.value.status == pkg._ffi.REO_EHIP and not isinstance(e.value, pkg.DimensionMismatch)


def test_sparse_data_keeps_the_shape_checks(pkg):
    M = sp.csr_matrix(_thin(12, 4, np.int64))
    names = list("abcdefghijkl")
    with pytest.raises(pkg.DimensionMismatch) as e:                             # :355
        pkg.run_identify_degs(M, ["a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(12, bool), 2, 1)
    assert "group" in e.value.message
    with pytest.raises(pkg.DimensionMismatch) as e:
        pkg.run_identify_degs(M, ["a", "a", "b", "b"], names[:-1], 0.01, 1.0, 0.05, np.ones(12, bool), 2, 1)
    assert "gene_names" in e.value.message


def test_csc_readers_under_sanitizers(tmp_path):
    """tests/upload_csc_driver.cpp: check_colptr_run / read_rows / narrow_values of csrc/upload_csc.h on containers and images at their
    exact sizes -- runs of 0 entries, one full column, many columns over 1 / 3 / 7 thread shares, an empty first and last column; G = 2,
    65 536 and 65 537 (16- and 32-bit row images); the verdicts for a row index equal to G, a negative one, an equal and a descending
    pair inside a column and a descending pair across a column boundary (legal); the value ladders at the 16- / 32-bit limits, one past
    them, -0.0, +-Inf, NaN, 2^53, 0.1 -- built with AddressSanitizer and UBSan as a program of its own.  The digest pins images and
    verdicts."""
    exe = str(tmp_path / "upload_csc_driver")
    # (static sanitizer runtimes, as tests/test_rowmajor_cpu.py builds its driver: the program needs no preloaded runtime)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "upload_csc_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]                                  # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok 593 ab6646b56fc3b167", lines[-1]
    rows, colptr, values = {}, {}, {}
    for l in lines[:-1]:
        kind, which, v = l.split()
        if kind == "rows": rows.setdefault(which, set()).add(int(v))
        elif kind == "colptr": colptr[which] = int(v)
        else: values.setdefault((kind, int(which)), []).append(v)
    # 0 ok, 1 a row index outside [0, G), 2 not strictly increasing, 3 not a column pointer: the same for 1, 3 and 7 shares
    assert rows == {"index_equal_G": {1}, "negative_index": {1}, "equal_pair": {2}, "descending_pair": {2}, "descending_across_columns": {0},
                    "row_65536_of_65537": {0}, "row_65537_of_65537": {1}}
    assert colptr == {"good": 0, "decreasing": 3, "beyond_nnz": 3, "negative_start": 3, "column_longer_than_G": 3}
    per = 6   # per special value: 3 places x 2 share counts, all the same verdict
    def firsts(key):
        groups = list(zip(*[iter(values[key])] * per))
        assert all(len(set(g)) == 1 for g in groups)
        return [g[0] for g in groups]
    # Int64 specials: 32767 32768 -32768 -32769 2^31-1 2^31 -2^31 -2^31-1 2^53
    assert firsts(("i64", 0)) == ["fits", "wider", "fits", "wider", "wider", "wider", "wider", "wider", "wider"]
    assert firsts(("i64", 1)) == ["fits", "fits", "fits", "fits", "fits", "wider", "fits", "wider", "wider"]
    # Float64 specials: the same eight limits, -0.0, NaN, +Inf, -Inf, 2^53, 0.1, 2^24 + 1, 0.5, 1e300 -- the verdicts of the dense
    # readers (tests/test_rowmajor_cpu.py) for the same values
    assert firsts(("f64", 0)) == ["fits", "wider", "fits", "wider"] + ["wider"] * 13
    assert firsts(("f64", 1)) == ["fits"] * 5 + ["wider", "fits", "wider"] + ["wider"] * 5 + ["wider", "fits", "wider", "wider"]
    assert firsts(("f64", 2)) == ["fits"] * 4 + ["wider", "fits", "fits", "wider", "fits", "wider", "fits", "fits", "fits", "wider", "wider", "fits", "wider"]
