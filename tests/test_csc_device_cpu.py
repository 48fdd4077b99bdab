"""Sparse matrices on the device (reo_set_matrix_csc_dev_*, reo_set_matrix_pseudobulk_*_dev_*), the parts that need no GPU: the ABI, the
routing of _ffi.device_csc_entry on CPU torch tensors, and the predicates of csrc/csc_check.h -- the ones the validation kernel evaluates
-- under the sanitizers against the host readers of csrc/upload_csc.h."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = ("f64", "i64", "f32", "i32")
FORMS = {"csc_dev": 8, "pseudobulk_csc_dev": 12, "pseudobulk_dense_dev": 9}    # arguments of each family
TORCH = {"f64": torch.float64, "i64": torch.int64, "f32": torch.float32, "i32": torch.int32}


def test_header_declares_and_library_exports_the_twelve_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    L = pkg._ffi.lib()
    assert "SPARSE ON THE DEVICE." in header
    for form, nargs in FORMS.items():
        for t in TYPES:
            s = f"reo_set_matrix_{form}_{t}"
            m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", header)
            assert m, s
            assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
            assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == nargs
            assert hasattr(L, s), s
    assert re.search(r"reo_set_matrix_csc_dev_f64\(reo_ctx \*ctx, int64_t G, int64_t S, int64_t nnz, const void \*d_colptr, const void \*d_rowidx,\s+"
                     r"int32_t index_bits /\* 32 or 64 \*/, const void \*d_val\);", header)


def test_info_has_the_csc_device_slot(pkg):
    src = open(os.path.join(ROOT, "rankcompv3.jl_amd", "_ffi.py")).read()
    assert "np.zeros(28, dtype=np.int64)" in src and '"csc_device": int(v[27])' in src


def _dense(G, S, dtype, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.integers(1, 50, size=(G, S)) * (rng.random((G, S)) < 0.3)
    return torch.from_numpy(X.astype(np.float64)).to(dtype)


def _redensify(colptr, rowidx, val, G, S):
    D = torch.zeros((G, S), dtype=val.dtype)
    for s in range(S):
        a, b = int(colptr[s]), int(colptr[s + 1])
        assert bool((rowidx[a + 1:b] > rowidx[a:b - 1]).all())                   # strictly increasing inside a column
        D[rowidx[a:b].long(), s] = val[a:b]
    return D


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", TYPES)
def test_sparse_csc_is_used_in_place(pkg, name, bits):
    G, S = 9, 6
    X = _dense(G, S, TORCH[name])
    t = X.to_sparse_csc()
    idx = torch.int32 if bits == 32 else torch.int64
    t = torch.sparse_csc_tensor(t.ccol_indices().to(idx), t.row_indices().to(idx), t.values(), size=(G, S))
    ty, g, s, nnz, colptr, rowidx, val, b, keep = pkg._ffi.device_csc_entry(t)
    assert (ty, g, s, b) == (name, G, S, bits) and nnz == int((X != 0).sum()) == rowidx.numel() == val.numel()
    assert colptr.data_ptr() == t.ccol_indices().data_ptr() and rowidx.data_ptr() == t.row_indices().data_ptr()
    assert val.data_ptr() == t.values().data_ptr()
    assert colptr.dtype == rowidx.dtype == idx and val.dtype == TORCH[name] and colptr.numel() == S + 1
    assert torch.equal(_redensify(colptr, rowidx, val, G, S), X)
    assert any(k is val for k in keep)


def test_transposed_cells_by_genes_csr_is_a_csc_view(pkg):
    G, C = 7, 11
    X = _dense(G, C, torch.float32, seed=5)
    csr = X.t().contiguous().to_sparse_csr()                                     # cells x genes, AnnData's orientation
    t = csr.t()
    assert t.layout == torch.sparse_csc and tuple(t.shape) == (G, C)
    ty, g, s, nnz, colptr, rowidx, val, bits, _ = pkg._ffi.device_csc_entry(t)
    assert (ty, g, s, bits) == ("f32", G, C, 64)
    assert colptr.data_ptr() == csr.crow_indices().data_ptr() and rowidx.data_ptr() == csr.col_indices().data_ptr()
    assert val.data_ptr() == csr.values().data_ptr()
    assert torch.equal(_redensify(colptr, rowidx, val, G, C), X)


@pytest.mark.parametrize("layout", ["coo", "csr"])
def test_coo_and_csr_go_through_to_sparse_csc(pkg, layout):
    G, S = 11, 7
    X = _dense(G, S, torch.int64, seed=7)
    t = X.to_sparse_coo() if layout == "coo" else X.to_sparse_csr()
    ty, g, s, nnz, colptr, rowidx, val, bits, _ = pkg._ffi.device_csc_entry(t)
    assert (ty, g, s) == ("i64", G, S) and nnz == int((X != 0).sum()) and bits in (32, 64)
    assert torch.equal(_redensify(colptr, rowidx, val, G, S), X)
    assert torch.equal(t.to_dense(), X)                                          # the caller's tensor is as it was


@pytest.mark.parametrize("dtype,want", [(torch.float16, "f64"), (torch.bfloat16, "f64"), (torch.int16, "i64"), (torch.uint8, "i64"), (torch.bool, "i64"),
                                        (torch.float64, "f64"), (torch.int64, "i64"), (torch.float32, "f32"), (torch.int32, "i32")])
def test_value_dtype_rules(pkg, dtype, want):
    G, S = 8, 5
    X = _dense(G, S, torch.int64) % 3
    base = X.to_sparse_csc()
    vals = base.values().to(dtype)
    t = torch.sparse_csc_tensor(base.ccol_indices(), base.row_indices(), vals, size=(G, S))
    assert t.dtype == dtype
    ty, _, _, nnz, colptr, rowidx, val, _, _ = pkg._ffi.device_csc_entry(t)
    assert ty == want and val.dtype == TORCH[want] and nnz == vals.numel()
    assert torch.equal(val, vals.to(TORCH[want]))
    assert (val.data_ptr() == t.values().data_ptr()) == (dtype == TORCH[want])  # cast only when it has to be


def test_the_mirror_does_not_sort(pkg):
    """torch takes an unsorted column with check_invariants=False; the mirror hands it over as it is (the library refuses it)"""
    colptr = torch.tensor([0, 2, 2, 5]); rowidx = torch.tensor([4, 1, 0, 5, 2]); val = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64)
    t = torch.sparse_csc_tensor(colptr, rowidx, val, size=(6, 3), check_invariants=False)
    _, _, _, _, cp, ri, va, _, _ = pkg._ffi.device_csc_entry(t)
    assert ri.tolist() == [4, 1, 0, 5, 2] and cp.tolist() == [0, 2, 2, 5] and va.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    assert "coalesce().to_sparse_csc()" in pkg._ffi.device_csc_entry.__doc__


def test_batched_and_other_ranks_are_refused(pkg):
    X = _dense(4, 3, torch.float64)
    batched = torch.stack([X, X]).to_sparse_csc()
    assert batched.dim() == 3
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.device_csc_entry(batched)
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.device_csc_entry(torch.stack([X, X]).to_sparse_coo())


def test_is_device_sparse_is_false_off_the_gpu(pkg):
    X = _dense(4, 3, torch.float64)
    assert not pkg._ffi.is_device_sparse(X.to_sparse_csc())                      # a CPU tensor
    assert not pkg._ffi.is_device_sparse(X) and not pkg._ffi.is_device_sparse(np.eye(3)) and not pkg._ffi.is_device_sparse(None)
    assert not pkg._ffi.is_device_tensor(X.to_sparse_csc())


OK, ROW_RANGE, ROW_ORDER, COLPTR = 0, 1, 2, 3


def test_validation_predicates_under_sanitizers(tmp_path):
    """tests/csc_check_driver.cpp: csc_check_column / csc_check_entry / csc_check_share of csrc/csc_check.h, which the kernel csc_validate
    runs, over valid containers (empty column, full column, G = 2, nnz = 0, a descending pair across a column boundary) and one of every
    bad class, int32 and int64 indices, arrays at exactly S + 1 and nnz elements -- AddressSanitizer and UBSan stay silent, so no bad colptr
    caused a read -- and class and column agree with check_colptr_run / read_rows of csrc/upload_csc.h on the same container."""
    exe = str(tmp_path / "csc_check_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "csc_check_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    got = {}
    for l in lines[:-1]:
        _, name, bits, cls, col, _, rcls, rcol = l.split()
        got[(name, int(bits))] = (int(cls), int(col))
        if rcls != "-":
            assert (int(rcls), int(rcol)) == (int(cls), int(col)), l             # the host readers agree
    want = {"empty_and_full_columns": (OK, -1), "G2": (OK, -1), "no_entries": (OK, -1), "descending_across_columns": (OK, -1),
            "full_column_of_300": (OK, -1),
            "index_equal_G": (ROW_RANGE, 1), "negative_index": (ROW_RANGE, 2), "equal_pair": (ROW_ORDER, 1), "descending_pair": (ROW_ORDER, 1),
            "order_then_range_in_one_column": (ROW_ORDER, 0), "range_then_order_in_one_column": (ROW_RANGE, 0),
            "fault_in_entry_299_of_300": (ROW_ORDER, 1), "two_faulty_columns_the_lower_one": (ROW_ORDER, 0),
            "colptr_starts_at_1": (COLPTR, 0), "colptr_decreasing": (COLPTR, 1), "colptr_end_beyond_nnz": (COLPTR, 2),
            "colptr_end_short_of_nnz": (COLPTR, 2), "colptr_negative": (COLPTR, 0), "colptr_middle_beyond_nnz": (COLPTR, 1),
            "column_longer_than_G": (COLPTR, 0), "colptr_fault_behind_a_row_fault": (COLPTR, 2)}
    for name, v in want.items():
        assert got[(name, 32)] == v and got[(name, 64)] == v, (name, got[(name, 32)], got[(name, 64)])
    assert got[("index_2_pow_32_plus_1", 64)] == (ROW_RANGE, 1) and got[("colptr_2_pow_40", 64)] == (COLPTR, 1)
    assert len(got) == 2 * len(want) + 2
