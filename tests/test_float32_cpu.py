"""Float32 / Int32 expression matrices: the ABI surface, the host-side entry choice and the conditions of the GPU tests
(tests/test_gpu_float32.py).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import float32_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["reo_set_matrix_f32", "reo_set_matrix_i32", "reo_set_matrix_dev_f32", "reo_set_matrix_dev_i32"]


def test_header_declares_and_library_exports_the_32_bit_entries(pkg):
    hdr = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    declared = set(re.findall(r"\b(reo_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(pkg._ffi.LIB_PATH)
    for s in NEW:
        assert s in declared, s
        assert hasattr(L, s), s
        assert s in pkg._ffi.SYMBOLS
    assert re.search(r"reo_set_matrix_f32\(reo_ctx \*ctx, const float \*X, int64_t G, int64_t S, int64_t ld\)", hdr)
    assert re.search(r"reo_set_matrix_i32\(reo_ctx \*ctx, const int32_t \*X, int64_t G, int64_t S, int64_t ld\)", hdr)
    assert "(double)fabsf(x - y) < 0.1" in hdr          # the Float32 rule is stated
    assert pkg._ffi.lib().reo_version() >= 200           # the minor version moved with the new entry points


@pytest.mark.parametrize("dtype,entry", [(np.float32, "reo_set_matrix_f32"), (np.int32, "reo_set_matrix_i32"),
                                         (np.float64, "reo_set_matrix_f64"), (np.int64, "reo_set_matrix_i64")])
def test_matrix_entry_hands_native_types_over_without_a_copy(pkg, dtype, entry):
    rng = np.random.default_rng(5)
    G, S = 37, 9
    X = np.asfortranarray(rng.integers(-50, 50, size=(G, S)).astype(dtype))
    name, out, ld = pkg._ffi.matrix_entry(X)
    assert name == entry and ld == G and out.dtype == dtype
    assert np.shares_memory(out, X) and out.ctypes.data == X.ctypes.data
    # a column-major view of rows of a taller matrix: passed with its leading dimension
    tall = np.asfortranarray(rng.integers(-50, 50, size=(G + 11, S)).astype(dtype))
    view = tall[3: 3 + G, :]
    name, out, ld = pkg._ffi.matrix_entry(view)
    assert name == entry and ld == G + 11
    assert np.shares_memory(out, tall) and out.ctypes.data == view.ctypes.data and np.array_equal(out, view)
    # a row-major matrix pays a transposing host copy and keeps its type
    C = np.ascontiguousarray(X)
    name, out, ld = pkg._ffi.matrix_entry(C)
    assert name == entry and ld == G and out.dtype == dtype and out.flags.f_contiguous and np.array_equal(out, C)


def test_matrix_entry_converts_every_other_type_as_before(pkg):
    rng = np.random.default_rng(6)
    base = rng.integers(0, 50, size=(12, 5))
    for dt in (np.int16, np.uint8, np.int8, np.uint32, np.bool_):
        name, out, ld = pkg._ffi.matrix_entry(np.asfortranarray(base.astype(dt)))
        assert name == "reo_set_matrix_i64" and out.dtype == np.int64 and ld == 12, dt
        assert np.array_equal(out, base.astype(dt).astype(np.int64))
    name, out, ld = pkg._ffi.matrix_entry(np.asfortranarray(base.astype(np.float16)))
    assert name == "reo_set_matrix_f64" and out.dtype == np.float64 and ld == 12
    name, out, ld = pkg._ffi.matrix_entry([[1, 2, 3], [4, 5, 6]])         # whatever np.asarray takes
    assert name == "reo_set_matrix_i64" and out.shape == (2, 3)
    with pytest.raises(pkg.DimensionMismatch):
        pkg._ffi.matrix_entry(np.zeros(5, dtype=np.float32))


def test_planted_pairs_separate_the_two_arithmetics(oracle):
    """The condition of the GPU tests: on planted(256, 64, 24) the Float32 comparator and the oracle's Float64 comparator on the
    widened matrix differ in at least 1 000 comparisons, each one Float32 "not tied" where Float64 says "tied"."""
    G, S = 256, 64
    X = fc.planted(G, S, 24, 0x5EED0F32)
    assert X.dtype == np.float32 and np.array_equal(X, fc.planted(G, S, 24, 0x5EED0F32))
    n, one_way, total = fc.disagreements(X)
    print(f"comparisons on which Float32 and Float64 disagree: {n} of {total} (Float32 not tied, Float64 tied: {one_way})")
    assert total == 2088960
    assert n >= 1000 and one_way == n
    # the same through the two restatements that the GPU tests use
    gid = (np.arange(S) >= S // 2).astype(np.int32)
    gt32, eq32 = fc.f32_pair_counts(X, gid, 2)
    gt64, eq64 = oracle.pair_counts(X.astype(np.float64), gid, 2, 0, G, 0, G)
    iu = np.triu_indices(G, 1)
    less_tied = (eq64.astype(np.int64) - eq32)[iu]
    assert (less_tied >= 0).all() and int(less_tied.sum()) == n
    more_ordered = (gt32 + gt32.transpose(1, 0, 2) - gt64.astype(np.int64) - gt64.transpose(1, 0, 2).astype(np.int64))[iu]
    assert np.array_equal(more_ordered, less_tied)       # a comparison that stops being a tie becomes an ordering, one way or the other


def test_exact_grid_is_the_same_in_both_arithmetics(oracle):
    G, S = 180, 12
    X = fc.exact_grid(G, S, 11)
    assert X.dtype == np.float32 and np.isinf(X).sum() >= 2
    finite = X[np.isfinite(X)].astype(np.float64) * 64.0
    assert np.array_equal(finite, np.rint(finite)) and np.abs(finite).max() < (1 << 17)
    n, _, total = fc.disagreements(X)
    assert n == 0 and total == G * (G - 1) // 2 * S
    gid = (np.arange(S) % 3).astype(np.int32)
    gt32, eq32 = fc.f32_pair_counts(X, gid, 3)
    gt64, eq64 = oracle.pair_counts(X.astype(np.float64), gid, 3, 0, G, 0, G)
    assert np.array_equal(gt32, gt64) and np.array_equal(eq32, eq64)
    off = ~np.eye(G, dtype=bool)
    assert eq32.sum(axis=2)[off].sum() > G               # ties are plentiful
