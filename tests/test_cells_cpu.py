"""Cells to DEGs with the profiles resident (reo_set_matrix_pseudobulk_*, reo_filter_matrix, reo_get_matrix, identify_degs_cells), the
parts that need no GPU: the ABI, hotpath.cells_partition against the construction of reoa.prepare, a numpy statement of the two filters
on special values, and csrc/filter_maps.h under the sanitizers."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = ["reo_set_matrix_pseudobulk_dense_f64", "reo_set_matrix_pseudobulk_dense_i64", "reo_set_matrix_pseudobulk_csc_f64",
      "reo_set_matrix_pseudobulk_csc_i64"]
NEW = PB + ["reo_filter_matrix", "reo_get_matrix"]


def test_header_declares_and_library_exports_the_new_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    L = pkg._ffi.lib()
    for s in NEW:
        assert re.search(r"int32_t\s+" + s + r"\s*\(reo_ctx \*ctx,", header), s
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES
        assert hasattr(L, s), s
    for s in PB:   # the arguments of the matching reo_pseudobulk_*, without `out`
        twin = s.replace("reo_set_matrix_pseudobulk_", "reo_pseudobulk_")
        assert pkg._ffi.SIGNATURES[s] == (pkg._ffi.SIGNATURES[twin][0], pkg._ffi.SIGNATURES[twin][1][:-1])
    assert len(pkg._ffi.SIGNATURES["reo_filter_matrix"][1]) == 7 and len(pkg._ffi.SIGNATURES["reo_get_matrix"][1]) == 3
    assert re.search(r"int32_t\s+reo_filter_matrix\s*\(reo_ctx \*ctx, int64_t min_profiles, int64_t min_features, uint8_t \*profile_kept, "
                     r"uint8_t \*gene_kept,\s*int64_t \*S_kept, int64_t \*G_kept\);", header)
    assert re.search(r"int32_t\s+reo_get_matrix\s*\(reo_ctx \*ctx, void \*out, int64_t bytes\);", header)
    assert "CELLS." in header and "ORDER OF CALLS with them" in header
    assert L.reo_version() >= 500
    for name in ("identify_degs_cells", "cells_partition", "CellsDegRun"):
        assert hasattr(pkg, name) and name in pkg.__all__
    for m in ("set_matrix_pseudobulk", "filter_matrix", "get_matrix"):
        assert callable(getattr(pkg.Context, m))


def _prepare_construction(R, values, cell_group, n_pseudo, seed):
    """reoa.prepare, lines 149-156, on a cell matrix whose column t has group cell_group[t] (the meta table in column order)."""
    g_name = list(dict.fromkeys(cell_group))
    mats, names, groups = [], [], []
    for gi, g in enumerate(g_name):
        cols = [t for t, c in enumerate(cell_group) if c == g]
        m, nm = R.pseudobulk_group(values[:, cols], n_pseudo, g, seed, gi, R.host_sums)
        mats.append(m); names += nm; groups += [g] * len(nm)
    return np.concatenate(mats, axis=1), names, groups


@pytest.mark.parametrize("labels,n_pseudo", [
    (["a", "b"] * 9 + ["a"] * 5, 4),                      # two groups, interleaved, 14 + 9 cells
    (["t", "c", "x", "c", "t", "t", "x", "c", "t", "c", "t", "x", "t"], 3),   # three groups, interleaved
    (["p"] * 9 + ["q"] * 20, 7),                         # 9 cells, n_pseudo 7: ceil(9 / 7) = 2 cells per chunk -> 5 chunks, not 7
    (["u", "v", "w"] * 3 + ["v"] * 8, 5),                 # three groups; u and w: 3 cells -> ceil = 1 -> 3 chunks
])
def test_cells_partition_is_the_construction_of_reoa_prepare(pkg, labels, n_pseudo):
    R = importlib.import_module(pkg.__name__ + ".reoa")
    seed = 0x5EED0CE1
    rng = np.random.default_rng(7)
    values = rng.integers(0, 50, size=(6, len(labels))).astype(np.int64)
    order, ptr, names, groups = pkg.cells_partition(labels, n_pseudo, seed)
    assert order.dtype == np.int32 and ptr.dtype == np.int32
    assert ptr[0] == 0 and ptr[-1] == order.size == len(labels) and np.all(np.diff(ptr) > 0)
    assert sorted(order.tolist()) == list(range(len(labels)))
    exp, enames, egroups = _prepare_construction(R, values, labels, n_pseudo, seed)
    assert names == enames and groups == egroups
    assert np.array_equal(R.host_sums(values, order, ptr), exp)
    lev = list(dict.fromkeys(labels))
    for g in lev:   # the chunk count of a group whose ceil(c / n_pseudo) does not divide into n_pseudo chunks
        c = labels.count(g)
        cp = -(-c // n_pseudo)
        assert groups.count(g) == -(-c // cp)
    if labels[0] == "p":
        assert groups.count("p") == 5 and groups.count("q") == 7
    # float sums take the cells in the same order: bit-equal
    fv = rng.random((6, len(labels)))
    assert np.array_equal(R.host_sums(fv, order, ptr), _prepare_construction(R, fv, labels, n_pseudo, seed)[0])


def filters_numpy(X, min_profiles, min_features):
    """src/RankCompV3.jl:618 then :626 as reoa.prepare writes them."""
    s_inds = (X > 0).sum(axis=0) > min_profiles
    kept = X[:, s_inds]
    inds = (kept > 0).sum(axis=1) > min_features
    return s_inds, inds, kept[inds, :]


def test_the_two_filters_on_special_values():
    sub = 5e-324
    with np.errstate(invalid="ignore"):
        X = np.array([
            # s0     s1      s2      s3     s4
            [-0.0,   1.0,    2.0,    0.0,   np.nan],    # g0: positive in s1 s2
            [-1.0,   np.inf, 0.0,    0.0,   np.nan],    # g1: +Inf counts (s1)
            [0.0,    sub,    sub,    0.0,   -np.inf],   # g2: subnormals count (s1 s2)
            [-0.0,   0.0,    -3.0,   7.0,   np.nan],    # g3: expressed only in s3
            [np.nan, 0.0,    -0.0,   0.0,   0.0],       # g4: nothing
        ])
        assert (X > 0).sum(axis=0).tolist() == [0, 3, 2, 1, 0]    # -0.0, negatives, NaN and -Inf do not count
        pk, gk, out = filters_numpy(X, 1, 0)                      # s3 has 1 positive: equal to the threshold, dropped
        assert pk.tolist() == [False, True, True, False, False]
        assert gk.tolist() == [True, True, True, False, False]    # g3 lived in the dropped s3 only
        assert out.shape == (3, 2) and out[1, 0] == np.inf and out[2, 1] == sub
        pk, gk, out = filters_numpy(X, 1, 1)                      # g1 has 1 positive among the kept: equal, dropped
        assert gk.tolist() == [True, False, True, False, False]
        pk, gk, out = filters_numpy(X, 0, 0)
        assert pk.tolist() == [False, True, True, True, False] and gk.tolist() == [True, True, True, True, False]
        # the rule the device evaluates on the bits (csrc/filter_maps.h, positive_bits) is the same predicate
        bits = X.view(np.int64)
        assert np.array_equal((bits > 0) & (bits <= np.float64(np.inf).view(np.int64)), X > 0)
        f = X.astype(np.float32)
        f[2, 1] = f[2, 2] = np.float32(1e-45)
        fb = f.view(np.int32)
        assert np.array_equal((fb > 0) & (fb <= np.float32(np.inf).view(np.int32)), f > 0)


def test_filter_maps_under_sanitizers(tmp_path):
    """tests/filter_maps_driver.cpp: filter_maps / filter_flags / positive_bits of csrc/filter_maps.h -- all kept, none kept, G' = 1,
    S' = 1, counts equal to the threshold (strict >), first and last element dropped, null masks, thresholds outside int32, and the bit
    rule on -0.0, negatives, +-Inf, subnormals and NaNs -- with counts and masks in heap blocks of their exact sizes, built with
    AddressSanitizer and UBSan as a program of its own."""
    exe = str(tmp_path / "filter_maps_driver")
    # (static sanitizer runtimes, as tests/test_csc_cpu.py builds its driver: the program needs no preloaded runtime)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "filter_maps_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]                                  # the sanitizers stay silent
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok 49", lines[-1]
    assert "all_kept 111 1111" in lines and "none_kept 000 00" in lines and "one_gene 1 3" in lines and "one_profile 3 1" in lines
    assert "at_threshold 01010 01001" in lines and "ends_dropped 1,2,3, 1,2,3," in lines


def test_cells_call_checks_its_arguments_before_the_gpu(pkg):
    X = np.zeros((12, 6), dtype=np.int64)
    names = list("abcdefghijkl")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.identify_degs_cells(X, ["a", "b"] * 2, names, 2, 0.01, 1.0, 0.05, None, 2, 1)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.identify_degs_cells(X, ["a", "b"] * 3, names[:-1], 2, 0.01, 1.0, 0.05, None, 2, 1)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.identify_degs_cells(X, ["a", "b"] * 3, names, 2, 0.01, 1.0, 0.05, np.ones(5, bool), 2, 1)
