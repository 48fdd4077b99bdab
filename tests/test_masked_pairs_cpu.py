"""The masked build (reo_set_valid_mask, reo_build_pairs_masked, reo_pair_counts_masked), the parts that need no GPU: the ABI, the shared
arithmetic and host argument checks of csrc/masked_pairs.h under the sanitizers, the numpy restatement against the oracle's build_codes,
and the argument handling of run_identify_degs that happens before a context is opened."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import masked_pairs_cases as mpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"reo_set_valid_mask": 5, "reo_build_pairs_masked": 4, "reo_pair_counts_masked": 8}


def test_header_declares_and_library_exports_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declaration hold , and ;)
    L = pkg._ffi.lib()
    for s, nargs in ENTRIES.items():
        m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, m.group(1)
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == nargs
        assert hasattr(L, s)
    assert L.reo_version() >= 1200
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer


def test_rules_words_thresholds_and_argument_checks_under_sanitizers(tmp_path, golden):
    """tests/masked_pairs_driver.cpp: the side-class rule on hand cases, validity words with padding slots and a group of exactly 32
    samples, the block counts, the threshold function against tests/golden/thresholds.json, every argument check with its message.
    AddressSanitizer and UBSan stay silent."""
    exe = str(tmp_path / "masked_pairs_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "masked_pairs_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 2000 + 100 + 80
    want = golden("thresholds.json")
    got = {}
    for l in lines[:-1]:
        tag, p, n, m = l.split()
        assert tag == "thr"
        got.setdefault(p, {})[n] = int(m)
    assert got == {p: {n: int(m) for n, m in tab.items()} for p, tab in want.items()}


@pytest.mark.parametrize("G,sizes,frac,seed", [(72, (37, 43), 0.25, 0x5EED0B01), (64, (20, 45), 0.40, 0x5EED0B02), (48, (33, 31, 40), 0.30, 0x5EED0B03)])
def test_restatement_with_an_all_ones_mask_is_build_codes(rn, G, sizes, frac, seed):
    """all-ones mask, min_complete <= the side sizes: the oracle's table, ties and coins included, for every comparison"""
    X, V, gid = mpc.float_case(G, sizes, frac, seed)
    ng = len(sizes)
    counts = mpc.masked_counts(X, np.ones_like(V), gid, ng)
    n_gt, n_eq = rn.pair_counts(X, gid, ng)
    assert np.array_equal(counts[0], n_gt) and np.array_equal(counts[1], n_eq)
    assert np.array_equal(counts[2], np.broadcast_to(np.bincount(gid), counts[2].shape))
    assert (n_eq.sum(axis=2)[np.triu_indices(G, 1)] > 0).mean() > 0.5           # the coins are exercised
    cnt = np.bincount(gid)
    for k in range(ng if ng > 2 else 1):
        thr = (rn.threshold(int(cnt[k])), rn.threshold(int(cnt.sum() - cnt[k])))
        want = rn.build_codes(X, gid, ng, k, thr, seed)
        for mc in ((1, 1), mpc.default_min_complete(cnt, k, 0.01), (int(cnt[k]), int(cnt.sum() - cnt[k]))):
            assert np.array_equal(mpc.masked_codes(counts, k, 0.01, mc, seed), want), (k, mc)
    # and the mask matters: with it the table differs
    plain0 = rn.build_codes(X, gid, ng, 0, (rn.threshold(int(cnt[0])), rn.threshold(int(cnt.sum() - cnt[0]))), seed)
    assert not np.array_equal(mpc.masked_codes(mpc.masked_counts(X, V, gid, ng), 0, 0.01, mpc.default_min_complete(cnt, 0, 0.01), seed), plain0)


def test_first_case_has_all_nine_codes_and_both_reasons():
    """the first GPU case cannot go hollow: every class code occurs, and class 2 occurs for a short side and for a lacking majority"""
    X, V, gid, seed = mpc.first_case()
    code, why = mpc.masked_codes(mpc.masked_counts(X, V, gid, 2), 0, 0.01, (8, 8), seed, detail=True)
    assert set(np.unique(code)) == set(range(9)) | {255}
    assert why["short_c"].any() and why["nomaj_c"].any() and why["nomaj_t"].any()
    assert (V[2, gid == 0].sum(), V[0, gid == 0].sum(), V[1].all()) == (5, 0, True)


def test_min_complete_and_mask_helpers(pkg):
    f = pkg._ffi
    assert f.first_informative_n(0.01) == 8 and f.first_informative_n(0.05) == 6
    assert f.resolve_min_complete(None, (37, 43), 0.01) == (8, 8) and f.resolve_min_complete(None, (5, 43), 0.01) == (5, 8)
    assert f.resolve_min_complete(3, (37, 43), 0.01) == (3, 3) and f.resolve_min_complete((2, 9), (37, 43), 0.01) == (2, 9)
    for bad in (0, -1, (0, 3), (3,), (1, 2, 3)):
        with pytest.raises(pkg.DimensionMismatch, match="min_complete"):
            f.resolve_min_complete(bad, (37, 43), 0.01)
    with pytest.raises(pkg.DimensionMismatch, match="pval_reo"):
        f.first_informative_n(0.0)
    v = f.valid_mask_bytes(np.array([[True, False, True], [False, False, True]]), (2, 3))
    assert v.dtype == np.uint8 and v.flags.f_contiguous and v.tolist() == [[1, 0, 1], [0, 0, 1]]
    assert f.valid_mask_bytes(np.array([[2.5, 0.0]]), (1, 2)).tolist() == [[1, 0]]
    with pytest.raises(pkg.DimensionMismatch, match="valid mask has shape"):
        f.valid_mask_bytes(np.ones((3, 2)), (2, 3))
    p = inspect.signature(pkg.Context.build_pairs_masked).parameters
    assert list(p) == ["self", "k", "pval_reo", "min_complete"] and (p["k"].default, p["pval_reo"].default, p["min_complete"].default) == (0, 0.01, None)
    assert list(inspect.signature(pkg.Context.pair_counts_masked).parameters) == ["self", "i0", "i1", "j0", "j1"]
    assert list(inspect.signature(pkg.Context.set_valid_mask).parameters) == ["self", "valid"]


def test_missing_defaults_are_none_and_keyword_only(pkg):
    for name in ("missing", "valid", "min_complete"):
        p = inspect.signature(pkg.run_identify_degs).parameters[name]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, name


def test_mask_derivation_from_nan_leaves_the_callers_array(pkg):
    hotpath = pkg.hotpath
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    X[1, 2] = X[4, 0] = np.nan
    keep = X.copy()
    data, mask = hotpath.missing_plan(X, "pairwise", None)
    assert np.array_equal(mask, ~np.isnan(keep)) and mask.dtype == bool
    assert data is not X and not np.isnan(data).any() and data[1, 2] == 0 and data[4, 0] == 0
    assert np.array_equal(data[mask], keep[mask])
    assert np.array_equal(np.isnan(X), np.isnan(keep)) and np.array_equal(X[mask], keep[mask])   # untouched
    # nothing asked for: the data as it came, no mask
    data, mask = hotpath.missing_plan(X, None, None)
    assert data is X and mask is None
    # an explicit mask for any host dtype; it implies the route
    Xi = np.arange(24, dtype=np.int64).reshape(6, 4)
    V = np.ones((6, 4), dtype=np.uint8)
    V[2, 3] = 0
    data, mask = hotpath.missing_plan(Xi, None, V)
    assert np.array_equal(data, Xi) and mask.dtype == bool and not mask[2, 3] and mask.sum() == 23
    # a float matrix without NaN under missing="pairwise": an all-ones mask, no copy needed
    clean = np.ones((3, 4))
    data, mask = hotpath.missing_plan(clean, "pairwise", None)
    assert mask.all() and np.array_equal(data, clean)


def test_every_refusal_comes_before_any_context(pkg):
    """No GPU here: opening a context would raise a ReoError that is no DimensionMismatch."""
    names = [f"g{i}" for i in range(6)]
    grp = ["a", "a", "b", "b"]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    X[1, 2] = np.nan
    args = (grp, names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)

    def refused(match, data=X, **kw):
        with pytest.raises(pkg.DimensionMismatch, match=match):
            pkg.run_identify_degs(data, *args, **kw)

    refused("missing = 'impute'", missing="impute")
    refused("missing = True", missing=True)
    refused(r"shard = \(0, 2\)", missing="pairwise", shard=(0, 2))
    refused("`contrasts`", missing="pairwise", contrasts="all")
    refused("`sample_scores`", missing="pairwise", sample_scores=True)
    refused("`sample_tests`", missing="pairwise", sample_tests=True)
    refused("`sample_calls`", missing="pairwise", sample_calls=True)
    refused("`pair_support`", missing="pairwise", pairs="reversed", pair_support=True)
    refused("`sample_tests`", data=np.nan_to_num(X), valid=np.ones((6, 4), bool), sample_tests=True)
    refused(r"valid mask has shape \(4, 6\)", data=np.nan_to_num(X), valid=np.ones((4, 6), bool))
    refused(r"valid mask has shape \(6,\)", data=np.nan_to_num(X), valid=np.ones(6, bool))
    refused("needs a matrix without NaN", valid=np.ones((6, 4), bool))
    refused("cannot hold one", data=np.arange(24).reshape(6, 4), missing="pairwise")
    refused("min_complete", missing="pairwise", min_complete=0)
    refused("min_complete", missing="pairwise", min_complete=(1, 2, 3))
    refused("sparse or device-resident", data=type("Sparse", (), {"tocsc": lambda self: self, "shape": (6, 4)})(), missing="pairwise")
