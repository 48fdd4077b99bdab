"""The label-permutation null (reo_perm_null, reo_perm_codes), the parts that need no GPU: the ABI, the shared arithmetic and host argument
checks of csrc/perm_null.h under the sanitizers (a stand-alone driver, tests/perm_null_driver.cpp), the word packing against a numpy
restatement, permuted_labels, the numpy restatement of a permuted table against the oracle's build_codes on the relabelled two-group
problem, and the argument handling of run_identify_degs that happens before a context is opened."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import perm_null_cases as pnc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"reo_perm_null": 13, "reo_perm_codes": 8}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("perm_null") / "perm_null_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "perm_null_driver.cpp")])
    return exe


def test_header_declares_and_library_exports_the_entries(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = pkg._ffi.lib()
    for s, nargs in ENTRIES.items():
        m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, m.group(1)
        assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == nargs
        assert hasattr(L, s)


def test_rules_and_argument_checks_under_sanitizers(driver):
    """row checks (a wrong count of ones and a byte other than 0 / 1 are both refused, with the row, the column and the value in the
    message), the exceed rule at equality and at delta1 = 0, the batch width, every argument check.  ASan and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    assert re.fullmatch(r"ok \d+", run.stdout.splitlines()[-1]) and int(run.stdout.split()[-1]) >= 86


@pytest.mark.parametrize("sizes", [(12, 9), (32, 64), (1, 20), (33, 31), (5, 40, 33)])
def test_word_packing_against_numpy(driver, sizes):
    """group sizes that are no multiples of 32, exactly 32 and 64, a group of one sample, a block seam inside a group, three groups;
    18 rows: a whole launch group of 16 and a ragged one"""
    rng = np.random.default_rng(sum(sizes))
    gid = pnc.mpc.interleaved(*sizes) if len(sizes) == 2 else np.repeat(np.arange(3, dtype=np.int32), sizes)
    S, B = int(gid.size), 18
    rows = pnc.shuffled_rows(gid, 0, B, sum(sizes))
    rows[1] = rng.permutation(rows[1])
    text = f"{S} {B} {len(sizes)}\n" + " ".join(map(str, gid)) + "\n" + "\n".join(" ".join(map(str, r)) for r in rows) + "\n"
    run = subprocess.run([driver, "words"], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    aw, live = pnc.pack_words(rows, gid, len(sizes))
    assert lines[0].split()[0] == "live" and np.array_equal(np.array(lines[0].split()[1:], dtype=np.uint64), live)
    got = np.array([l.split()[1:] for l in lines[1:]], dtype=np.uint64)
    assert got.shape == aw.shape and np.array_equal(got, aw)
    assert not (aw & ~live[None, :]).any()                                                   # A is a subset of live
    assert all(bin(int(w)).count("1") for w in live) and sum(bin(int(w)).count("1") for w in live) == S
    assert np.array_equal(np.array([sum(bin(int(w)).count("1") for w in r) for r in aw]), rows.sum(axis=1))


def test_permuted_labels(pkg):
    gid = np.array([0, 1] * 10 + [1] * 5, dtype=np.int32)
    rows = pkg.permuted_labels(gid, 0, 50, seed=3)
    assert rows.dtype == np.uint8 and rows.shape == (50, 25) and set(np.unique(rows)) == {0, 1}
    assert (rows.sum(axis=1) == 10).all()                                                    # the count of ones is kept
    obs = (gid == 0).astype(np.uint8)
    assert not (rows == obs).all(axis=1).any() and len({r.tobytes() for r in rows}) == 50    # never the observed labelling, never twice
    assert np.array_equal(rows, pkg.permuted_labels(gid, 0, 50, seed=3))                     # the same seed, the same rows
    assert not np.array_equal(rows, pkg.permuted_labels(gid, 0, 50, seed=4))
    assert (pkg.permuted_labels(gid, 1, 7, seed=3).sum(axis=1) == 15).all()
    first = pkg.permuted_labels(gid, 0, 5, seed=3, include_observed=True)
    assert np.array_equal(first[0], obs) and not (first[1:] == obs).all(axis=1).any()
    strata = np.array(["a"] * 8 + ["b"] * 8 + ["c"] * 9)
    rs = pkg.permuted_labels(gid, 0, 40, seed=5, strata=strata)
    for v in ("a", "b", "c"):
        assert (rs[:, strata == v].sum(axis=1) == obs[strata == v].sum()).all(), v             # shuffled inside each stratum
    assert np.array_equal(rs, pkg.permuted_labels(gid, 0, 40, seed=5, strata=strata))
    with pytest.raises(ValueError, match="distinct arrangements"):
        pkg.permuted_labels(np.array([0, 1, 1]), 0, 3, seed=0)                               # only two besides the observed one
    with pytest.raises(ValueError, match="nothing to permute"):
        pkg.permuted_labels(np.array([0, 0, 0]), 0, 3)
    with pytest.raises(ValueError, match="strata has"):
        pkg.permuted_labels(gid, 0, 3, strata=["a"])


def test_perm_null_object(pkg):
    pn = pkg.PermNull(np.array([0.5, 0.0, -0.2]), np.array([0, 4, 2], dtype=np.int32), np.array([3, 0, 1, 0], dtype=np.int32),
                      np.array([1, 0, 0, 3], dtype=np.int32), np.ones(4))
    assert pn.n_perm == 4 and pn.delta1_null is None
    assert np.array_equal(pn.p_perm, np.array([1 / 5, 5 / 5, 3 / 5]))
    assert pn.expected_false_calls() == 2.0
    assert pn.fdr_hat(8) == 0.25 and pn.fdr_hat(1) == 1.0 and pn.fdr_hat(0) == 1.0
    p = inspect.signature(pkg.Context.permutation_null).parameters
    assert list(p) == ["self", "side_a", "k", "ref_mask", "pval_deg", "padj_deg", "keep_null"]
    assert (p["k"].default, p["ref_mask"].default, p["keep_null"].default) == (0, None, False)
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        q = inspect.signature(fn).parameters
        assert q["permutations"].default is None and q["perm_seed"].default == 0 and q["perm_strata"].default is None, fn
        assert q["permutations"].kind is inspect.Parameter.KEYWORD_ONLY


@pytest.mark.parametrize("kind", ["ranks", "ties"])
def test_a_permuted_table_is_the_oracles_build_of_the_relabelled_problem(rn, kind):
    """G = 40, S = 21 (12 + 9): the restatement of the permuted semantics (sides by the row, coins keyed 0 / 1, the context's thresholds)
    equals oracle.reo_numpy.build_codes of the two-group problem with group ids 1 - row -- as they are, and with the columns put side A
    first as the GPU tests do"""
    seed = 0x5EED0C01
    X, gid = pnc.case(40, (12, 9), kind, seed)
    thr = (rn.threshold(12), rn.threshold(9))
    rows = pnc.shuffled_rows(gid, 0, 3, seed)
    if kind == "ties":
        n_eq = rn.pair_counts(X, (1 - rows[0]).astype(np.int32), 2)[1]
        assert (n_eq[:, :, 0][np.triu_indices(40, 1)] > 0).mean() > 0.3 and (n_eq[:, :, 1][np.triu_indices(40, 1)] > 0).mean() > 0.3   # coins on both sides
    tables = []
    for row in rows:
        got = pnc.permuted_codes(X, row, thr, seed)
        assert np.array_equal(got, rn.build_codes(X, (1 - row).astype(np.int32), 2, 0, thr, seed))
        X2, gid2 = pnc.relabelled(X, row)
        assert gid2[0] == 0 and np.array_equal(got, rn.build_codes(X2, gid2, 2, 0, thr, seed))
        tables.append(got)
    assert not np.array_equal(tables[0], tables[1])                                          # the labels matter
    obs = (gid == 0).astype(np.uint8)
    assert np.array_equal(pnc.permuted_codes(X, obs, thr, seed), rn.build_codes(X, gid, 2, 0, thr, seed))   # the identity row


def test_every_refusal_comes_before_any_context(pkg):
    """No GPU here: opening a context would raise a ReoError that is no DimensionMismatch."""
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    args = (["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)

    def refused(match, data=X, **kw):
        with pytest.raises(pkg.DimensionMismatch, match=match):
            pkg.run_identify_degs(data, *args, **kw)

    refused("permutations = 0", permutations=0)
    refused("together with `contrasts`", permutations=5, contrasts="all")
    refused("validity mask", permutations=5, missing="pairwise")
    refused("validity mask", permutations=5, valid=np.ones((6, 4), bool))
    refused(r"shard = \(0, 2\)", permutations=5, shard=(0, 2))
    with pytest.raises(pkg.DimensionMismatch, match="together with `contrasts`"):
        pkg.identify_degs_cells(np.ones((6, 8)), ["a"] * 4 + ["b"] * 4, names, 2, 0.01, 1.0, 0.05, None, 2, 1, permutations=3, contrasts="all")
    with pytest.raises(pkg.DimensionMismatch, match="label rows are B x S"):
        pkg._ffi.side_a_rows(np.ones((2, 5), dtype=np.uint8), 4)
    assert pkg._ffi.side_a_rows(np.array([True, False, True]), 3).tolist() == [[1, 0, 1]]


def test_writers(pkg, tmp_path):
    pn = pkg.PermNull(np.array([0.5, -0.25]), np.array([0, 3], dtype=np.int32), np.array([3, 0, 1], dtype=np.int32), np.array([1, 0, 0], dtype=np.int32),
                      np.array([0.125, 0.25, 0.5]))
    pkg.write_perm_null_tsv(str(tmp_path / "n.tsv"), ["gA", "gB"], pn)
    pkg.write_perm_summary_tsv(str(tmp_path / "s.tsv"), pn)
    assert open(tmp_path / "n.tsv").read() == "gene\tdelta1\tn_ge\tp_perm\ngA\t0.5\t0\t0.25\ngB\t-0.25\t3\t1.0\n"
    assert open(tmp_path / "s.tsv").read() == "perm\tn_up\tn_down\tse\n0\t3\t1\t0.125\n1\t0\t0\t0.25\n2\t1\t0\t0.5\n"
