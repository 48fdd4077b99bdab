"""Pairwise group contrasts (reo_build_pairs_contrast), the parts that need no GPU: the ABI, the argument checks and derived sides of
csrc/contrast.h under the sanitizers, parse_contrasts, the file and column names of the writers from a hand-made run, and
PairSupport.delta(k, other)."""
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    s = "reo_build_pairs_contrast"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    assert m, s
    assert [a.strip() for a in m.group(1).split(",")] == ["reo_ctx *ctx", "int32_t ctrl", "int32_t treat"]
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 3
    assert hasattr(L, s)
    assert L.reo_version() >= 900
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    assert list(inspect.signature(pkg.Context.build_contrast).parameters) == ["self", "ctrl", "treat"]
    # a null context is refused by the library itself, with a message that names the function
    assert L.reo_build_pairs_contrast(None, 0, 1) == pkg._ffi.REO_EINVAL
    assert L.reo_last_error().decode() == "reo_build_pairs_contrast: null context"


def test_contrasts_keyword_defaults_to_none(pkg):
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        p = inspect.signature(fn).parameters["contrasts"]
        assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert "parse_contrasts" in pkg.__all__


def test_argument_checks_and_derived_sides_under_sanitizers(tmp_path):
    """tests/contrast_driver.cpp: contrast_check_args, every check with its message and their order; contrast_sides for interleaved labels,
    groups of 1, 31, 32 and 33 samples, and 70 groups.  AddressSanitizer and UBSan stay silent."""
    exe = str(tmp_path / "contrast_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "contrast_driver.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    # 3 + 4 + 70 groups: 6 + 12 + 4830 ordered contrasts, seven checks each
    assert int(lines[-1].split()[1]) > 7 * (6 + 12 + 4830)
    msgs = [l.split(" ", 2) for l in lines if l.startswith("msg ")]
    assert sorted({int(m[1]) for m in msgs}) == list(range(1, 10))               # every refusal was printed ...
    assert all(m[2].startswith("reo_build_pairs_contrast: ") for m in msgs)      # ... and names the function
    by_no = {int(m[1]): m[2] for m in msgs}
    assert "65535 samples" in by_no[7] and "REO_SHARE_GROUP_COUNTS=0" in by_no[8] and "123456789012 bytes" in by_no[9]
    sides = [l.split()[1:] for l in lines if l.startswith("sides ")]
    # blocks summed over every ordered contrast: each group's blocks appear 2 (C - 1) times
    blocks70 = 2 * 69 * sum((n + 31) // 32 for n in range(1, 71))
    assert sides == [["interleaved", "3", "45", str(2 * 2 * 3)], ["block_edges", "4", "97", str(2 * 3 * 5)], ["seventy", "70", "2485", str(blocks70)]]


def test_parse_contrasts(pkg):
    pc = pkg.parse_contrasts
    assert pc(["w", "x", "y", "z"], "all") == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert pc(["a", "b"], "all") == [(0, 1)]
    assert pc(["ctl", "A", "B"], [("A", "ctl"), ("B", "ctl"), ("A", "B")]) == [(1, 0), (2, 0), (1, 2)]
    assert pc(["ctl", "A", "B"], [["ctl", "B"], ("B", "ctl")]) == [(0, 2), (2, 0)]   # the mirrored contrast is another contrast
    assert pc([1, 2, 3], [(np.int64(3), 1)]) == [(2, 0)]
    DM = pkg.DimensionMismatch
    with pytest.raises(DM, match=r"contrasts: unknown level 'D' \(the levels of 'group' are \['ctl', 'A', 'B'\]\)"):
        pc(["ctl", "A", "B"], [("ctl", "A"), ("ctl", "D")])
    with pytest.raises(DM, match="contrasts: ctrl == treat == 'A', a contrast needs two different levels"):
        pc(["ctl", "A", "B"], [("A", "A")])
    with pytest.raises(DM, match="contrasts: the list is empty"):
        pc(["ctl", "A", "B"], [])
    with pytest.raises(DM, match=r"contrasts: \('ctl', 'A'\) is listed twice"):
        pc(["ctl", "A", "B"], [("ctl", "A"), ("B", "A"), ("ctl", "A")])
    with pytest.raises(DM, match="is not \"all\""):
        pc(["ctl", "A", "B"], "every")
    with pytest.raises(DM, match="is not a .ctrl, treat. pair"):
        pc(["ctl", "A", "B"], [("ctl", "A", "B")])


def test_contrasts_are_refused_before_any_context(pkg, tmp_path):
    """No GPU here: opening a context would raise a ReoError that is no DimensionMismatch."""
    names = [f"g{i}" for i in range(6)]
    X = np.arange(36, dtype=np.float64).reshape(6, 6)
    grp = ["a", "a", "b", "b", "c", "c"]
    with pytest.raises(pkg.DimensionMismatch, match="contrasts: unknown level 'd'"):
        pkg.run_identify_degs(X, grp, names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1, contrasts=[("a", "d")])
    with pytest.raises(pkg.DimensionMismatch, match="contrasts: the list is empty"):
        pkg.run_identify_degs(X, grp, names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1, contrasts=[])
    with pytest.raises(pkg.DimensionMismatch, match="contrasts: ctrl == treat == 'b'"):
        pkg.identify_degs_cells(X, grp, names, 1, 0.01, 1.0, 0.05, None, 2, 1, contrasts=[("b", "b")])


def hand_made_run(pkg, with_extras):
    G, S = 4, 6
    genes = ["A1BG", "TP53", "g3", "g4"]
    samples = [f"s{q}" for q in range(S)]
    groups = ["ctl", "ctl", "trtA", "trtA", "trtB", "trtB"]
    rng = np.random.default_rng(1)
    comps = []
    for k, c, t in ((0, "ctl", "trtA"), (0, "ctl", "trtB"), (2, "trtB", "trtA")):
        res = rng.random((G, 15))
        cm = {"k": k, "ctrl": c, "treat": t, "result": res, "labels": np.array(["up", "no change", "down", "no change"], dtype=object),
              "iters_run": 1, "trace": [(2, 2)]}
        if with_extras:
            pl = pkg.PairList(np.array([0, 2], dtype=np.int32), np.array([0, 1, 2], dtype=np.int64), np.array([1, 3], dtype=np.int32),
                              np.array([2, 6], dtype=np.uint8))
            z = np.ones((2, S), dtype=np.int32)
            cm["pairs"] = pl
            cm["pair_support"] = pkg.PairSupport(pl.genes, pl.rowptr, pl.partner, pl.code, np.array([[2, 0, 1], [0, 2, 2]], dtype=np.int32),
                                                 np.zeros((2, 3), dtype=np.int32), None, np.array([2, 2, 2], dtype=np.int64))
            cm["sample_scores"] = pkg.SampleScores(pl.genes, np.array([1, 1], dtype=np.int32), z, 0 * z, 0 * z)
        comps.append(cm)
    run = pkg.DegRun(result=comps[0]["result"], labels=comps[0]["labels"], levels=["ctl", "trtA", "trtB"], thresholds=np.zeros((2, 3), np.int32),
                     iters_run=1, trace=[(2, 2)], comparisons=comps, gene_names=genes)
    prep = {"data": np.arange(G * S, dtype=np.int64).reshape(G, S), "sample_names": samples, "sample_groups": groups, "gene_names": genes,
            "g_name": ["ctl", "trtA", "trtB"], "ref": np.ones(G, bool), "meta": None}
    return run, prep


def test_writers_name_files_and_columns_by_ctrl_and_treat(pkg, tmp_path):
    reoa_mod = sys.modules[pkg.__name__ + ".reoa"]   # (pkg.reoa is the function)
    run, prep = hand_made_run(pkg, with_extras=True)
    assert run.res.shape == (4, 1 + 16 * 3)
    df = reoa_mod.write_outputs("expr", prep, run, str(tmp_path))
    assert list(df.columns) == ["gene_name", "ctl_vs_trtA", "ctl_vs_trtB", "trtB_vs_trtA"]   # <ctrl>_vs_<treat>, the two-group naming (:683)
    extra = reoa_mod.write_extras("expr", prep, run, str(tmp_path))
    want = {"expr_df_expr.tsv", "expr_df_meta.tsv", "expr_gene_up_down.tsv"}
    for fg in ("ctl_trtA", "ctl_trtB", "trtB_trtA"):                               # <stem>_<ctrl>_<treat>_result.tsv (:670)
        want |= {f"expr_{fg}_result.tsv", f"expr_{fg}_pairs.tsv", f"expr_{fg}_pair_support.tsv", f"expr_{fg}_sample_scores.tsv"}
    assert set(os.listdir(tmp_path)) == want
    assert sorted(os.path.basename(p) for p in extra) == sorted(f for f in want if f.endswith(("_pairs.tsv", "_pair_support.tsv", "_sample_scores.tsv")))
    head = (tmp_path / "expr_gene_up_down.tsv").read_text().split("\n")[0]
    assert head == "gene_name\tctl_vs_trtA\tctl_vs_trtB\ttrtB_vs_trtA"
    lines = (tmp_path / "expr_trtB_trtA_result.tsv").read_text().split("\n")
    assert lines[0].split("\t")[0] == "genename" and lines[1].split("\t")[0] == "A1BG" and lines[1].split("\t")[-1] == "up"
    assert float(lines[1].split("\t")[1]) == run.comparisons[2]["result"][0, 0]
    assert (tmp_path / "expr_ctl_trtB_pairs.tsv").read_bytes() == b"gene\tpartner\tclass\nA1BG\tTP53\tn13\ng3\tg4\tn31\n"
    # without the extras no further file; one-vs-rest and two-group runs keep their names
    run2, prep2 = hand_made_run(pkg, with_extras=False)
    assert reoa_mod.write_extras("expr", prep2, run2, str(tmp_path / "none")) == []
    assert reoa_mod.fg_name(["a", "b", "c"], {"k": 1}) == "b" and reoa_mod.fg_name(["a", "b"], {"k": 0}) == "a_b"
    assert reoa_mod.fg_name(["a", "b"], {"k": 1, "ctrl": "b", "treat": "a"}) == "b_a"


def test_pair_support_delta_against_one_other_group(pkg):
    # three groups of unequal size: 2, 3 and 5 samples
    ps = pkg.PairSupport(np.array([0, 4], dtype=np.int32), np.array([0, 1, 3], dtype=np.int64), np.array([1, 2, 3], dtype=np.int32), None,
                         np.array([[2, 3, 0], [1, 0, 4], [0, 3, 5]], dtype=np.int32), None, None, np.array([2, 3, 5], dtype=np.int64))
    assert ps.delta(0, 1).tolist() == [2 / 2 - 3 / 3, 1 / 2 - 0 / 3, 0 / 2 - 3 / 3]
    assert ps.delta(0, 2).tolist() == [2 / 2 - 0 / 5, 1 / 2 - 4 / 5, 0 / 2 - 5 / 5]
    assert ps.delta(2, 1).tolist() == [0 / 5 - 3 / 3, 4 / 5 - 0 / 3, 5 / 5 - 3 / 3]
    assert np.array_equal(ps.delta(1, 0), -ps.delta(0, 1)) and ps.delta(0, 1).dtype == np.float64
    assert np.array_equal(ps.delta(0, other=2), ps.delta(0, 2))
    # the default is the comparison against ALL other samples, as before
    assert ps.delta(0).tolist() == [2 / 2 - 3 / 8, 1 / 2 - 4 / 8, 0 / 2 - 8 / 8] and np.array_equal(ps.delta(0, None), ps.delta(0))
    assert not np.array_equal(ps.delta(0), ps.delta(0, 1))
    for k, o in ((0, 0), (0, 3), (0, -1), (3, 0)):
        with pytest.raises(pkg.DimensionMismatch):
            ps.delta(k, o)
