"""The top partners of a gene (reo_top_partners), the parts that need no GPU: the ABI, the shared header csrc/top_partners.h under the
sanitizers (tests/top_partners_driver.cpp), the identity of the two definitions of a row -- straight from the values, and as the
subsequence of the search's order over the pairs that contain the gene (tests/top_partners_cases.py) --, the TopPartners algebra on
hand-made arrays, the plan function and the writer."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import top_pairs_cases as tpc
import top_partners_cases as tprc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry(pkg):
    header = open(os.path.join(ROOT, "include", "reo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)                          # (the comments inside the declarations hold , and ;)
    s = "reo_top_partners"
    m = re.search(r"int32_t\s+" + s + r"\s*\(([^;]*)\);", code)
    # ctx, a, b, genes, n_genes, partner_mask, m_want, partner, counts, key, n_found: the eleven of the declaration
    assert m and len(m.group(1).split(",")) == 11, m and m.group(1)
    L = pkg._ffi.lib()
    assert s in pkg._ffi.SYMBOLS and s in pkg._ffi.SIGNATURES and len(pkg._ffi.SIGNATURES[s][1]) == 11
    assert hasattr(L, s) and L.reo_version() >= 1600
    assert re.search(r"REO_NTIMINGS\s*=\s*12\b", header) and pkg._ffi.NTIMINGS == 12   # no new stage timer
    p = inspect.signature(pkg.Context.top_partners).parameters
    assert list(p) == ["self", "genes", "m", "a", "b", "partner_mask"]
    assert p["genes"].default is None and p["m"].default == 1 and p["a"].default == 0 and p["b"].default is None and p["partner_mask"].default is None
    assert pkg.TopPartners._fields == ("genes", "partner", "n_gt", "n_eq", "num", "rank_num", "n_found", "side_sizes", "a", "b")
    for method in ("best", "csr", "pairs"):
        assert callable(getattr(pkg.TopPartners, method))
    for prop in ("score", "rank_score", "direction"):
        assert isinstance(getattr(pkg.TopPartners, prop), property)
    assert {"TopPartners", "write_top_partners_tsv"} <= set(pkg.__all__)
    for fn in (pkg.run_identify_degs, pkg.identify_degs_cells, pkg.reoa):
        q = inspect.signature(fn).parameters["top_partners"]
        assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY, fn
    csrc = os.path.join(ROOT, "rankcompv3.jl_amd", "csrc")
    unit = open(os.path.join(csrc, "Makefile")).read()
    assert "toppartners.o" in unit and re.search(r"^toppartners\.o:.*top_partners\.h", unit, flags=re.M)
    shared = open(os.path.join(csrc, "top_partners.h")).read()
    assert "hip_runtime" not in shared and '#include "top_pairs.h"' in shared
    assert "subsequence of\n// reo_top_pairs' total order" in shared             # the identity with the search's order is written down


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("top_partners") / "top_partners_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                           "-I", os.path.join(ROOT, "rankcompv3.jl_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "top_partners_driver.cpp")])
    return exe


def test_cell_order_rounds_orientation_batch_and_argument_checks_under_sanitizers(driver):
    """tests/top_partners_driver.cpp: the cell at its limits, the row's order against the packed key of the search, the rounds of the
    selection against a sort, the orientation rule against a recount, the batch rule and every argument check with its message.
    AddressSanitizer and UBSan stay silent."""
    run = subprocess.run([driver], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-2000:]
    assert run.stderr == "", run.stderr[-2000:]
    lines = run.stdout.splitlines()
    assert re.fullmatch(r"ok \d+", lines[-1]), lines[-1]
    assert int(lines[-1].split()[1]) > 5000


@pytest.mark.parametrize("name", tpc.EQUALITY)
def test_a_row_from_the_values_is_the_subsequence_of_the_search(name):
    """the identity of the two definitions, on the CPU: row_oracle (O(G S) per row, D from the search's oracle) equals from_pairs for
    every gene, with all partners and with half of them"""
    X, gid, ng, a, b = tpc.case(name)
    exp = tpc.expected(name)
    G = X.shape[0]
    mask = tpc.half_mask(G)
    assert 0 < mask.sum() < G
    for pm in (None, mask):
        for q in range(G):
            direct, sub = tprc.row_oracle(X, gid, ng, a, b, exp.D, q, pm), tprc.from_pairs(exp, q, pm)
            assert tprc.same(direct, sub), (name, q, pm is not None)
            assert direct.partner.size == (G - 1 if pm is None else int(mask.sum()) - int(mask[q]))
    first = tprc.from_pairs(exp, int(exp.gene_i[0]))                               # the best pair of all leads the rows of both its genes
    assert first.partner[0] == exp.gene_j[0] and first.num[0] == exp.num[0]
    second = tprc.from_pairs(exp, int(exp.gene_j[0]))
    assert second.partner[0] == exp.gene_i[0] and second.num[0] == -exp.num[0]


def hand_made(pkg):
    """sides of 4 and 3 samples; queries 5, 2, 9 (a row without a partner) and 2 again, m = 3"""
    genes = np.array([5, 2, 9, 2], dtype=np.int32)
    partner = np.array([[2, 7, 0], [5, 8, -1], [-1, -1, -1], [5, 8, -1]], dtype=np.int32)
    n_gt = np.array([[[4, 0], [3, 0], [1, 2]], [[0, 3], [2, 0], [0, 0]], [[0, 0]] * 3, [[0, 3], [2, 0], [0, 0]]], dtype=np.int32)
    n_eq = np.array([[[0, 0], [1, 1], [1, 0]], [[0, 0], [0, 1], [0, 0]], [[0, 0]] * 3, [[0, 0], [0, 1], [0, 0]]], dtype=np.int32)
    sizes = np.array([4, 3], dtype=np.int64)
    w = 2 * n_gt.astype(np.int64) + n_eq - sizes                                 # gt - lt per side
    num = w[:, :, 0] * 3 - w[:, :, 1] * 4
    found = np.array([3, 2, 0, 2], dtype=np.int32)
    num[np.arange(3)[None, :] >= found[:, None]] = 0
    gam = np.array([[9, 5, 7], [9, 1, 0], [0, 0, 0], [9, 1, 0]], dtype=np.int64)
    return pkg.TopPartners(genes, partner, n_gt, n_eq, num, gam, found, sizes, 0, None)


def test_the_algebra_on_hand_made_arrays(pkg):
    tp = hand_made(pkg)
    assert tp.num.tolist() == [[24, 17, -7], [-24, 8, 0], [0, 0, 0], [-24, 8, 0]]
    assert np.array_equal(tp.score, np.abs(tp.num) / 24.0) and tp.score[2].tolist() == [0.0, 0.0, 0.0]
    assert np.array_equal(tp.rank_score, tp.rank_num / 24.0)
    assert tp.direction.dtype == np.int8 and tp.direction.tolist() == [[1, 1, -1], [-1, 1, 0], [0, 0, 0], [-1, 1, 0]]
    bp, bs = tp.best()
    assert bp.dtype == np.int32 and bp.tolist() == [2, 5, -1, 5] and bs.tolist() == [1.0, 1.0, 0.0, 1.0]
    g, rowptr, pa = tp.csr()
    assert g.dtype == np.int32 and rowptr.dtype == np.int64 and pa.dtype == np.int32
    assert g.tolist() == [5, 2, 9, 2] and rowptr.tolist() == [0, 3, 5, 5, 7] and pa.tolist() == [2, 7, 0, 5, 8, 5, 8]
    pairs = tp.pairs()
    assert isinstance(pairs, pkg.TopPairs) and pairs.passes == 0 and (pairs.a, pairs.b) == (0, None)
    # (2, 5) is listed three times -- from 5 and twice from 2 -- and kept once; |N| 24, 17, 8, 7; (5, 2) and (5, 0) are re-oriented
    assert pairs.gene_i.tolist() == [2, 5, 2, 0] and pairs.gene_j.tolist() == [5, 7, 8, 5]
    assert pairs.num.tolist() == [-24, 17, 8, 7] and pairs.rank_num.tolist() == [9, 5, 1, 7]
    assert pairs.n_gt.tolist() == [[0, 3], [3, 0], [2, 0], [2, 1]] and pairs.n_eq.tolist() == [[0, 0], [1, 1], [0, 1], [1, 0]]
    assert pairs.n_gt.dtype == np.int32 and pairs.num.dtype == np.int64 and pairs.gene_i.dtype == np.int32
    w = 2 * pairs.n_gt.astype(np.int64) + pairs.n_eq - tp.side_sizes             # the re-oriented counts give the re-oriented N
    assert np.array_equal(w[:, 0] * 3 - w[:, 1] * 4, pairs.num)
    assert pairs.disjoint(3).tolist() == [0]                                     # every further pair holds gene 2 or gene 5
    far = tp._replace(partner=np.where(tp.partner == 8, 1, np.where(tp.partner == 7, 3, tp.partner)))   # (5, 3) still holds 5; (1, 2) holds 2
    assert far.pairs().gene_i.tolist() == [2, 3, 1, 0] and far.pairs().disjoint(3).tolist() == [0]
    free = tp._replace(genes=np.array([5, 4, 9, 4], dtype=np.int32), partner=np.where(tp.partner == 5, 6, tp.partner))
    assert free.pairs().gene_i.tolist() == [2, 4, 5, 4, 0] and free.pairs().gene_j.tolist() == [5, 6, 7, 8, 5]   # (4, 6): twice listed, once kept
    assert free.pairs().disjoint(3).tolist() == [0, 1]                           # (2, 5), (4, 6); (5, 7), (4, 8) and (0, 5) hold a used gene
    assert pairs.csr()[0].tolist() == [2, 5, 2, 0]
    empty = tp._replace(genes=tp.genes[:0], partner=tp.partner[:0], n_gt=tp.n_gt[:0], n_eq=tp.n_eq[:0], num=tp.num[:0], rank_num=tp.rank_num[:0],
                        n_found=tp.n_found[:0])
    assert empty.pairs().gene_i.size == 0 and empty.pairs().n_gt.shape == (0, 2) and empty.best()[0].size == 0
    assert empty.csr()[1].tolist() == [0] and empty.csr()[2].size == 0


def test_the_plan_refuses_before_a_context_is_opened(pkg, tmp_path):
    plan = pkg.hotpath.top_partners_plan
    assert plan(None) is None and plan(1) is None and plan(np.int64(1024)) is None and plan(None, masked=True, shard=(0, 2)) is None
    for bad in (0, -1, 1025, 2.5, "3", True):
        with pytest.raises(pkg.DimensionMismatch, match="top_partners = .*between 1 and 1024"):
            plan(bad)
    with pytest.raises(pkg.DimensionMismatch, match="top_partners: .*validity mask"):
        plan(3, masked=True)
    with pytest.raises(pkg.DimensionMismatch, match="top_partners: the search has no sharded form"):
        plan(3, shard=(1, 2))
    names = [f"g{i}" for i in range(6)]
    X = np.arange(24, dtype=np.float64).reshape(6, 4)
    args = (X, ["a", "a", "b", "b"], names, 0.01, 1.0, 0.05, np.ones(6, bool), 2, 1)
    with pytest.raises(pkg.DimensionMismatch, match="top_partners = 1025"):      # before any context is opened: there is no GPU here
        pkg.run_identify_degs(*args, top_partners=1025)
    with pytest.raises(pkg.DimensionMismatch, match="top_partners: .*validity mask"):
        pkg.run_identify_degs(*args, top_partners=3, valid=np.ones((6, 4), dtype=bool))
    with pytest.raises(pkg.DimensionMismatch, match="top_partners: .*validity mask"):
        pkg.run_identify_degs(*args, top_partners=3, missing="pairwise")
    with pytest.raises(pkg.DimensionMismatch, match="top_partners: the search has no sharded form"):
        pkg.run_identify_degs(*args, top_partners=3, shard=(0, 2))
    with pytest.raises(pkg.DimensionMismatch, match="top_partners = 0"):
        pkg.identify_degs_cells(X, ["a", "a", "b", "b"], names, 1, 0.01, 1.0, 0.05, None, 2, 1, top_partners=0)
    with pytest.raises(pkg.DimensionMismatch, match="top_partners = 0"):
        pkg.reoa(str(tmp_path / "no_such_expr.txt"), str(tmp_path / "no_such_meta.txt"), work_dir=str(tmp_path), top_partners=0)
    assert os.listdir(tmp_path) == []


def test_the_writer_byte_for_byte(pkg, tmp_path):
    tp = hand_made(pkg)
    out = tmp_path / "partners.tsv"
    pkg.write_top_partners_tsv(str(out), [f"g{i}" for i in range(10)], tp)
    assert out.read_bytes() == (b"gene\trank\tpartner\tnum\tscore\trank_num\tgt_A\teq_A\tgt_B\teq_B\n"
                                b"g5\t1\tg2\t24\t1.0\t9\t4\t0\t0\t0\n"
                                b"g5\t2\tg7\t17\t0.7083333333333334\t5\t3\t1\t0\t1\n"
                                b"g5\t3\tg0\t-7\t0.2916666666666667\t7\t1\t1\t2\t0\n"
                                b"g2\t1\tg5\t-24\t1.0\t9\t0\t0\t3\t0\n"
                                b"g2\t2\tg8\t8\t0.3333333333333333\t1\t2\t0\t0\t1\n"
                                b"g2\t1\tg5\t-24\t1.0\t9\t0\t0\t3\t0\n"
                                b"g2\t2\tg8\t8\t0.3333333333333333\t1\t2\t0\t0\t1\n")
