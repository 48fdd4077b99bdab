"""The label-permutation null on the GPU (reo_perm_null, reo_perm_codes; csrc/permpairs.hip).  Every check is an exact equality.  The
comparison side is the existing, oracle-pinned path: a second two-group context with the same seed and group ids 1 - row (its columns put
side A first, because the library numbers group ids in order of first appearance; a class table does not depend on the order of the
columns inside a side: tests/perm_null_cases.py, relabelled), then build_pairs(0), get_codes and identify_degs(ref_mask, n_iter = 1).

The tables of a BATCH are not handed out by the library.  A table behind the first is looked at whole through the REO_PERM_CODES_SLOT test
seam of reo_perm_codes; beyond that they are held to the relabelled build through what a pass makes of them: with a reference set of all
genes every pair's class enters the tallies of both its genes, and delta1_null must equal the relabelled context's delta1 bit for bit, for
every permutation of batches that cross the launch-group width (16) and the batch width."""
import os

import numpy as np
import pytest

import perm_null_cases as pnc

pytestmark = pytest.mark.gpu

PVAL_DEG, PADJ_DEG = 0.2, 0.9   # wide, so that permutations call genes and n_up / n_down are not all zero


def open_ctx(pkg, X, gid, seed, build_k=None, pval_reo=0.01):
    ctx = pkg.Context(device=0, seed=seed)
    ctx.set_groups(gid, int(np.max(gid)) + 1)
    ctx.compute_thresholds(pval_reo)
    ctx.set_matrix(X)
    if build_k is not None:
        ctx.build_pairs(build_k)
    return ctx


class Relabelled:
    """one context for all relabelled problems of a test: new groups and matrix per row"""

    def __init__(self, pkg, seed):
        self.ctx = pkg.Context(device=0, seed=seed)

    def build(self, X, row, pval_reo=0.01):
        X2, gid2 = pnc.relabelled(X, row)
        self.ctx.set_groups(gid2, 2)
        self.ctx.compute_thresholds(pval_reo)
        self.ctx.set_matrix(X2)
        self.ctx.build_pairs(0)

    def codes(self, X, row, rect=None):
        """the whole table, or the rectangle (i0, i1, j0, j1) of it"""
        self.build(X, row)
        G = X.shape[0]
        return self.ctx.get_codes(*(rect if rect is not None else (0, G, 0, G)))

    def one_pass(self, X, row, ref, pval_deg=PVAL_DEG, padj_deg=PADJ_DEG):
        self.build(X, row)
        return self.ctx.identify_degs(ref, pval_deg, padj_deg, 1, 0)[0]

    def close(self):
        self.ctx.close()


@pytest.fixture
def rel(pkg):
    made = []

    def make(seed):
        made.append(Relabelled(pkg, seed))
        return made[-1]
    yield make
    for r in made:
        r.close()


def check_codes(pkg, rel, X, gid, seed, k=0, n_rows=2):
    G = X.shape[0]
    r = rel(seed)
    rows = pnc.shuffled_rows(gid, k, n_rows, seed + 1)
    with open_ctx(pkg, X, gid, seed) as ctx:
        for row in rows:
            got = ctx.perm_codes(row, k=k)
            want = r.codes(X, row)
            assert got.shape == (G, G) and np.array_equal(got, want), (int((got != want).sum()), row.tolist())
        strip = ctx.perm_codes(rows[0], k, G // 3, G // 3 + 5, 1, G - 1)            # a rectangle off the origin
        assert np.array_equal(strip, r.codes(X, rows[0])[G // 3: G // 3 + 5, 1: G - 1])
    return rows


@pytest.mark.parametrize("G,sizes,kind", [(70, (12, 9), "ties"), (1100, (12, 9), "ranks"), (70, (32, 64), "ties"), (70, (1, 20), "ties")])
def test_perm_codes_equal_the_relabelled_build(pkg, rel, G, sizes, kind):
    """a column tile seam with ties on both sides; several column tiles, a second 1024-gene pad and a row-tile remainder (tie-free kernel,
    the relabelled build runs in slot order); groups of exactly 32 and 64 samples; a side of one sample"""
    seed = 0x5EED0C10 + G + sizes[0]
    X, gid = pnc.case(G, sizes, kind, seed)
    check_codes(pkg, rel, X, gid, seed)
    if sizes == (12, 9):
        check_codes(pkg, rel, X, gid, seed, k=1, n_rows=1)


@pytest.mark.parametrize("kind,dtype", [("counts", np.int64), ("ties", np.float64), ("ties", np.float32)])
def test_perm_codes_dtypes(pkg, rel, kind, dtype):
    seed = 0x5EED0C20
    X, gid = pnc.case(70, (12, 9), kind, seed, dtype=dtype)
    assert X.dtype == dtype
    check_codes(pkg, rel, X, gid, seed, n_rows=1)


@pytest.mark.parametrize("slot", [5, 17])
@pytest.mark.parametrize("kind", ["ties", "ranks"])
def test_tables_behind_the_first_of_a_batch(pkg, rel, monkeypatch, slot, kind):
    """REO_PERM_CODES_SLOT: the permutation is built as table `slot` of a batch whose other tables hold rotations of the row -- a table
    behind the first, and one in the second launch group of 16 -- and its whole table equals the relabelled build"""
    monkeypatch.setenv("REO_PERM_CODES_SLOT", str(slot))
    seed = 0x5EED0C28 + slot
    X, gid = pnc.case(70, (12, 9), kind, seed)
    check_codes(pkg, rel, X, gid, seed)


def planted(G, sizes, seed, kind="ties"):
    X, gid = pnc.case(G, sizes, kind, seed)
    X = X.copy(order="F")
    X[: G // 10, gid == 0] += 2.5 if kind == "ties" else 0.0
    return X, gid


def check_null_against_relabelled(pkg, rel, X, gid, seed, k, rows, ref, keep=None):
    """keep: a rectangle (i0, i1, j0, j1) of the resident table that is read before the call and must read the same after it"""
    G = X.shape[0]
    r = rel(seed)
    with open_ctx(pkg, X, gid, seed, build_k=k) as ctx:
        before = ctx.get_codes(*keep) if keep is not None else None
        pn = ctx.permutation_null(rows, k=k, ref_mask=ref, pval_deg=PVAL_DEG, padj_deg=PADJ_DEG, keep_null=True)
        info = ctx.info()
        if keep is not None:
            assert np.array_equal(ctx.get_codes(*keep), before), "the resident table changed under reo_perm_null"
    assert pn.delta1_null.shape == (rows.shape[0], G)
    called = 0
    for p, row in enumerate(rows):
        res = r.one_pass(X, row, ref)
        assert np.array_equal(pn.delta1_null[p], res[:, 11]), (p, int((pn.delta1_null[p] != res[:, 11]).sum()))
        lab = pkg.label_genes(res, PVAL_DEG, PADJ_DEG)
        assert (int(pn.n_up[p]), int(pn.n_down[p])) == (int((lab == "up").sum()), int((lab == "down").sum())), p
        assert pn.se_null[p] == res[0, 13], p
        called += int(pn.n_up[p]) + int(pn.n_down[p])
    assert np.array_equal(pn.n_ge, (np.abs(pn.delta1_null) >= np.abs(pn.delta1_obs)[None, :]).sum(axis=0))
    return pn, info, called


@pytest.mark.parametrize("cap,n_perm", [(3, 4), (3, 9), (17, 18)])
def test_batch_seams(pkg, rel, monkeypatch, cap, n_perm):
    """REO_PERM_BATCH forces the batch width P: n_perm = P + 1 and 2 P + 3 at P = 3, and P = 17 > one launch group of 16 with one
    permutation left for a second batch.  G = 200, tie-rich, all genes in the reference set."""
    monkeypatch.setenv("REO_PERM_BATCH", str(cap))
    seed = 0x5EED0C30
    X, gid = planted(200, (12, 9), seed)
    rows = pkg.permuted_labels(gid, 0, n_perm, seed=cap)
    pn, info, called = check_null_against_relabelled(pkg, rel, X, gid, seed, 0, rows, np.ones(200, dtype=bool))
    assert info["perm_batch"] == cap and info["perm_kernel_us"] > 0
    assert called > 0                                                                # the counts of calls are exercised


def test_identity_row(pkg):
    """side_a = the observed labels of a two-group context: the resident table, the observed delta1, and n_ge >= 1 everywhere"""
    seed = 0x5EED0C40
    X, gid = planted(200, (12, 9), seed)
    obs = (gid == 0).astype(np.uint8)
    ref = np.ones(200, dtype=bool)
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        assert np.array_equal(ctx.perm_codes(obs), ctx.get_codes(0, 200, 0, 200))
        rows = np.stack([obs, pnc.shuffled_rows(gid, 0, 1, 5)[0]])
        pn = ctx.permutation_null(rows, ref_mask=ref, keep_null=True)
        assert np.array_equal(pn.delta1_null[0], pn.delta1_obs) and (pn.n_ge >= 1).all()
        res = ctx.identify_degs(ref, 1.0, 0.05, 1, 0)[0]
        assert np.array_equal(pn.delta1_obs, res[:, 11]) and pn.se_null[0] == res[0, 13]


def test_n_ge_is_the_numpy_count(pkg):
    """B = 40, G = 300, tie-free; the default batch (one batch of 40: three launch groups, the last ragged)"""
    seed = 0x5EED0C50
    X, gid = pnc.case(300, (12, 9), "ranks", seed)
    rows = pkg.permuted_labels(gid, 0, 40, seed=1)
    ref = np.zeros(300, dtype=bool)
    ref[::3] = True
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        pn = ctx.permutation_null(rows, ref_mask=ref, keep_null=True)
        assert ctx.info()["perm_batch"] == 40
    want = (np.abs(pn.delta1_null) >= np.abs(pn.delta1_obs)[None, :]).sum(axis=0)
    assert np.array_equal(pn.n_ge, want) and pn.n_ge.dtype == np.int32
    assert 0 < want.min() + 1 and want.max() <= 40 and len(np.unique(want)) > 5
    assert np.array_equal(pn.p_perm, (1.0 + want) / 41.0)
    assert len({d.tobytes() for d in pn.delta1_null}) == 40                          # forty different tables


def test_three_groups_k1(pkg, rel):
    """a three-group context, k = 1: the permuted tables are two-group tables, one coin stream per side"""
    seed = 0x5EED0C60
    X, gid = pnc.case(70, (10, 12, 9), "ties", seed)
    rows = check_codes(pkg, rel, X, gid, seed, k=1)
    assert rows.sum(axis=1).tolist() == [12, 12]
    check_null_against_relabelled(pkg, rel, X, gid, seed, 1, pkg.permuted_labels(gid, 1, 3, seed=2), np.ones(70, dtype=bool))


def test_state_after_the_call(pkg):
    seed = 0x5EED0C70
    X, gid = planted(200, (12, 9), seed)
    ref0 = np.zeros(200, dtype=bool)
    ref0[20:120] = True
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        before = ctx.get_codes(0, 200, 0, 200)
        run_before = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        ref = ctx.ref_mask()
        pn = ctx.permutation_null(pkg.permuted_labels(gid, 0, 5, seed=3))            # ref_mask=None: fetched before the call
        assert np.array_equal(pn.delta1_obs, ctx.identify_degs(ref, 1.0, 0.05, 1, 0)[0][:, 11])
        assert np.array_equal(ctx.get_codes(0, 200, 0, 200), before)
        ctx.permutation_null(pkg.permuted_labels(gid, 0, 2, seed=4), ref_mask=ref)
        with pytest.raises(pkg.DimensionMismatch, match="reo_perm_null has run"):
            ctx.ref_mask()
        run_after = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert np.array_equal(run_after[0], run_before[0]) and run_after[1:] == run_before[1:]
        assert np.array_equal(ctx.ref_mask(), ref)
        assert np.array_equal(ctx.get_codes(0, 200, 0, 200), before)


def raw_null(pkg, ctx, rows, k=0, ref="ok", n_perm=None, null_out=None):
    """reo_perm_null through ctypes, so that null pointers and a wrong n_perm can be passed"""
    f = pkg._ffi
    G = ctx.G
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    refb = np.ones(G, dtype=np.uint8)
    B = rows.shape[0] if n_perm is None else n_perm
    n = max(B, 1)
    d, nge, up, dn, se = np.zeros(G), np.zeros(G, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
    out = {"delta1_obs": f._ptr(d), "n_ge": f._ptr(nge), "n_up": f._ptr(up), "n_down": f._ptr(dn), "se_null": f._ptr(se)}
    if null_out:
        out[null_out] = None
    f.check(ctx._L.reo_perm_null(ctx._h, k, f._ptr(rows) if rows.size else None, B, f._ptr(refb) if ref == "ok" else None, 1.0, 0.05,
                                 out["delta1_obs"], out["n_ge"], out["n_up"], out["n_down"], out["se_null"], None))


REFUSALS = ["null side_a", "null ref_mask", "null n_ge", "count of ones", "byte 2", "n_perm 0", "k out of range", "no table of k", "mask set"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_leave_the_table_intact(pkg, what):
    seed = 0x5EED0C80
    X, gid = pnc.case(70, (10, 12, 9), "ties", seed)
    rows = pnc.shuffled_rows(gid, 0, 2, 1)
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        before = ctx.get_codes(0, 70, 0, 70)
        ref = np.ones(70, dtype=bool)
        ctx.identify_degs(ref, 1.0, 0.05, 1, 0)
        DM = pkg.DimensionMismatch
        if what == "null side_a":
            with pytest.raises(DM, match="must not be null"):
                raw_null(pkg, ctx, np.zeros((0, 31), np.uint8), n_perm=2)
        elif what == "null ref_mask":
            with pytest.raises(DM, match="must not be null"):
                raw_null(pkg, ctx, rows, ref=None)
        elif what == "null n_ge":
            with pytest.raises(DM, match="must not be null"):
                raw_null(pkg, ctx, rows, null_out="n_ge")
        elif what == "count of ones":
            bad = rows.copy()
            bad[1, np.flatnonzero(bad[1] == 0)[0]] = 1
            with pytest.raises(DM, match="row 1 of side_a has 11 ones, side A of the comparison has 10 samples"):
                ctx.permutation_null(bad, ref_mask=ref)
            with pytest.raises(DM, match="reo_perm_codes: row 0 of side_a has 11 ones"):
                ctx.perm_codes(bad[1])
        elif what == "byte 2":
            bad = rows.copy()
            bad[0, 3] = 2
            with pytest.raises(DM, match="row 0 of side_a holds the byte 2 in column 3"):
                ctx.permutation_null(bad, ref_mask=ref)
        elif what == "n_perm 0":
            with pytest.raises(DM, match="n_perm = 0"):
                raw_null(pkg, ctx, rows, n_perm=0)
        elif what == "k out of range":
            with pytest.raises(DM, match=r"comparison 3 outside \[0,3\)"):
                ctx.permutation_null(rows, k=3, ref_mask=ref)
        elif what == "no table of k":
            with pytest.raises(DM, match="no class table of comparison 1 is resident"):
                ctx.permutation_null(pnc.shuffled_rows(gid, 1, 2, 1), k=1, ref_mask=ref)
        elif what == "mask set":
            ctx.set_valid_mask(np.ones(X.shape, dtype=bool))
            with pytest.raises(DM, match="reo_perm_null compares on the bit planes .* validity mask"):
                ctx.permutation_null(rows, ref_mask=ref)
            with pytest.raises(DM, match="reo_perm_codes compares on the bit planes"):
                ctx.perm_codes(rows[0])
            ctx.set_valid_mask(None)
        assert np.array_equal(ctx.get_codes(0, 70, 0, 70), before)
        assert np.array_equal(ctx.ref_mask(), ref)                                  # a refused call has not touched the iteration's buffers


def test_refused_without_thresholds_or_table(pkg):
    seed = 0x5EED0C81
    X, gid = pnc.case(70, (12, 9), "ties", seed)
    rows = pnc.shuffled_rows(gid, 0, 2, 1)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="thresholds not set"):
            ctx.permutation_null(rows, ref_mask=np.ones(70, bool))
        with pytest.raises(pkg.DimensionMismatch, match="thresholds not set"):
            ctx.perm_codes(rows[0])
        ctx.compute_thresholds(0.01)
        with pytest.raises(pkg.DimensionMismatch, match="no class table of comparison 0 is resident"):
            ctx.permutation_null(rows, ref_mask=np.ones(70, bool))
        ctx.build_pairs(0)
        before = ctx.get_codes(0, 70, 0, 70)
        ctx.set_valid_mask(np.ones(X.shape, dtype=bool))
        ctx.build_pairs_masked(0)
        ctx.set_valid_mask(None)                                                     # no mask any more, but the resident table is a masked one
        with pytest.raises(pkg.DimensionMismatch, match="a contrast or masked table does not count"):
            ctx.permutation_null(rows, ref_mask=np.ones(70, bool))
        ctx.build_pairs(0)
        assert np.array_equal(ctx.get_codes(0, 70, 0, 70), before)


def test_sharded_and_multi_contexts_are_refused(pkg, monkeypatch):
    seed = 0x5EED0C82
    X, gid = pnc.case(70, (12, 9), "ties", seed)
    rows = pnc.shuffled_rows(gid, 0, 2, 1)
    with open_ctx(pkg, X, gid, seed, build_k=0) as ctx:
        ctx.set_shard(0, 2)
        with pytest.raises(pkg.DimensionMismatch, match="reo_perm_null is not available on a sharded context"):
            ctx.permutation_null(rows, ref_mask=np.ones(70, bool))
        with pytest.raises(pkg.DimensionMismatch, match="reo_perm_codes is not available on a sharded context"):
            ctx.perm_codes(rows[0])
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=seed, n_gpus=2) as ctx:
        ctx.set_groups(gid, 2)
        ctx.compute_thresholds(0.01)
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_perm_null is not available on a reo_create_multi context"):
            ctx.permutation_null(rows, ref_mask=np.ones(70, bool))


@pytest.mark.parametrize("G,S", [(65536, 6), (64, 65536)])
def test_sizes_above_the_16_plane_layout_are_refused(pkg, G, S):
    """nothing is built: the size checks come before the thresholds and the table are looked at"""
    X = np.asfortranarray(np.arange(G * S, dtype=np.float32).reshape(G, S) % 977)
    gid = np.array([0, 1] * (S // 2), dtype=np.int32)
    rows = pnc.shuffled_rows(gid, 0, 1, 1)
    with pkg.Context(device=0, seed=1) as ctx:
        ctx.set_matrix(X)
        ctx.set_groups(gid, 2)
        with pytest.raises(pkg.DimensionMismatch, match="at most 65535 (genes|samples)"):
            ctx.permutation_null(rows, ref_mask=np.ones(G, bool))
        with pytest.raises(pkg.DimensionMismatch, match="at most 65535 (genes|samples)"):
            ctx.perm_codes(rows[0], 0, 0, 4, 0, 4)


def test_end_to_end(pkg, tmp_path):
    """run_identify_degs(permutations = 20) on G = 400, S = 40 with 10 % shifted genes; reoa writes the two files"""
    seed = 0x5EED0C90
    rng = np.random.default_rng(seed)
    G, S = 400, 40
    group = ["ctl", "trt"] * (S // 2)
    X = rng.normal(8.0, 1.0, size=(G, S)) + rng.normal(0.0, 1.5, size=(G, 1))
    X[:40, 1::2] += 3.0
    names = [f"g{i}" for i in range(G)]
    ref0 = np.zeros(G, dtype=bool)
    ref0[40:] = True
    run = pkg.run_identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 16, 1, seed=seed, device=0, permutations=20, perm_seed=7, pairs="reversed")
    assert len(run.comparisons) == 1
    cm = run.comparisons[0]
    pn = cm["perm_null"]
    assert isinstance(pn, pkg.PermNull) and pn.n_perm == 20 and pn.delta1_null is None
    with pkg.Context(device=0, seed=seed) as ctx:                                   # delta1_obs: one pass from the run's last reference set
        ctx.set_groups(pkg.encode_groups(group)[0], 2)
        ctx.compute_thresholds(0.01)
        ctx.set_matrix(X)
        ctx.build_pairs(0)
        one = ctx.identify_degs(cm["ref_mask"], 1.0, 0.05, 1, 0)[0]
    assert np.array_equal(pn.delta1_obs, one[:, 11])
    if run.iters_run < 16:                                                          # converged: the last pass is that pass
        assert np.array_equal(pn.delta1_obs, run.result[:, 11])
    n_called = int((run.labels != "no change").sum())
    assert n_called >= 30 and (pn.p_perm[:40] <= 2 / 21).mean() > 0.8               # the shifted genes stand out of the null
    assert 0.0 <= pn.fdr_hat(n_called) <= 1.0 and pn.expected_false_calls() == float(np.mean(pn.n_up + pn.n_down))
    plain = pkg.run_identify_degs(X, group, names, 0.01, 1.0, 0.05, ref0, 16, 1, seed=seed, device=0)
    assert "perm_null" not in plain.comparisons[0] and np.array_equal(plain.result, run.result)

    expr = tmp_path / "expr.txt"
    meta = tmp_path / "meta.txt"
    with open(expr, "w") as f:
        f.write("gene\t" + "\t".join(f"s{t}" for t in range(S)) + "\n")
        for i in range(G):
            f.write(names[i] + "\t" + "\t".join(f"{v:.4f}" for v in np.abs(X[i])) + "\n")
    with open(meta, "w") as f:
        f.write("sample\tgroup\n")
        for t in range(S):
            f.write(f"s{t}\t{group[t]}\n")
    df = pkg.reoa(str(expr), str(meta), use_hk_genes="no", work_dir=str(tmp_path), seed=seed, device=0, permutations=6, n_iter=8)
    files = sorted(p for p in os.listdir(tmp_path) if "_perm_" in p)
    assert len(files) == 2 and files[0].endswith("_perm_null.tsv") and files[1].endswith("_perm_summary.tsv"), files
    null_lines = open(tmp_path / files[0]).read().splitlines()
    summ_lines = open(tmp_path / files[1]).read().splitlines()
    rpn = df.attrs["run"].comparisons[0]["perm_null"]
    assert null_lines[0] == "gene\tdelta1\tn_ge\tp_perm" and len(null_lines) == 1 + rpn.n_ge.size
    assert summ_lines[0] == "perm\tn_up\tn_down\tse" and len(summ_lines) == 1 + 6
    assert [int(l.split("\t")[2]) for l in null_lines[1:]] == rpn.n_ge.tolist()
    assert [float(l.split("\t")[3]) for l in summ_lines[1:]] == rpn.se_null.tolist()
