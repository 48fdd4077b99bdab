"""Sample tests on the GPU (reo_sample_tests; csrc/sampletests.hip): is a gene up or down in one single sample?  The expected integers come
from the numpy restatement of the comparators (tests/sample_counts_cases.py: states, selection, counts_of) under the two class masks
0x1C0 and 0x007 and are compared bit for bit; the expected p_up and p_down are the exact tails of tests/sample_tests_cases.py (Python
integers), under the tolerance constant measured there.  Every test prints the largest relative error it met."""
import numpy as np
import pytest

from query_cases import band_matrix, code_rows, halves, planted_ranks
import sample_counts_cases as scc
import sample_tests_cases as stc

pytestmark = pytest.mark.gpu

TODAY = {"k", "result", "labels", "iters_run", "trace"}
INTS = ("n_above_ctrl", "n_below_ctrl", "rev_up", "rev_down", "tied")


def interleaved_33_37():
    labels = np.array(["a" if (s % 2 == 0 and s < 66) else "b" for s in range(70)], dtype=object)
    assert (labels == "a").sum() == 33 and (labels == "b").sum() == 37
    return labels


def tie_rich(G, S, seed, second):
    """small integers with gene levels and an effect in the samples `second` (bool over the samples): ties in every sample, stable pairs of
    both directions in the control group"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(G, 1)) + rng.integers(0, 3, size=(G, S))
    X[: G // 4, second] += 4
    X[G // 4: G // 2, second] -= 4
    X += np.arange(S)[None, :] % 3 * (np.arange(G)[:, None] % 2)                  # every sample its own pattern: a swapped column shows
    return X.astype(np.int64)


def open_ctx(pkg, X, labels, pval_reo=0.1, seed=11, k=0, treat=None):
    ctx = pkg.Context(device=0, seed=seed)
    gid, lev = pkg.encode_groups(labels)
    ctx.set_groups(gid, len(lev))
    ctx.compute_thresholds(pval_reo)
    ctx.set_matrix(X)
    if treat is None:
        ctx.build_pairs(k)
    else:
        ctx.build_contrast(k, treat)
    return ctx


def same_integers(got, exp, tag=None, counts=True):
    for f in INTS[:2]:
        assert getattr(got, f).dtype == np.int32 and np.array_equal(getattr(got, f), exp[f]), (tag, f)
    for f in INTS[2:]:
        if counts:
            assert getattr(got, f).dtype == np.int32 and getattr(got, f).shape == exp[f].shape and np.array_equal(getattr(got, f), exp[f]), (tag, f)
        else:
            assert getattr(got, f) is None, (tag, f)


def check(ctx, X, genes, pm, pkg, rows=None, st=None, tag=None, counts=True):
    """one call against the restatement and the exact tails; pm None: the reference set of the last identify_degs"""
    genes = np.asarray(genes, dtype=np.int32)
    rows = rows if rows is not None else code_rows(ctx, genes)
    mask = ctx.ref_mask() if pm is None else pm
    exp = stc.expected_integers(X, lambda i: rows[i], genes, mask, st)
    got = ctx.sample_tests(genes, pm, counts=counts)
    assert np.array_equal(got.genes, genes)
    assert got.p_up.dtype == np.float64 and got.p_up.shape == got.p_down.shape == exp["u"].shape, tag
    same_integers(got, exp, tag, counts)
    background = int((exp["n_above_ctrl"].astype(np.int64) + exp["n_below_ctrl"]).max(initial=0))
    worst = stc.check_tails(got.p_up, got.p_down, exp["n_above_ctrl"][:, None], exp["n_below_ctrl"][:, None], exp["u"], exp["d"],
                            stc.tolerance(background), tag)
    print(f"{tag}: background <= {background}, largest relative error {worst:.3e} (bound {stc.tolerance(background):.3e})")
    return got, exp


def bitwise(a, b):
    for f in pkg_fields():
        x, y = getattr(a, f), getattr(b, f)
        assert (x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()), f


def pkg_fields():
    return ("genes",) + INTS + ("p_up", "p_down")


@pytest.mark.parametrize("G", [33, 64, 65, 127])
def test_word_tails_interleaved_labels_every_mask_form(pkg, G):
    """S = 70, labels a b a b ... (33 and 37 samples: the slot map is not the identity, both groups end in a partly filled block), Int64
    with ties; all genes queried, with repeats; an explicit random mask, an all-zero mask and, after identify_degs, the NULL mask."""
    seed = 9
    labels = interleaved_33_37()
    X = tie_rich(G, 70, seed, labels == "b")
    rng = np.random.default_rng(seed)
    q = np.concatenate([np.arange(G), [G - 1, 0, 0, 32]]).astype(np.int32)
    with open_ctx(pkg, X, labels, pval_reo=0.05) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        rows = {i: codes[i] for i in range(G)}
        st = scc.states(X, q)
        pm = rng.random(G) < 0.7
        got, exp = check(ctx, X, q, pm, pkg, rows, st, f"G={G} random mask")
        assert exp["n_above_ctrl"].sum() > 0 and exp["n_below_ctrl"].sum() > 0 and exp["tied"].sum() > 0
        assert exp["rev_up"].sum() > 0 and exp["rev_down"].sum() > 0
        assert got.p_up.min() < 0.05 and got.p_down.min() < 0.05                 # planted effects: both directions are found
        assert np.array_equal(got.p_up[G - 1], got.p_up[G]) and np.array_equal(got.p_up[0], got.p_up[G + 1]) and np.array_equal(got.p_down[0], got.p_down[G + 2])
        assert len({tuple(c) for c in exp["u"].T.tolist()}) > 35                 # the columns differ: their order is checked
        assert np.array_equal(got.pval, np.minimum(1.0, 2.0 * np.minimum(got.p_up, got.p_down))) and got.padj().shape == got.pval.shape
        none, _ = check(ctx, X, q, np.zeros(G, dtype=bool), pkg, rows, st, f"G={G} zero mask")
        assert (none.n_above_ctrl == 0).all() and (none.n_below_ctrl == 0).all() and (none.tied == 0).all()
        assert (none.p_up == 1.0).all() and (none.p_down == 1.0).all() and (none.calls(1.0, 1.0) == 0).all()
        ctx.identify_degs(rng.random(G) < 0.8, 1.0, 0.05, 4, 1)
        ref = ctx.ref_mask()
        null, _ = check(ctx, X, q, None, pkg, rows, st, f"G={G} NULL mask")
        bitwise(null, ctx.sample_tests(q, ref))
        everything = ctx.sample_tests(partner_mask=pm)                           # genes=None: all genes
        assert np.array_equal(everything.genes, np.arange(G)) and everything.p_up.tobytes() == got.p_up[:G].tobytes()


def test_float64_band(pkg):
    G, S, seed = 70, 12, 3
    X = band_matrix(G, S, seed)
    q = np.arange(G, dtype=np.int32)
    with open_ctx(pkg, X, halves(S)) as ctx:
        got, exp = check(ctx, X, q, np.ones(G, dtype=bool), pkg, tag="float64 band")
        assert exp["tied"].sum() > 0 and exp["n_above_ctrl"].sum() > 0 and exp["n_below_ctrl"].sum() > 0


def test_tile_seam_and_batch_seam(pkg, monkeypatch):
    """G = 4 200, S = 40: a row spans two tiles of 4 096 table columns.  Queries either side of the seam, about 300 partners on both sides
    of column 4 096; batches of one and of three queries give bitwise the arrays of the default.  Then the dense mask and 16 queries: the
    long tails of the recurrence."""
    G, S, seed = 4200, 40, 77
    labels = halves(S)
    X = tie_rich(G, S, seed, labels == "g1")
    rng = np.random.default_rng(seed)
    q = np.array([0, 4095, 4096, 4199], dtype=np.int32)
    pm = np.zeros(G, dtype=bool)
    pm[rng.choice(4096, 200, replace=False)] = True
    pm[4096 + rng.choice(G - 4096, 100, replace=False)] = True
    pm[[0, 4095, 4096, 4199]] = True
    q16 = np.concatenate([q, rng.choice(G, 12, replace=False)]).astype(np.int32)
    with open_ctx(pkg, X, labels) as ctx:
        rows = code_rows(ctx, q16)
        st16 = scc.states(X, q16)
        st = (st16[0][:4], st16[1][:4])
        got, exp = check(ctx, X, q, pm, pkg, rows, st, "seam, about 300 partners")
        assert 100 < int((got.n_above_ctrl + got.n_below_ctrl).max()) <= 304
        got7 = ctx.sample_tests(q16[:7], pm, counts=False)
        for b in ("1", "3"):
            monkeypatch.setenv("REO_SAMPLE_TESTS_BATCH", b)                      # (read per call)
            bitwise(ctx.sample_tests(q, pm), got)
            bitwise(ctx.sample_tests(q16[:7], pm, counts=False), got7)           # 7 queries in batches of 3: a short last batch
        monkeypatch.delenv("REO_SAMPLE_TESTS_BATCH")
        dense, exp = check(ctx, X, q16, np.ones(G, dtype=bool), pkg, rows, st16, "dense mask, 16 queries")
        assert int((dense.n_above_ctrl + dense.n_below_ctrl).max()) > 1500 and exp["tied"].max() > 64
        monkeypatch.setenv("REO_SAMPLE_TESTS_BATCH", "3")
        bitwise(ctx.sample_tests(q16, np.ones(G, dtype=bool)), dense)


def plane_case(pkg, G, q, marks, seed, tag):
    """S = 8, labels a b a b ..., Int64 gene levels with the first 20 000 genes up in b; a mask of `marks` and 194 random partners keeps
    the exact tails cheap"""
    S = 8
    rng = np.random.default_rng(seed)
    X = (rng.integers(0, 30000, size=(G, 1)) + rng.integers(0, 6000, size=(G, S))).astype(np.int64)
    X[:20000, 1::2] += 9000
    X = np.asfortranarray(X)
    labels = np.array(["a", "b"] * (S // 2), dtype=object)
    q = np.asarray(q, dtype=np.int32)
    pm = np.zeros(G, dtype=bool)
    pm[rng.choice(G, 194, replace=False)] = True
    pm[list(marks)] = True
    with open_ctx(pkg, X, labels, pval_reo=0.3) as ctx:
        got, exp = check(ctx, X, q, pm, pkg, tag=tag)
        assert int((got.n_above_ctrl + got.n_below_ctrl).max()) > 100 and exp["u"].max() > 50 and exp["d"].max() > 50


def test_17_plane_layout(pkg):
    """G = 66 000: five pos quads, edge rows of eight uint4; partners either side of 65 536; the log-factorial table has 131 999 entries.
    A mask of about 200 partners keeps the exact tails cheap."""
    plane_case(pkg, 66000, [65999, 0, 40000, 65535, 65536, 7], [0, 4095, 4096, 65535, 65536, 65999], 61, "17 planes")


@pytest.mark.parametrize("k,treat", [(0, None), (2, None), (1, 2)])
def test_three_groups_and_a_contrast(pkg, k, treat):
    """7 / 40 / 23 samples in a shuffled order: comparison k against the rest (k = 0, 2), and the contrast of group 1 (control, the c-side)
    against group 2 alone; tails for every sample of every group"""
    G, S, seed = 90, 70, 41
    rng = np.random.default_rng(seed)
    labels = rng.permutation(np.array(["u"] * 7 + ["v"] * 40 + ["w"] * 23, dtype=object))
    gid, lev = pkg.encode_groups(labels)
    X = tie_rich(G, S, seed, gid != k)
    with open_ctx(pkg, X, labels, k=k, treat=treat) as ctx:
        assert ctx.info()["contrast_treat"] == (-1 if treat is None else treat)
        q = np.arange(G, dtype=np.int32)
        got, exp = check(ctx, X, q, rng.random(G) < 0.8, pkg, tag=f"three groups k={k} treat={treat}")
        assert exp["n_above_ctrl"].sum() > 0 and exp["n_below_ctrl"].sum() > 0 and got.p_up.shape == (G, S)


def test_after_a_real_identify_degs(pkg):
    G, S, seed = 400, 24, 7
    X = planted_ranks(G, S, seed)
    group = pkg.synth.groups(S)
    gid, lev = pkg.encode_groups(group)
    ref0 = pkg.synth.ref_mask(G, 150, seed)
    names = [f"g{i}" for i in range(G)]
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        ref = ctx.ref_mask()
        q = np.arange(G, dtype=np.int32)
        st, exp = check(ctx, X, q, None, pkg, tag="after identify_degs")          # partner_mask=None: the reference set of the tallies
        assert np.array_equal(st.n_above_ctrl, result[:, 2 + 6: 2 + 9].sum(axis=1).astype(np.int32))   # n31 + n32 + n33
        assert np.array_equal(st.n_below_ctrl, result[:, 2 + 0: 2 + 3].sum(axis=1).astype(np.int32))   # n11 + n12 + n13
        ca, cb = ctx.sample_counts(q, stc.MASK_ABOVE), ctx.sample_counts(q, stc.MASK_BELOW)
        assert np.array_equal(st.n_above_ctrl, ca.n_sel) and np.array_equal(st.n_below_ctrl, cb.n_sel)
        assert np.array_equal(st.rev_up, cb.n_gt) and np.array_equal(st.rev_down, ca.n_lt) and np.array_equal(st.tied, ca.n_eq + cb.n_eq)
        assert (st.tied == 0).all() and ctx.info()["has_ties"] == 0
        calls = st.calls(1.0, 0.05)
        treated = np.asarray(gid) != 0
        up, dn = calls[:30][:, treated], calls[30:60][:, treated]                  # the planted genes, in the treated samples
        print("planted genes called in treated samples:", (up == 1).mean(), (dn == -1).mean(), "calls in control samples:", (calls[:, ~treated] != 0).mean())
        assert (up == 1).mean() > 0.5 and (dn == -1).mean() > 0.5 and not (up == -1).any() and not (dn == 1).any()
        assert (calls[:, ~treated] != 0).mean() < 0.05
        assert np.array_equal(ctx.ref_mask(), ref)                               # the call outdates nothing
        again = ctx.identify_degs(ref0, 1.0, 0.05, 8, 1)
        assert again[1:] == (iters, trace) and np.array_equal(again[0], result, equal_nan=True)
        light = ctx.sample_tests(counts=False)                                   # the counts=False form, all genes
        assert light.rev_up is None and light.rev_down is None and light.tied is None
        assert light.p_up.tobytes() == st.p_up.tobytes() and light.p_down.tobytes() == st.p_down.tobytes()
        assert np.array_equal(light.n_above_ctrl, st.n_above_ctrl) and np.array_equal(light.calls(1.0, 0.05), calls)
    args = (X, group, names, 0.01, 1.0, 0.05, ref0, 8, 1)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    off = pkg.run_identify_degs(*args, seed=seed, device=0, sample_tests=False)
    on = pkg.run_identify_degs(*args, seed=seed, device=0, sample_tests=True)
    assert set(plain.comparisons[0]) == TODAY == set(off.comparisons[0]) and set(on.comparisons[0]) == TODAY | {"sample_tests"}
    for r in (off, on):
        assert np.array_equal(r.result, plain.result, equal_nan=True) and r.trace == plain.trace and np.array_equal(r.result, result, equal_nan=True)
    bitwise(on.comparisons[0]["sample_tests"], st)


def test_every_refusal_has_its_message(pkg, monkeypatch):
    G, S = 70, 10
    labels = halves(S)
    X = tie_rich(G, S, 5, labels == "g1")
    q = np.arange(G, dtype=np.int32)
    ones = np.ones(G, dtype=np.uint8)
    p_up, p_down = np.full((G, S), -7.0), np.full((G, S), -7.0)
    ints = np.full((G, S), -7, dtype=np.int32)
    E = pkg._ffi.REO_EINVAL
    with open_ctx(pkg, X, labels) as ctx:
        msgs = []
        P = pkg._ffi._ptr

        def raw(genes, n, pm, up, down):                                         # the entry itself: a null pointer and a count are separate things
            o = lambda a: None if a is None else P(a)   # noqa: E731
            pkg._ffi.check(ctx._L.reo_sample_tests(ctx._h, o(genes), n, o(pm), None, None, P(ints), P(ints), P(ints), o(up), o(down)))

        for args, pattern in (((None, G, ones, p_up, p_down), "genes, p_up and p_down must not be null"),
                              ((q, G, ones, None, p_down), "genes, p_up and p_down must not be null"),
                              ((q, G, ones, p_up, None), "genes, p_up and p_down must not be null"),
                              ((q, 0, ones, p_up, p_down), "n_genes = 0"), ((q, -3, ones, p_up, p_down), "n_genes = -3"),
                              ((q, (1 << 30) + 1, ones, p_up, p_down), r"n_genes = 1073741825.*2\^30"),
                              ((np.array([0, G], dtype=np.int32), 2, ones, p_up, p_down), rf"genes\[1\] = {G} is outside \[0, {G}\)"),
                              ((np.array([-1], dtype=np.int32), 1, ones, p_up, p_down), r"genes\[0\] = -1"),
                              ((q, G, None, p_up, p_down), "partner_mask is null.*reo_identify_degs")):
            with pytest.raises(pkg.DimensionMismatch, match=pattern) as e:
                raw(*args)
            assert e.value.status == E and "reo_sample_tests" in e.value.message
            msgs.append(e.value.message)
        assert len(set(msgs)) == 7, msgs
        assert (p_up == -7.0).all() and (p_down == -7.0).all() and (ints == -7).all()   # a refused call writes nothing
        ctx.sample_tests_raw(q, ones, None, None, None, None, None, p_up, p_down)    # every integer array is optional
        assert ((p_up >= 0) & (p_up <= 1) & (p_down >= 0) & (p_down <= 1)).all() and (p_up + p_down >= 1.0 - 1e-12).all()
        ctx.identify_degs(np.ones(G, dtype=bool), 1.0, 0.05, 2, 1)
        assert ctx.sample_tests(q).p_up.shape == (G, S)                            # now there is a reference set
        ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.DimensionMismatch, match="partner_mask is null.*reo_tally"):
            ctx.sample_tests(q)
        ctx.sample_tests(q, ones)                                                 # an explicit mask still works
        with pytest.raises(pkg.DimensionMismatch, match="partner mask length"):
            ctx.sample_tests(q, ones[:-1])
    with pkg.Context(device=0, seed=1) as ctx:                                   # no table built
        ctx.G, ctx.S = G, S
        with pytest.raises(pkg.DimensionMismatch, match="no class table"):
            ctx.sample_tests(q, ones)
    with pkg.Context(device=0, seed=3) as ctx:                                   # a shard's part of the table: as reo_tally
        gid, lev = pkg.encode_groups(labels)
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.1); ctx.set_shard(0, 2); ctx.set_matrix(X)
        ctx.build_pairs(0)
        with pytest.raises(pkg.ReoError) as t:
            ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.ReoError) as e:
            ctx.sample_tests(q, ones)
        assert e.value.status == t.value.status == pkg._ffi.REO_ECOMM and e.value.message == t.value.message
    monkeypatch.setenv("REO_MULTI_ONE_DEVICE", "1")
    with pkg.Context(seed=1, n_gpus=2) as ctx:
        ctx.set_matrix(X)
        with pytest.raises(pkg.DimensionMismatch, match="reo_sample_tests is not available on a reo_create_multi context"):
            ctx.sample_tests(q, ones)


def test_cells_to_degs_with_sample_tests(pkg):
    seed, G, C = 8, 150, 240
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.integers(1, 30, size=(G, 1)).astype(float), size=(G, C)).astype(np.int64)
    X[: G // 6, C // 2:] *= 3
    X[G // 6: G // 3, : C // 2] *= 3
    labels = ["a"] * (C // 2) + ["b"] * (C - C // 2)
    args = (X, labels, [f"gene{i}" for i in range(G)], 8, 0.01, 1.0, 0.3, np.arange(G) >= G // 3, 8, 1)
    plain = pkg.identify_degs_cells(*args, seed=seed, device=0)
    got = pkg.identify_degs_cells(*args, seed=seed, device=0, sample_tests=True)
    cm = got.run.comparisons[0]
    assert set(plain.run.comparisons[0]) == TODAY and set(cm) == TODAY | {"sample_tests"}
    assert np.array_equal(cm["result"], plain.run.result, equal_nan=True)
    st = cm["sample_tests"]
    Gk, S = cm["result"].shape[0], got.run.info["S"]
    assert np.array_equal(st.genes, np.arange(Gk)) and st.p_up.shape == (Gk, S) and st.rev_up.shape == (Gk, S)
    assert np.array_equal(st.n_above_ctrl, cm["result"][:, 8:11].sum(axis=1).astype(np.int32))
    assert np.array_equal(st.n_below_ctrl, cm["result"][:, 2:5].sum(axis=1).astype(np.int32))
    assert ((st.p_up >= 0) & (st.p_up <= 1)).all() and (st.p_up + st.p_down >= 1.0 - 1e-12).all() and st.pval.min() < 0.05


def test_reoa_writes_a_sample_calls_file(pkg, tmp_path):
    """reoa(use_testdata="yes", sample_tests=True): <stem>_<fg_name>_sample_calls.tsv beside the result files, one row per gene with a
    call; with the default there is neither the key nor the file"""
    off_dir, on_dir = tmp_path / "off", tmp_path / "on"
    off_dir.mkdir(); on_dir.mkdir()
    off = pkg.reoa(use_testdata="yes", work_dir=str(off_dir), seed=0x5EED0001, device=0)
    assert "sample_tests" not in off.attrs["run"].comparisons[0] and not list(off_dir.glob("*sample_calls*"))
    df = pkg.reoa(use_testdata="yes", work_dir=str(on_dir), seed=0x5EED0001, device=0, sample_tests=True)
    run = df.attrs["run"]
    st = run.comparisons[0]["sample_tests"]
    assert np.array_equal(run.result, off.attrs["run"].result, equal_nan=True)
    calls = st.calls(1.0, 0.05)                                                  # reoa's default thresholds
    called = np.flatnonzero((calls != 0).any(axis=1))
    lines = (on_dir / "fn_expr_group1_group2_sample_calls.tsv").read_text().split("\n")
    head = lines[0].split("\t")
    assert head[0] == "gene" and len(head) == 1 + calls.shape[1] and lines[-1] == "" and len(lines) == called.size + 2
    assert [l.split("\t")[0] for l in lines[1:-1]] == [run.gene_names[int(g)] for g in called]
    for l, g in zip(lines[1:-1], called):
        assert l.split("\t")[1:] == [str(int(v)) for v in calls[g]]
    assert set(np.unique(calls).tolist()) <= {-1, 0, 1}
    assert sorted(p.name for p in on_dir.iterdir() if p.name not in {q.name for q in off_dir.iterdir()}) == ["fn_expr_group1_group2_sample_calls.tsv"]
