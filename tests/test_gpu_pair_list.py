"""Pair lists on the GPU (reo_get_ref_mask, reo_pair_list; csrc/pairlist.hip): which partner genes make up a gene's tallies.  The expected
lists always come from the existing parity hook -- ctx.get_codes for the queried rows plus numpy -- and the row lengths from the tallies
that identify_degs returns, so a wrong mask slot, a wrong word of the table or a wrong place in the CSR all show."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ALL = 0x1FF
N13, N22, N31 = 2, 4, 6


def tie_rich(G, S, seed):
    """small integers with gene levels and group effects: every one of the nine classes occurs (asserted where it matters)"""
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 8, size=(G, 1)) + rng.integers(0, 3, size=(G, S))
    X[: G // 4, S // 2:] += 4
    X[G // 4: G // 2, S // 2:] -= 4
    return X.astype(np.int64)


def labels_of(S, ngroups=2):
    return np.array([f"g{min(s * ngroups // S, ngroups - 1)}" for s in range(S)], dtype=object)


def open_ctx(pkg, X, ngroups=2, pval_reo=0.1, seed=11, k=0, matrix_first=False):
    ctx = pkg.Context(device=0, seed=seed)
    gid, lev = pkg.encode_groups(labels_of(X.shape[1], ngroups))
    if matrix_first:
        ctx.set_matrix(X)
    ctx.set_groups(gid, len(lev))
    ctx.compute_thresholds(pval_reo)
    if not matrix_first:
        ctx.set_matrix(X)
    ctx.build_pairs(k)
    return ctx


def expected(codes_of_row, genes, mask, partner_mask):
    """(rowptr, partner, code) from the class codes of the queried rows: codes_of_row(i) is row i of get_codes (255 on the diagonal)"""
    rowptr, partner, code = [0], [], []
    pm = np.asarray(partner_mask, dtype=bool)
    for i in genes:
        c = codes_of_row(int(i)).astype(np.int64)
        sel = (c < 9) & pm
        sel[sel] = ((mask >> c[sel]) & 1) == 1
        j = np.flatnonzero(sel)
        partner.append(j); code.append(c[j])
        rowptr.append(rowptr[-1] + j.size)
    return (np.asarray(rowptr, dtype=np.int64), np.concatenate(partner).astype(np.int32) if partner else np.zeros(0, np.int32),
            np.concatenate(code).astype(np.uint8) if code else np.zeros(0, np.uint8))


def same(pl, exp, tag=None):
    rowptr, partner, code = exp
    assert pl.rowptr.dtype == np.int64 and pl.partner.dtype == np.int32 and pl.code.dtype == np.uint8
    assert np.array_equal(pl.rowptr, rowptr), tag
    assert np.array_equal(pl.partner, partner), tag
    assert np.array_equal(pl.code, code), tag


def every_mask_and_the_tallies(pkg, G, S, seed, queries):
    X = tie_rich(G, S, seed)
    ref0 = pkg.synth.ref_mask(G, G // 2, seed)
    with open_ctx(pkg, X) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        assert set(range(9)) <= set(np.unique(codes).tolist()) and (np.diag(codes) == 255).all()
        ones = np.ones(G, dtype=bool)
        for mask in range(1, ALL + 1):                                           # every class mask against every gene
            same(ctx.pair_list(queries, mask, ones), expected(lambda i: codes[i], queries, mask, ones), mask)
        result, iters, _ = ctx.identify_degs(ref0, 1.0, 0.05, 6, 1)
        ref = ctx.ref_mask()
        assert iters >= 1
        for c in range(9):                                                       # the NULL mask: the reference set of the returned tallies
            pl = ctx.pair_list(queries, 1 << c)
            same(pl, expected(lambda i: codes[i], queries, 1 << c, ref), c)
            assert np.array_equal(np.diff(pl.rowptr), result[queries, 2 + c].astype(np.int64)), c
            assert (pl.code == c).all()
        names = [pkg.HEADER[2 + c] for c in range(9)]
        same(ctx.pair_list(queries, names), expected(lambda i: codes[i], queries, ALL, ref))


def test_every_class_mask_and_the_tallies(pkg):
    every_mask_and_the_tallies(pkg, 70, 10, 5, np.arange(70))


def test_partial_last_word(pkg):
    """G = 33: one bit in the second word; queries include the genes either side of the word boundary and the last gene"""
    every_mask_and_the_tallies(pkg, 33, 8, 6, np.array([32, 31, 0, 30, 32, 16, 1]))


def test_slot_order_build_is_read_in_gene_order(pkg):
    G, S, seed = 70, 12, 21
    rng = np.random.default_rng(seed)
    X = rng.permuted(np.tile(3.0 * np.arange(G)[:, None], (1, S)), axis=0)      # tie-free Float64: every sample a permutation of 0, 3, 6, ...
    X[: G // 5, S // 2:] += 60.5                                                # (shifted genes stay 0.5 away from everything else)
    X = np.asfortranarray(X)
    with open_ctx(pkg, X, matrix_first=True) as ctx:                            # (groups first would pair the sides as they arrive: identity order)
        assert ctx.info()["k1_slot_order"] == 1 and ctx.info()["has_ties"] == 0
        codes = ctx.get_codes(0, G, 0, G)
        q = np.arange(G)
        ones = np.ones(G, dtype=bool)
        for mask in (ALL, 0x44, 1 << N22, 0x101):
            same(ctx.pair_list(q, mask, ones), expected(lambda i: codes[i], q, mask, ones), mask)
        result, _, _ = ctx.identify_degs(pkg.synth.ref_mask(G, 30, seed), 1.0, 0.05, 4, 1)
        pl = ctx.pair_list(q, "reversed")
        assert np.array_equal(np.diff(pl.rowptr), (result[:, 2 + N13] + result[:, 2 + N31]).astype(np.int64))


def test_second_loop_step(pkg):
    """G = 8300: a wave covers 64 lanes x 128 columns = 8192 columns per loop step, so the last 108 genes come from the second step, on top
    of the running base of the first"""
    G, S, seed = 8300, 6, 31
    X = tie_rich(G, S, seed)
    rng = np.random.default_rng(seed)
    q = np.concatenate([[0, 31, 32, 8191, 8192, 8299], rng.choice(G, 34, replace=False)]).astype(np.int32)
    pm = rng.random(G) < 0.5
    pm[[8191, 8192, 8299, 0]] = True
    mask = (1 << N13) | (1 << N31) | (1 << N22)
    with open_ctx(pkg, X) as ctx:
        rows = {int(i): ctx.get_codes(int(i), int(i) + 1, 0, G)[0] for i in set(q.tolist())}
        exp = expected(lambda i: rows[i], q, mask, pm)
        pl = ctx.pair_list(q, ["n13", "n31", "n22"], pm)
        same(pl, exp)
        assert (pl.partner[pl.partner >= 8192]).size > 0 and np.diff(pl.rowptr).min() > 0
        for k in range(q.size):                                                  # ascending inside every row
            assert (np.diff(pl.row(k)[0]) > 0).all()


def test_partner_mask_variants(pkg):
    G, S = 70, 10
    X = tie_rich(G, S, 5)
    with open_ctx(pkg, X) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        q = np.arange(G, dtype=np.int32)
        zeros = np.zeros(G, dtype=np.uint8)
        rowptr = np.full(G + 1, -1, dtype=np.int64)
        ctx.pair_list_raw(q, ALL, zeros, rowptr, None, None, 0)                   # count only
        assert (rowptr == 0).all()
        rowptr[:] = -1
        part, code = np.full(4, -7, dtype=np.int32), np.full(4, 99, dtype=np.uint8)
        ctx.pair_list_raw(q, ALL, zeros, rowptr, part, code, 0)                   # arrays given, capacity 0
        assert (rowptr == 0).all() and (part == -7).all() and (code == 99).all()
        pl = ctx.pair_list(q, ALL, zeros)
        assert pl.partner.size == 0 and (pl.rowptr == 0).all()
        only = np.zeros(G, dtype=bool); only[17] = True
        pl = ctx.pair_list([17], ALL, only)                                       # only the query gene itself: the diagonal is no pair
        assert pl.rowptr.tolist() == [0, 0]
        pl = ctx.pair_list(q, ALL, only)                                          # one single gene: every other gene lists it, with its class
        assert pl.partner.size == G - 1 and (pl.partner == 17).all()
        assert np.array_equal(pl.code, np.delete(codes[:, 17], 17))
        same(pl, expected(lambda i: codes[i], q, ALL, only))
        rep = np.array([69, 3, 3, 0, 69, 40, 3], dtype=np.int32)                   # repeats, any order: every entry is its own row
        ones = np.ones(G, dtype=bool)
        same(ctx.pair_list(rep, 0x1EF, ones), expected(lambda i: codes[i], rep, 0x1EF, ones))
        pl = ctx.pair_list([40], "n22", ones)                                     # n_genes = 1
        same(pl, expected(lambda i: codes[i], [40], 1 << N22, ones))
        assert pl.genes.tolist() == [40]


def test_capacity_too_small_and_the_other_refusals(pkg):
    G, S = 70, 10
    X = tie_rich(G, S, 5)
    with open_ctx(pkg, X) as ctx:
        codes = ctx.get_codes(0, G, 0, G)
        q = np.arange(G, dtype=np.int32)
        ones = np.ones(G, dtype=np.uint8)
        exp = expected(lambda i: codes[i], q, 0x44, ones)
        total = int(exp[0][-1])
        assert total > 8
        cap = total - 1
        rowptr = np.full(G + 1, -1, dtype=np.int64)
        part, code = np.full(total + 16, -7, dtype=np.int32), np.full(total + 16, 99, dtype=np.uint8)
        with pytest.raises(pkg.ReoError) as e:
            ctx.pair_list_raw(q, 0x44, ones, rowptr, part, code, cap)
        assert e.value.status == pkg._ffi.REO_EINVAL and str(total) in e.value.message and str(cap) in e.value.message
        assert np.array_equal(rowptr, exp[0])
        assert (part[cap:] == -7).all() and (code[cap:] == 99).all()
        ctx.pair_list_raw(q, 0x44, ones, rowptr, part, code, total)              # exactly enough
        assert np.array_equal(part[:total], exp[1]) and np.array_equal(code[:total], exp[2]) and (part[total:] == -7).all()
        # every other refusal has a message of its own
        msgs = []
        for args in ((None, 0x44, ones, rowptr, None, None, 0), (q, 0x44, ones, None, None, None, 0),
                     (np.array([0, G], dtype=np.int32), 0x44, ones, rowptr, None, None, 0), (np.array([-1], dtype=np.int32), 0x44, ones, rowptr, None, None, 0),
                     (q[:0], 0x44, ones, rowptr, None, None, 0), (q, 0, ones, rowptr, None, None, 0), (q, 0x200, ones, rowptr, None, None, 0),
                     (q, 0x44, None, rowptr, None, None, 0)):
            with pytest.raises(pkg.DimensionMismatch) as e:
                ctx.pair_list_raw(*args)
            assert e.value.status == pkg._ffi.REO_EINVAL
            msgs.append(e.value.message)
        assert len(set(msgs)) >= 6, msgs
        assert "partner_mask is null" in msgs[-1] and "reo_identify_degs" in msgs[-1]   # the NULL mask with no valid reference set
    with pkg.Context(device=0, seed=1) as ctx:                                   # no table built
        ctx.G = G
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.pair_list(q, 0x44, ones)
        assert "no class table" in e.value.message


def light_case(G, S, seed):
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 12, size=(G, 1)) * 3 + rng.integers(0, 7, size=(G, S))
    up = rng.random(G) < 0.15
    X[up, S // 2:] += rng.integers(2, 9, size=(int(up.sum()), 1))
    dn = (~up) & (rng.random(G) < 0.15)
    X[dn, S // 2:] -= rng.integers(2, 9, size=(int(dn.sum()), 1))
    return X.astype(np.int64)


# (G, S, seed, n_iter, n_conv, padj_deg): converging calls, short forced ones (n_iter runs out on a light pass), long forced ones (the
# reference sets cycle -- a fixed point is a cycle of period 1 -- and whole periods are skipped), one and two passes
REF_CASES = [(230, 12, 17, 30, 2, 0.3), (200, 12, 18, 30, 2, 0.3), (120, 16, 3, 1, 0, 0.05), (240, 16, 4, 2, 0, 0.05),
             (160, 16, 5, 5, 0, 0.05), (230, 12, 6, 7, 0, 0.3), (230, 12, 17, 4, 0, 0.3), (200, 12, 18, 6, 0, 0.3), (180, 16, 7, 40, 0, 0.05), (140, 12, 8, 51, 0, 0.3), (220, 20, 9, 64, 0, 0.05)]


def test_ref_mask_is_the_set_of_the_last_executed_pass(pkg, monkeypatch, capfd):
    monkeypatch.setenv("REO_LIGHT_MIN_G", "64")
    monkeypatch.setenv("REO_LIGHT_WINDOW", "6")      # (the default window of 24 ranks either side of a quantile does not fit 5 % of 120 genes: no light pass)
    monkeypatch.setenv("REO_DEBUG_PASSES", "1")      # the library then says on stderr whether the last batch ended on a sorting pass
    kinds = {"converged": 0, "light_exhausted": 0, "cycle_skipped": 0, "one_pass": 0}
    seen = []
    for G, S, seed, n_iter, n_conv, padj_deg in REF_CASES:
        tag = (G, S, seed, n_iter, n_conv)
        X = light_case(G, S, seed)
        ref0 = pkg.synth.ref_mask(G, G // 3, seed)
        with open_ctx(pkg, X, pval_reo=0.05, seed=seed) as ctx:
            with pytest.raises(pkg.DimensionMismatch) as e:                      # before any identify_degs
                ctx.ref_mask()
            assert "not run" in e.value.message or "reo_build_pairs" in e.value.message
            capfd.readouterr()
            result, iters, trace = ctx.identify_degs(ref0, 1.0, padj_deg, n_iter, n_conv)
            err = capfd.readouterr().err
            last_full = [int(v) for v in re.findall(r"last_full (\d)", err)][-1]
            info = ctx.info()
            seen.append((tag, iters, last_full, info["cycle_period"], info["cycle_passes_skipped"]))
            if iters < n_iter:
                kinds["converged"] += 1
            elif info["cycle_passes_skipped"] > 0:
                kinds["cycle_skipped"] += 1
            elif iters == 1:
                kinds["one_pass"] += 1
            elif not last_full:
                kinds["light_exhausted"] += 1
            mask = ctx.ref_mask()
            assert mask.dtype == bool and mask.shape == (G,)
            assert np.array_equal(ctx.tally(mask), result[:, 2:11].astype(np.int32)), tag
            with pytest.raises(pkg.DimensionMismatch) as e:                      # reo_tally has used the mask buffers
                ctx.ref_mask()
            assert "reo_tally" in e.value.message
            with pytest.raises(pkg.DimensionMismatch):
                ctx.pair_list([0], ALL)
            p = iters - 1
            if p == 0:
                assert np.array_equal(mask, ref0), tag
            else:
                r2, i2, _ = ctx.identify_degs(ref0, 1.0, padj_deg, p, n_conv)
                assert i2 == p, tag
                assert np.array_equal(mask, ~((r2[:, 0] <= 1.0) & (r2[:, 1] <= padj_deg))), tag
            ctx.identify_degs(ref0, 1.0, padj_deg, 0, n_conv)                     # n_iter <= 0: no pass, no mask
            with pytest.raises(pkg.DimensionMismatch) as e:
                ctx.ref_mask()
            assert "n_iter" in e.value.message
    assert kinds["converged"] > 0 and kinds["light_exhausted"] > 0 and kinds["cycle_skipped"] > 0 and kinds["one_pass"] > 0, (kinds, seen)


TODAY = {"k", "result", "labels", "iters_run", "trace"}


def test_three_groups_pairs_per_comparison(pkg):
    G, S, seed = 90, 18, 41
    X = tie_rich(G, S, seed)
    X[G // 2: G // 2 + 12, 2 * S // 3:] += 5
    group = labels_of(S, 3)
    ref0 = pkg.synth.ref_mask(G, 40, seed)
    names = [f"g{i}" for i in range(G)]
    args = (X, group, names, 0.1, 1.0, 0.3, ref0, 6, 1)
    plain = pkg.run_identify_degs(*args, seed=seed, device=0)
    assert len(plain.comparisons) == 3 and all(set(cm) == TODAY for cm in plain.comparisons)
    run = pkg.run_identify_degs(*args, seed=seed, device=0, pairs="reversed")
    assert all(set(cm) == TODAY | {"ref_mask", "pairs"} for cm in run.comparisons)
    gid, lev = pkg.encode_groups(group)
    ndeg = 0
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 3); ctx.compute_thresholds(0.1); ctx.set_matrix(X)
        for cm, pm in zip(run.comparisons, plain.comparisons):
            assert np.array_equal(cm["result"], pm["result"], equal_nan=True)
            ctx.build_pairs(cm["k"])
            codes = ctx.get_codes(0, G, 0, G)
            degs = np.flatnonzero(cm["labels"] != "no change")
            ndeg += degs.size
            pl = cm["pairs"]
            assert np.array_equal(pl.genes, degs)
            same(pl, expected(lambda i: codes[i], degs, 0x44, cm["ref_mask"]), cm["k"])
            assert np.array_equal(np.diff(pl.rowptr), (cm["result"][degs, 2 + N13] + cm["result"][degs, 2 + N31]).astype(np.int64))
        # after build_pairs(1) on three groups the mask of the earlier comparison is out of date
        ctx.identify_degs(ref0, 1.0, 0.3, 3, 1)
        assert ctx.ref_mask().shape == (G,)
        ctx.build_pairs(1)
        with pytest.raises(pkg.DimensionMismatch) as e:
            ctx.ref_mask()
        assert "reo_build_pairs" in e.value.message
    assert ndeg > 0


def test_sharded_context_answers_as_tally_does(pkg):
    G, S = 70, 10
    X = tie_rich(G, S, 5)
    with pkg.Context(device=0, seed=3) as ctx:
        gid, lev = pkg.encode_groups(labels_of(S))
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.1); ctx.set_shard(0, 2); ctx.set_matrix(X)
        ctx.build_pairs(0)
        with pytest.raises(pkg.ReoError) as t:
            ctx.tally(np.ones(G, dtype=bool))
        with pytest.raises(pkg.ReoError) as e:
            ctx.pair_list(np.arange(G), ALL, np.ones(G, dtype=bool))
        assert e.value.status == t.value.status == pkg._ffi.REO_ECOMM and e.value.message == t.value.message


def test_cells_to_degs_with_pairs(pkg):
    seed, G, C = 8, 150, 240
    rng = np.random.default_rng(seed)
    X = rng.poisson(rng.integers(1, 30, size=(G, 1)).astype(float), size=(G, C)).astype(np.int64)
    X[: G // 6, C // 2:] *= 3
    X[G // 6: G // 3, : C // 2] *= 3
    labels = ["a"] * (C // 2) + ["b"] * (C - C // 2)
    names = [f"gene{i}" for i in range(G)]
    args = (X, labels, names, 8, 0.01, 1.0, 0.3, np.arange(G) >= G // 3, 8, 1)
    plain = pkg.identify_degs_cells(*args, seed=seed, device=0)
    got = pkg.identify_degs_cells(*args, seed=seed, device=0, pairs=["n13", "n31"])
    assert got.gene_kept.all() and set(plain.run.comparisons[0]) == TODAY
    cm = got.run.comparisons[0]
    assert set(cm) == TODAY | {"ref_mask", "pairs"} and np.array_equal(cm["result"], plain.run.result, equal_nan=True)
    degs = np.flatnonzero(cm["labels"] != "no change")
    pl = cm["pairs"]
    assert degs.size > 0 and np.array_equal(pl.genes, degs) and cm["ref_mask"].shape == (G,)
    assert np.array_equal(np.diff(pl.rowptr), (cm["result"][degs, 2 + N13] + cm["result"][degs, 2 + N31]).astype(np.int64))
    assert cm["ref_mask"][pl.partner].all() and np.isin(pl.code, (N13, N31)).all() and pl.partner.size > 0


def test_reoa_writes_a_pairs_file(pkg, tmp_path):
    """reoa(use_testdata="yes", pairs="reversed"): <stem>_<fg_name>_pairs.tsv beside the result files, one line per listed pair"""
    df = pkg.reoa(use_testdata="yes", work_dir=str(tmp_path), seed=0x5EED0001, device=0, pairs="reversed")
    run = df.attrs["run"]
    cm = run.comparisons[0]
    pl = cm["pairs"]
    degs = np.flatnonzero(cm["labels"] != "no change")
    assert np.array_equal(pl.genes, degs)
    assert np.array_equal(np.diff(pl.rowptr), (cm["result"][degs, 2 + N13] + cm["result"][degs, 2 + N31]).astype(np.int64))
    lines = (tmp_path / "fn_expr_group1_group2_pairs.tsv").read_text().split("\n")
    assert lines[0] == "gene\tpartner\tclass" and lines[-1] == "" and len(lines) == pl.partner.size + 2
    if pl.partner.size:
        q = int(np.flatnonzero(np.diff(pl.rowptr) > 0)[0])
        assert lines[1].split("\t") == [run.gene_names[int(pl.genes[q])], run.gene_names[int(pl.partner[0])], pkg.HEADER[2 + int(pl.code[0])]]
        assert lines[-2].split("\t")[1] == run.gene_names[int(pl.partner[-1])]
    assert (tmp_path / "fn_expr_group1_group2_result.tsv").stat().st_size > 0
