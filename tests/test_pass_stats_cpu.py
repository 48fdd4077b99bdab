"""The exact reference of the six pass statistics (tests/pass_stats_cases.py) against itself, the measurement of what float64 delivers
(the figures the GPU tests assert a multiple of), the oracle's own error, and the conditions on the inputs of tests/test_gpu_pass_stats.py.
No GPU: the tallies come from the oracle, and the library's are equal to them bit for bit by the other tests."""
import functools

import numpy as np
import pytest

import pass_stats_cases as psc

MP = psc.MP


@functools.lru_cache(maxsize=None)
def tables_and_rows():
    cont = psc.tables(1)
    return cont, psc.exact_rows(cont)


@functools.lru_cache(maxsize=None)
def oracle_run(name, n_iter):
    """(oracle result [G, 15], tallies, exact_mccullagh per gene, exact_pass) of one whole run; computed once, never modified"""
    from oracle import identify_degs
    gen, args, padj_deg = psc.WHOLE_RUNS[name]
    X, group = gen(*args)
    gid = (group == "group2").astype(np.int32)
    res, iters, trace = identify_degs(X, gid, 2, psc.RUN["pval_reo"], psc.RUN["pval_deg"], padj_deg, np.ones(X.shape[0], dtype=np.uint8),
                                      n_iter, psc.RUN["n_conv"], psc.RUN["seed"])
    assert iters == n_iter
    cont = res[:, 2:11].astype(np.int64)
    for row in cont.tolist():                                                  # the corner that follows the oracle's elimination by design
        a, b, d, _, _, det = psc.system_of(row)
        assert det != 0 or b == 0, (name, n_iter, row)
    rows = psc.exact_rows(cont)
    res.setflags(write=False)
    return res, cont, rows, psc.exact_pass(cont, rows)


def test_exact_mccullagh_reproduces_the_known_answer(golden):
    """the general k x k form at 50 digits against the reference's one known answer (McCullagh 1977, a 4 x 4 table), and the closed form
    for 3 x 3 tables against the general form"""
    g = golden("mccullagh_kat.json")
    got = psc.exact_mccullagh_general(g["mat"])
    for v, e in zip(got, g["expected"]):
        assert abs(float(v) - e) <= 4e-15 * abs(e), (float(v), e)              # the stored numbers are Float64 results of the reference
    cont, rows = tables_and_rows()
    for i in range(0, cont.shape[0], 7):
        gen = psc.exact_mccullagh_general(cont[i].reshape(3, 3))
        ex = rows[i]
        for v, e in zip(gen, (ex.p, ex.delta1, ex.delta2, ex.se, ex.z1)):
            assert abs(v - e) <= MP.mpf(10) ** -38 * max(abs(e), ex.scale) * max(1, ex.kappa) * max(1, abs(ex.z1)) ** 2, (list(cont[i]), v, e)
    assert psc.exact_mccullagh([5, 0, 0, 0, 9, 0, 0, 0, 7]).singular             # a zero pivot: (1, 0, 0, 0, 0)
    assert psc.exact_mccullagh([5, 3, 0, 3, 9, 0, 0, 0, 7]).singular             # d = 0
    with pytest.raises(ValueError):
        psc.exact_mccullagh([0, 0, 4, 0, 1, 0, 4, 0, 0])                        # a = b = d = 8: not this module's business


def test_exact_pass_reproduces_the_stored_vectors(golden):
    vec = golden("bh_trimmed_std.json")
    for key, g in vec.items():
        bh = psc.exact_bh([MP.mpf(v) for v in g["p"]])
        assert np.allclose([float(v) for v in bh], g["bh"], rtol=1e-14, atol=0), key
        if g["trimmed_std"] is not None:
            assert list(psc.slice_bounds(len(g["d"]))) == g["slice"], key
            assert abs(float(psc.exact_trimmed_std([MP.mpf(v) for v in g["d"]])) - g["trimmed_std"]) <= 1e-14 * g["trimmed_std"], key
    assert psc.slice_bounds(1230) == (62, 1168) and psc.slice_bounds(1250) == (62, 1188)   # 61.5 and 62.5: half to even
    assert psc.bucket(10.0, psc.KAPPA_BUCKETS) == 10.0 and psc.bucket(10.5, psc.KAPPA_BUCKETS) == 1e3
    assert psc.judge_p(2.0 ** -995, MP.mpf(2) ** -1001) == ("underflow", True) and psc.judge_p(2.0 ** -990, MP.mpf(2) ** -1001) == ("underflow", False)
    assert psc.judge_p(0.25, MP.mpf(2) ** -999)[0] == "value"
    assert psc.judge_delta2(1e-4 + 1e-9, MP.mpf(1e-4)) < 1.1e-9 and abs(psc.judge_delta2(0.5, MP.mpf(0.25)) - 1.0) < 1e-15
    assert psc.judge_scaled(0.0, MP.mpf(0), MP.mpf(0)) == 0.0 and psc.judge_scaled(1e-300, MP.mpf(0), MP.mpf(0)) == np.inf


def test_tables_hold_what_they_promise():
    cont, rows = tables_and_rows()
    assert 2900 <= cont.shape[0] <= 3500 and cont.dtype == np.int32 and (cont >= 0).all() and cont.sum(axis=1).max() <= psc.TALLY_SUM_MAX
    assert np.array_equal(cont, psc.tables(1)) and not np.array_equal(cont, psc.tables(2))
    assert not any(r.singular for r in rows)
    kappa = np.array([float(r.kappa) for r in rows])
    z = np.array([abs(float(r.z1)) for r in rows])
    assert ((kappa > 10) & (kappa <= 1e3)).sum() >= 30 and (kappa > 1e4).sum() >= 300 and kappa.max() > 1e5
    for lo, hi in ((0, 2), (2, 8), (8, 20), (20, 37), (37, 38.4), (38.4, 1e9)):
        assert ((z > lo) & (z <= hi)).sum() >= 50, (lo, hi)
    s = cont.astype(np.int64)
    a, b, d = s[:, [1, 2, 3, 6]].sum(axis=1), s[:, [2, 6]].sum(axis=1), s[:, [2, 5, 6, 7]].sum(axis=1)
    R1, R2 = s[:, [1, 2]].sum(axis=1), s[:, [2, 5]].sum(axis=1)
    for what in (R1 == 0, R1 == a, R2 == 0, R2 == d):
        assert what.sum() >= 80
    under = sum(r.p < psc.UNDERFLOW_EXACT for r in rows)
    assert 100 <= under <= cont.shape[0] // 2
    assert len({tuple(r) for r in cont.tolist()}) < cont.shape[0]                # repeated rows


def test_measure_the_closed_form_in_float64(capsys):
    """what double arithmetic delivers over tables(1) and over the tallies of the whole runs (their columns 11..14 are judged by the
    same figures): printed, and inside the recorded figures that the GPU tests assert 4 x of"""
    cont, rows = tables_and_rows()
    worst, under = psc.measure_table(psc.closed_form_f64(cont), cont, rows)
    runs = psc.Worst()
    for name in psc.WHOLE_RUNS:
        for n_iter in psc.N_ITERS:
            res, cont_r, rows_r, ex = oracle_run(name, n_iter)
            psc.measure_table(psc.closed_form_f64(cont_r), cont_r, rows_r, worst=runs, with_p=False)
    with capsys.disabled():
        print("\nclosed_form_f64 over tables(1):", worst.show(), "underflow rows", under)
        print("closed_form_f64 over the tallies of the whole runs:", runs.show())
    rec = psc.MEASURED_REL_ERR["table"]
    assert set(worst.v) == set(rec) and set(runs.v) <= set(rec), sorted(set(worst.v) ^ set(rec), key=repr)
    for key, v in list(worst.v.items()) + list(runs.v.items()):
        assert v <= rec[key], (key, v, rec[key])


def test_measure_the_pass_in_float64(capsys):
    """the same for the end of a pass over every whole run, both numbers of passes: plain two-pass moments (the recorded figure) and the
    library's per-block moments combined by Chan's rule (its own figure)"""
    plain, blocks = psc.Worst(), psc.Worst()
    for name in psc.WHOLE_RUNS:
        for n_iter in psc.N_ITERS:
            res, cont, rows, ex = oracle_run(name, n_iter)
            d1 = psc.closed_form_f64(cont)[:, 1]
            for worst, fn in ((plain, psc.pass_f64), (blocks, psc.pass_blocks_f64)):
                se, p, padj = fn(d1)
                worst.add(("se",), psc.judge_rel(se, ex["se"]))
                psc.measure_pass(p, padj, cont, ex, worst=worst)
    with capsys.disabled():
        print("\npass_f64 over the whole runs:", plain.show())
        print("pass_blocks_f64 over the whole runs:", blocks.show())
    for worst, kind in ((plain, "pass"), (blocks, "pass_blocks")):
        rec = psc.MEASURED_REL_ERR[kind]
        assert set(worst.v) == set(rec), sorted(set(worst.v) ^ set(rec), key=repr)
        for key, v in worst.v.items():
            assert v <= rec[key], (kind, key, v, rec[key])


def test_the_oracles_own_error_is_why_the_old_tolerances_are_loose(oracle, capsys):
    """the oracle's Gauss-Jordan inverse against the exact values: printed per bucket; it stays under what _check_result grants
    (P_ATOL = 1e-6 absolute on p, STAT_RTOL = 1e-7 on the statistics), and in the ill-conditioned buckets it is orders of magnitude
    above the closed form's error: the oracle, not the kernel, is why those tolerances are what they are"""
    cont, rows = tables_and_rows()
    out = np.array([oracle.mccullagh(r.reshape(3, 3))[0] for r in cont])
    worst, _ = psc.measure_table(out, cont, rows)
    runs = psc.Worst()
    for name in psc.WHOLE_RUNS:
        for n_iter in psc.N_ITERS:
            res, cont_r, rows_r, ex = oracle_run(name, n_iter)
            psc.measure_pass(res[:, 0], res[:, 1], cont_r, ex, worst=runs)
    with capsys.disabled():
        print("\noracle.mccullagh over tables(1):", worst.show())
        print("oracle.identify_degs, p and padj of the whole runs:", runs.show())
    for i, ex in enumerate(rows):
        assert abs(out[i, 0] - float(ex.p)) <= 1e-6, i
        for col, e in ((1, ex.delta1), (2, ex.delta2), (3, ex.se), (4, ex.z1)):
            assert abs(out[i, col] - float(e)) <= 1e-7 * abs(float(e)) + 1e-9, (i, col)
    f64 = psc.MEASURED_REL_ERR["table"]
    assert worst.v[("se", 1e6)] > 1e3 * f64[("se", 1e6)] and worst.v[("se", 10.0)] < 1e-14
    assert max(runs.v.values()) < 1e-11


def test_conditions_on_the_whole_run_inputs():
    """conditions, not measurements: the cases reach where the absolute 1e-6 of the old comparison cannot see"""
    for name in psc.WHOLE_RUNS:
        for n_iter in psc.N_ITERS:
            res, cont, rows, ex = oracle_run(name, n_iter)
            G = cont.shape[0]
            p = ex["p"]
            tag = (name, n_iter)
            assert sum(v < 1e-6 for v in p) >= 20, tag
            under = sum(v < psc.UNDERFLOW_EXACT for v in p)
            if name == "underflow":
                assert under >= 5 and sum(psc.UNDERFLOW_EXACT <= v < MP.mpf(10) ** -100 for v in p) >= 5, tag
                assert under <= G // 2, tag
            else:
                assert under == 0, tag
            if name == "tail_0005":
                assert sum(v < MP.mpf(10) ** -30 for v in p) >= 5, tag
            if name == "seam" and n_iter == 6:
                assert sum(v < 1e-6 for v in p) > 1024, tag                     # the first BH block seam lies inside the tail
                order = sorted(range(G), key=lambda i: p[i])                     # ... and the minimum is carried across it
                assert min(p[order[r - 1]] * G / r for r in range(1025, 1100)) < p[order[1023]] * G / 1024, tag
            a, b = psc.slice_bounds(G)                                           # the quantile windows of a light pass can be laid
            s = sorted(ex["delta1"])
            assert s[a - 1 + 6] < s[b - 1 - 6], tag
    assert psc.SEAM_G % 1000 == 0 and psc.SEAM_G <= 65535


def test_the_judging_notices_the_faults_it_is_for():
    """three subtly wrong results that the absolute 1e-6 lets through, on the seam case: a reverse cumulative minimum that stops at the
    1 024-rank block seam, an erfc that flushes subnormal results, and two of the smallest p-values swapped"""
    res, cont, rows, ex = oracle_run("seam", 6)
    G = cont.shape[0]
    se, p, padj = psc.pass_f64(psc.closed_form_f64(cont)[:, 1])
    tol = psc.tolerance("pass")
    psc.measure_pass(p, padj, cont, ex, tol=tol)                                 # the right result passes
    order = np.argsort(p, kind="stable")
    adj = p[order] * (G / np.arange(1, G + 1))
    adj[1024:] = np.minimum.accumulate(adj[1024:][::-1])[::-1]
    adj[:1024] = np.minimum.accumulate(adj[:1024][::-1])[::-1]                   # the first block: no minimum over the blocks behind it
    broken = np.empty(G)
    broken[order] = np.minimum(adj, 1.0)
    assert np.abs(broken - padj).max() < 1e-6 and (broken[order[:1024]] != padj[order[:1024]]).any()   # the old tolerance is blind to it
    with pytest.raises(AssertionError):
        psc.measure_pass(p, broken, cont, ex, tol=tol)
    swapped = p.copy()
    swapped[order[[3, 4]]] = p[order[[4, 3]]]
    assert p[order[3]] != p[order[4]] and np.abs(swapped - p).max() < 1e-6
    with pytest.raises(AssertionError):
        psc.measure_pass(swapped, padj, cont, ex, tol=tol)
    res_u, cont_u, rows_u, ex_u = oracle_run("underflow", 6)
    se, p, padj = psc.pass_f64(psc.closed_form_f64(cont_u)[:, 1])
    psc.measure_pass(p, padj, cont_u, ex_u, tol=tol)
    small = min((i for i in range(len(p)) if ex_u["p"][i] >= psc.UNDERFLOW_EXACT), key=lambda i: p[i])
    assert p[small] < 1e-100                                                     # above 2^-1000: a value, not an underflow
    flushed = p.copy()
    flushed[small] = 0.0
    with pytest.raises(AssertionError):
        psc.measure_pass(flushed, padj, cont_u, ex_u, tol=tol)
