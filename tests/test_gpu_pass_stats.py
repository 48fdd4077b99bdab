"""pval, padj, delta1, delta2, se and z1 of the HIP path against the exact reference of tests/pass_stats_cases.py (mpmath, 50 digits),
under 4 x the error that plain float64 arithmetic was measured to have (MEASURED_REL_ERR there; tests/test_pass_stats_cpu.py measures
it).  The comparison with the oracle (test_gpu_parity._check_result: 1e-6 absolute on a p-value) cannot see a p-value below 1e-6; here
every p-value is held by its relative error down to 2^-1000, and below that to the underflow bound.

The final columns 0, 1 and 11..14 are a function of the last pass's tallies (columns 2..10, pinned bit for bit by the other tests), so
the whole runs are judged from the tallies they return.

Every test prints the largest errors it finds."""
import re

import numpy as np
import pytest

import pass_stats_cases as psc

pytestmark = pytest.mark.gpu


def test_mccullagh_tables_against_the_exact_reference(pkg, capsys):
    """Context.mccullagh over tables(1), one launch: every row against exact_mccullagh per bucket, the underflow class by its bound,
    equal rows equal bits."""
    cont = psc.tables(1)
    with pkg.Context(device=0) as ctx:
        out = ctx.mccullagh(cont)
    assert np.isfinite(out).all()
    seen = {}
    for row, got in zip(cont.tolist(), out.tolist()):
        assert seen.setdefault(tuple(row), got) == got, row                    # the same table, the same bits
    assert len(seen) < cont.shape[0]
    worst, under = psc.Worst(), 0
    try:
        worst, under = psc.measure_table(out, cont, worst=worst, tol=psc.tolerance("table"), tag="tables(1)")
    finally:
        with capsys.disabled():
            print("\nContext.mccullagh over tables(1), largest errors:", worst.show(), "underflow rows", under)
    assert under >= 100
    assert (out[:, 0] >= 0).all() and (out[:, 0] <= 1).all()


def _run(pkg, name, n_iter):
    gen, args, padj_deg = psc.WHOLE_RUNS[name]
    X, group = gen(*args)
    G = X.shape[0]
    return pkg.run_identify_degs(X, group, list(range(G)), psc.RUN["pval_reo"], psc.RUN["pval_deg"], padj_deg, np.ones(G, dtype=bool),
                                 n_iter, psc.RUN["n_conv"], seed=psc.RUN["seed"], device=0)


@pytest.mark.parametrize("n_iter", psc.N_ITERS)
@pytest.mark.parametrize("name", list(psc.WHOLE_RUNS))
def test_whole_runs_against_the_exact_reference(pkg, monkeypatch, capfd, name, n_iter):
    """run_identify_degs, Float64, all-ones reference set: once a sorting pass only, once 6 passes with the light passes forced on at
    this size (a light pass must have completed: the final columns then come from the replayed sorting pass)."""
    monkeypatch.setenv("REO_LIGHT_MIN_G", "64")
    monkeypatch.setenv("REO_LIGHT_WINDOW", "6")
    monkeypatch.setenv("REO_DEBUG_PASSES", "1")
    capfd.readouterr()
    run = _run(pkg, name, n_iter)
    err = capfd.readouterr().err
    assert run.iters_run == n_iter
    batches = [tuple(int(v) for v in m) for m in re.findall(r"batch: (\d+) sorting \+ (\d+) light launches, passes (\d+) -> (\d+)", err)]
    assert batches, err[-500:]
    light = sum(b[3] - b[2] for b in batches if b[1] > 0)
    if n_iter == 1:
        assert light == 0
    else:
        assert light > 0, (name, batches)                                      # a light pass completed
    res = run.result
    G = res.shape[0]
    assert np.isfinite(res).all()
    cont = res[:, 2:11].astype(np.int64)
    assert np.array_equal(cont, res[:, 2:11])
    rows = psc.exact_rows(cont)
    ex = psc.exact_pass(cont, rows)
    stats, ps = psc.Worst(), psc.Worst()
    try:
        psc.measure_table(res[:, [0, 11, 12, 13, 14]], cont, rows, worst=stats, tol=psc.tolerance("table"), tag=(name, n_iter), with_p=False)
        _, under = psc.measure_pass(res[:, 0], res[:, 1], cont, ex, worst=ps, tol=psc.tolerance("pass"), tag=(name, n_iter))
    finally:
        with capfd.disabled():
            print(f"\n{name}, {n_iter} passes (light passes completed: {light}), largest errors:", stats.show(), ps.show())
    assert (under > 0) == (name == "underflow")
    # what an absolute tolerance cannot see
    pval, padj, ad1 = res[:, 0], res[:, 1], np.abs(res[:, 11])
    order = np.lexsort((padj, pval))
    assert (np.diff(padj[order]) >= 0).all()                                   # padj never decreases along ascending pval
    assert (padj >= pval).all() and (pval >= 0).all() and (padj <= 1).all()
    by = np.argsort(ad1, kind="stable")
    same = np.flatnonzero(np.diff(ad1[by]) == 0)                               # equal |delta1|: equal bits of pval and of padj
    assert np.array_equal(pval[by][same], pval[by][same + 1]) and np.array_equal(padj[by][same], padj[by][same + 1])
