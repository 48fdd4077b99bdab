"""Per-sample tests of ALL genes at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family, the workload of bench.py), after a
real identify_degs (n_iter = 128, n_conv = 5), computed two ways that alternate in ONE process on one context:
  sample_tests    reo_sample_tests with the NULL mask (the reference set of the tallies): the integers and both tails copied back;
  host route      the only route there was before: reo_sample_counts twice for every gene (class masks 0x1C0 and 0x007, tied counts
                  included), the 2 x 2 tables formed in numpy, the tails by scipy.stats.hypergeom.
The integer outputs must be equal, for all genes.  scipy needs about 50 us per cell for the two tails, a quarter of an hour for the
2 * 10^7 cells of config 3, so the scipy step is TIMED ON A SEEDED SAMPLE of genes (second argument, default 300; 0 = all genes) and its
time for all genes is a linear extrapolation, marked as such; the counting step of the host route is timed in full.  On the sample the
tails are compared with scipy's and the largest relative difference is reported (scipy is not exact: the bound of the tests comes from
exact integer tails, tests/sample_tests_cases.py).
No speed is promised and none is asserted.  Whole calls are timed -- uploads, launches, copies back, waits; the kernel alone is not timed.
Writes profiles/sample_tests_ab.txt.
python tools/sample_tests_ab.py [repeats] [scipy genes]"""
import os
import sys
import time

import numpy as np
from scipy import stats

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter
ABOVE, BELOW = 0x1C0, 0x007


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    n_scipy = int(sys.argv[2]) if len(sys.argv) > 2 else 300
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S = 20000, 1000
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    q = np.arange(G, dtype=np.int32)
    rows = q if n_scipy <= 0 or n_scipy >= G else np.sort(np.random.default_rng(seed).choice(G, n_scipy, replace=False))
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)
        ref = ctx.ref_mask()
        say("config 3: %d x %d, %d passes, %d reference genes in the last pass; all %d genes queried; %d repeats, the first dropped"
            % (G, S, iters, int(ref.sum()), G, reps))
        t = {"sample_tests": [], "no counts": [], "host counts": [], "host scipy": []}
        for r in range(reps):
            t0 = T(); st = ctx.sample_tests(); t["sample_tests"].append((T() - t0) * 1e3)
            t0 = T()
            ca, cb = ctx.sample_counts(q, ABOVE), ctx.sample_counts(q, BELOW)
            u = ca.n_gt + cb.n_gt
            tied = ca.n_eq + cb.n_eq
            d = (ca.n_sel + cb.n_sel)[:, None] - u - tied
            t["host counts"].append((T() - t0) * 1e3)
            t0 = T()
            a_, b_, u_, d_ = ca.n_sel[rows, None].astype(np.int64), cb.n_sel[rows, None].astype(np.int64), u[rows].astype(np.int64), d[rows].astype(np.int64)
            N, K, n = a_ + b_ + u_ + d_, a_ + u_, u_ + d_
            up = stats.hypergeom.sf(u_ - 1, N, K, n)
            down = stats.hypergeom.cdf(u_, N, K, n)
            t["host scipy"].append((T() - t0) * 1e3)
            t0 = T(); light = ctx.sample_tests(counts=False); t["no counts"].append((T() - t0) * 1e3)
            same = (np.array_equal(st.n_above_ctrl, ca.n_sel) and np.array_equal(st.n_below_ctrl, cb.n_sel) and np.array_equal(st.rev_up, cb.n_gt)
                    and np.array_equal(st.rev_down, ca.n_lt) and np.array_equal(st.tied, tied)
                    and light.p_up.tobytes() == st.p_up.tobytes() and light.p_down.tobytes() == st.p_down.tobytes())
            if not same:
                say("  repeat %d: the integer outputs of the two routes DIFFER" % r)
                return 1
            say("  repeat %d  sample_tests %10.3f ms   without the integer fields %10.3f ms   host: 2 x sample_counts + numpy %10.3f ms, scipy on %d genes %10.3f ms"
                % (r, t["sample_tests"][-1], t["no counts"][-1], t["host counts"][-1], rows.size, t["host scipy"][-1]))
        assert np.array_equal(st.n_above_ctrl, result[:, 8:11].sum(axis=1).astype(np.int32))
        assert np.array_equal(st.n_below_ctrl, result[:, 2:5].sum(axis=1).astype(np.int32))
        with np.errstate(divide="ignore", invalid="ignore"):
            big = (up > 1e-280) & (down > 1e-280)
            rel = np.maximum(np.abs(st.p_up[rows] - up) / up, np.abs(st.p_down[rows] - down) / down)[big]
        say("  background per gene: %.1f partners on average (largest %d); tails against scipy on %d genes x %d samples: largest relative "
            "difference %.3e (over the %d cells with both scipy tails above 1e-280)"
            % (float((st.n_above_ctrl + st.n_below_ctrl).mean()), int((st.n_above_ctrl + st.n_below_ctrl).max()), rows.size, S,
               float(rel.max(initial=0.0)), int(big.sum())))
        calls = st.calls(1.0, 0.05)
        say("  calls at pval_deg 1, padj_deg 0.05: %d up, %d down of %d cells; %d genes with at least one call"
            % (int((calls == 1).sum()), int((calls == -1).sum()), calls.size, int((calls != 0).any(axis=1).sum())))
        say("  the host route moved %d bytes of counts to the host per repeat; sample_tests %d bytes (%d without the integer fields)"
            % (2 * (ca.n_gt.nbytes + ca.n_eq.nbytes + ca.n_sel.nbytes), st.p_up.nbytes * 2 + st.rev_up.nbytes * 3 + st.n_above_ctrl.nbytes * 2,
               st.p_up.nbytes * 2 + st.n_above_ctrl.nbytes * 2))
        med = {}
        for k in ("sample_tests", "no counts", "host counts", "host scipy"):
            v = t[k][1:] if len(t[k]) > 1 else t[k]
            med[k] = float(np.median(v))
            say("  median %-13s %12.3f ms (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
        if rows.size < G:
            say("  host route for all genes: %.3f ms of counting (measured) + %.0f ms of scipy (EXTRAPOLATED from %d genes, linear in the cells)"
                % (med["host counts"], med["host scipy"] * G / rows.size, rows.size))
        say("  whole calls were timed (uploads, launches, copies back, waits); the kernel alone was not timed; no speed is promised")
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "sample_tests_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/sample_tests_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
