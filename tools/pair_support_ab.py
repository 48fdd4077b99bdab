"""The per-group support of the reversed pairs (n13, n31) of every DEG at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family,
the workload of bench.py), after a real identify_degs (n_iter = 128, n_conv = 5), computed two ways that alternate in ONE process on one
context, over the same CSR (reo_pair_list, taken once):
  pair_support    reo_pair_support, n_gt / n_eq copied back;
  host route      the route it replaces: reo_get_matrix brings the matrix down, numpy restates the comparator row by row (config 3 is Int64:
                  tied = equal) and sums over each group's samples.
The outputs must be equal.  Per route: wall time of every repeat (the first dropped) and the median -- WHOLE CALLS (uploads, kernel, copies
back, waits), not the kernel alone.  Also timed, device only: the same call without the tied counts (n_eq = NULL), and the outcome form
(entries x S bytes) on the 200 pairs with the largest |delta| only, checked against numpy on the same matrix.
Writes profiles/pair_support_ab.txt.
python tools/pair_support_ab.py [repeats]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter


def host_route(ctx, pl, gid, ngroups):
    """(n_gt, n_eq), entries x ngroups, through reo_get_matrix + numpy over the CSR"""
    M = ctx.get_matrix()
    assert M.dtype == np.int64
    n = int(pl.rowptr[-1])
    n_gt = np.zeros((n, ngroups), dtype=np.int32)
    n_eq = np.zeros((n, ngroups), dtype=np.int32)
    cols = [np.flatnonzero(gid == g) for g in range(ngroups)]
    for q, i in enumerate(pl.genes):
        a, b = int(pl.rowptr[q]), int(pl.rowptr[q + 1])
        if a == b:
            continue
        xp = M[pl.partner[a:b], :]
        xi = M[int(i), :][None, :]
        gt, eq = xi > xp, xi == xp
        for g in range(ngroups):
            n_gt[a:b, g] = gt[:, cols[g]].sum(axis=1)
            n_eq[a:b, g] = eq[:, cols[g]].sum(axis=1)
    return n_gt, n_eq, M


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S = 20000, 1000
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)
        labels = pkg.label_genes(result, 1.0, 0.05)
        degs = np.flatnonzero(labels != "no change").astype(np.int32)
        if degs.size == 0:
            say("no DEGs: nothing to count")
            return 1
        pl = ctx.pair_list(degs, "reversed")
        n = int(pl.rowptr[-1])
        say("config 3: %d x %d, %d passes, %d DEGs, %d reversed pairs (n13 | n31, %.1f per DEG) against the last pass's reference set; %d repeats, "
            "the first dropped; whole calls are timed, not the kernel alone" % (G, S, iters, degs.size, n, n / degs.size, reps))
        t = {"pair_support": [], "host route": [], "no ties": [], "outcomes, top 200": []}
        for r in range(reps):
            t0 = T(); ps = ctx.pair_support(pl); t["pair_support"].append((T() - t0) * 1e3)
            t0 = T(); old = host_route(ctx, pl, gid, len(lev)); t["host route"].append((T() - t0) * 1e3)
            t0 = T(); nt = ctx.pair_support(pl, ties=False); t["no ties"].append((T() - t0) * 1e3)
            top = ps.top(200)
            sig = (ps.entry_genes[top], np.arange(top.size + 1, dtype=np.int64), ps.partner[top])   # every pair a row of its own
            t0 = T(); oc = ctx.pair_support(sig, outcomes=True); t["outcomes, top 200"].append((T() - t0) * 1e3)
            M = old[2]
            xi, xp = M[sig[0], :], M[sig[2], :]
            if not (np.array_equal(ps.n_gt, old[0]) and np.array_equal(ps.n_eq, old[1]) and np.array_equal(nt.n_gt, old[0]) and nt.n_eq is None
                    and np.array_equal(oc.outcome, (2 * (xi > xp) + (xi == xp)).astype(np.uint8)) and np.array_equal(oc.n_gt, ps.n_gt[top])):
                say("  repeat %d: the two routes DIFFER" % r)
                return 1
            say("  repeat %d  pair_support %9.3f ms   get_matrix + numpy %9.3f ms   without n_eq %9.3f ms   outcomes of the top 200 %9.3f ms"
                % (r, t["pair_support"][-1], t["host route"][-1], t["no ties"][-1], t["outcomes, top 200"][-1]))
        say("  the host route moved %d bytes of matrix to the host per repeat; pair_support sent %d bytes of partners and work items and brought back "
            "%d bytes of counts" % (X.nbytes, pl.partner.nbytes + 16 * int(np.sum((np.diff(pl.rowptr) + 63) // 64)), ps.n_gt.nbytes + ps.n_eq.nbytes))
        med = {}
        for k in t:
            v = t[k][1:] if len(t[k]) > 1 else t[k]
            med[k] = float(np.median(v))
            say("  median %-18s %10.3f ms (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
        say("  %d pairs x %d samples, two chains each = %.3e pair-sample comparisons in %.3f ms: %.3e per second over the WHOLE call"
            % (n, S, 2.0 * n * S, med["pair_support"], 2.0 * n * S / (med["pair_support"] * 1e-3)))
        d = ps.delta()
        say("  |delta| of the listed pairs: min %.3f, median %.3f, max %.3f (every reversed pair has |delta| > 0)" % (np.abs(d).min(), np.median(np.abs(d)), np.abs(d).max()))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "pair_support_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/pair_support_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
