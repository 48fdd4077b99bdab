"""The per-sample counts of the reversed pairs (n13, n31) of every DEG at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family,
the workload of bench.py), after a real identify_degs (n_iter = 128, n_conv = 5), computed two ways that alternate in ONE process on one
context:
  sample_counts   reo_sample_counts with the NULL mask (the reference set of the tallies), n_sel / n_gt / n_eq copied back;
  host route      the only route there was before: reo_get_matrix brings the matrix down, reo_pair_list lists the partners, numpy restates
                  the comparator per DEG (config 3 is Int64: tied = equal) and sums over the partners.
The outputs must be equal.  Per route: wall time of every repeat (the first dropped) and the median.  Also timed, device only: the same call
without the tied counts (n_eq = NULL), and the all-classes call (0x1FF against the same reference set) for the same queries -- the dense
case, where the compare chain rather than the reduction dominates; its pair-sample comparisons per second are reported.
Writes profiles/sample_counts_ab.txt.
python tools/sample_counts_ab.py [repeats]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter


def host_route(ctx, degs, mask):
    """(n_sel, n_gt, n_eq) through reo_get_matrix + reo_pair_list + numpy"""
    M = ctx.get_matrix()
    assert M.dtype == np.int64
    pl = ctx.pair_list(degs, mask)
    S = M.shape[1]
    n_gt = np.zeros((degs.size, S), dtype=np.int32)
    n_eq = np.zeros((degs.size, S), dtype=np.int32)
    for q, i in enumerate(degs):
        xp = M[pl.row(q)[0], :]
        xi = M[int(i), :][None, :]
        n_gt[q] = (xi > xp).sum(axis=0)
        n_eq[q] = (xi == xp).sum(axis=0)
    return np.diff(pl.rowptr).astype(np.int32), n_gt, n_eq


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
    mask = pkg._ffi.class_mask("reversed")
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)
        labels = pkg.label_genes(result, 1.0, 0.05)
        degs = np.flatnonzero(labels != "no change").astype(np.int32)
        ref = ctx.ref_mask()
        say("config 3: %d x %d, %d passes, %d DEGs, %d reference genes in the last pass; classes n13 | n31; %d repeats, the first dropped"
            % (G, S, iters, degs.size, int(ref.sum()), reps))
        if degs.size == 0:
            say("no DEGs: nothing to count")
            return 1
        t = {"sample_counts": [], "host route": [], "no ties": [], "all classes": []}
        for r in range(reps):
            t0 = T(); sc = ctx.sample_counts(degs, mask); t["sample_counts"].append((T() - t0) * 1e3)
            t0 = T(); old = host_route(ctx, degs, mask); t["host route"].append((T() - t0) * 1e3)
            t0 = T(); nt = ctx.sample_counts(degs, mask, ties=False); t["no ties"].append((T() - t0) * 1e3)
            t0 = T(); dense = ctx.sample_counts(degs, 0x1FF); t["all classes"].append((T() - t0) * 1e3)
            if not (np.array_equal(sc.n_sel, old[0]) and np.array_equal(sc.n_gt, old[1]) and np.array_equal(sc.n_eq, old[2])
                    and np.array_equal(nt.n_gt, old[1])):
                say("  repeat %d: the two routes DIFFER" % r)
                return 1
            say("  repeat %d  sample_counts %9.3f ms   get_matrix + pair_list + numpy %9.3f ms   without n_eq %9.3f ms   all classes %9.3f ms"
                % (r, t["sample_counts"][-1], t["host route"][-1], t["no ties"][-1], t["all classes"][-1]))
        assert np.array_equal(sc.n_sel, (result[degs, 4] + result[degs, 8]).astype(np.int32))
        assert np.array_equal(dense.n_sel, result[degs, 2:11].sum(axis=1).astype(np.int32))
        assert (dense.n_gt + dense.n_eq <= dense.n_sel[:, None]).all()
        say("  %d reversed pairs (%.1f per DEG) x %d samples; the host route moved %d bytes of matrix to the host per repeat, sample_counts %d bytes of counts"
            % (int(sc.n_sel.sum()), sc.n_sel.sum() / degs.size, S, X.nbytes, sc.n_gt.nbytes + sc.n_eq.nbytes + sc.n_sel.nbytes))
        med = {}
        for k in ("sample_counts", "host route", "no ties", "all classes"):
            v = t[k][1:] if len(t[k]) > 1 else t[k]
            med[k] = float(np.median(v))
            say("  median %-13s %10.3f ms (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
        npairs = int(dense.n_sel.sum())
        say("  all classes: %d pairs x %d samples, two chains each = %.3e pair-sample comparisons in %.3f ms: %.3e per second over the WHOLE call "
            "(uploads, kernel, %d bytes of counts back, waits)"
            % (npairs, S, 2.0 * npairs * S, med["all classes"], 2.0 * npairs * S / (med["all classes"] * 1e-3), dense.n_gt.nbytes + dense.n_eq.nbytes))
        if med["sample_counts"] > med["host route"]:
            say("  THE DEVICE CALL IS SLOWER THAN THE HOST ROUTE")
            return 1
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "sample_counts_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/sample_counts_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
