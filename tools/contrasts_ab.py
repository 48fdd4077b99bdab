"""All six pairwise contrasts of four groups of 250 samples at 20 000 genes x 1 000 samples (T0 family: per-sample ranks, tie-free), each
followed by a real identify_degs (n_iter = 128, n_conv = 5), two ways that alternate contrast by contrast in ONE process:
  route A   one context that holds the whole matrix: build_contrast(ctrl, treat) + identify_degs.  The first build of the context counts
            every group once (k1w_group_counts); every contrast is then one table-sized classification (k1_classify_contrast).
  route B   the route it replaces, per contrast: a device gather of the two groups' columns, set_matrix_tensor, groups, thresholds,
            build_pairs(0) -- ranking, the full pair kernel -- and identify_degs, on a second context.
The matrix is on the device before anything is timed.  The two routes' results (all 15 columns, passes, trace) must be equal for every
contrast, or the tool fails.  Reported: wall ms per contrast for both routes, WHOLE calls up to the return of identify_degs (median and
range over the rounds after the first, whose first contrast of route A carries the counting and is shown apart), and, from one more round
with the stage timers on, the K1 timer (pair kernel or classification) and the transform timer per contrast.
Writes profiles/contrasts_ab.txt.
python tools/contrasts_ab.py [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter


def main():
    import torch
    rounds = max(int(sys.argv[1]) if len(sys.argv) > 1 else 4, 4)   # the first round warms up and counts; at least three are measured
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S, C = 20000, 1000, 4
    X = pkg.synth.t0_ranks(G, S, seed)
    gid = (np.arange(S) // (S // C)).astype(np.int32)             # quarters: groups 0, 1 lie in the generator's first half, 2, 3 in its shifted one
    levels = list(range(C))
    contrasts = pkg.parse_contrasts(levels, "all")
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    dev = torch.device("cuda", 0)
    XT = torch.from_numpy(np.ascontiguousarray(X.T)).to(dev)      # samples x genes, contiguous: .t() is the column-major matrix
    cols = {g: torch.from_numpy(np.flatnonzero(gid == g)).to(dev) for g in range(C)}
    sub_gid = {}
    for c, t in contrasts:
        sel = np.flatnonzero((gid == c) | (gid == t))
        sub_gid[c, t] = (gid[sel] == t).astype(np.int32)          # ctrl appears first: id 0, the control of build_pairs(0)
        assert sub_gid[c, t][0] == 0
    torch.cuda.synchronize()

    def route_a(ctx, c, t):
        ctx.build_contrast(c, t)
        return ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)

    def route_b(ctx, c, t):
        idx = torch.sort(torch.cat([cols[c], cols[t]])).values
        sub = XT.index_select(0, idx).t()                         # the device gather: genes x 500, column-major
        ctx.set_matrix_tensor(sub)
        ctx.set_groups(sub_gid[c, t], 2)
        ctx.compute_thresholds(0.01)
        ctx.build_pairs(0)
        return ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)

    ta = {ct: [] for ct in contrasts}
    tb = {ct: [] for ct in contrasts}
    say("%d x %d, %d groups of %d, T0 ranks; %d contrasts; %d rounds, the first apart; whole calls up to the return of identify_degs"
        % (G, S, C, S // C, len(contrasts), rounds))
    with pkg.Context(device=0, seed=seed) as A, pkg.Context(device=0, seed=seed) as B:
        t0 = T()
        A.set_matrix_tensor(XT.t()); A.set_groups(gid, C); A.compute_thresholds(0.01)
        say("  route A set-up (matrix on the device, groups, thresholds; the ranking waits for the first build): %.3f ms" % ((T() - t0) * 1e3))
        for r in range(rounds + 1):
            timers = r == rounds                                  # the last round: stage timers on, wall times not kept
            A.set_profiling(timers); B.set_profiling(timers)
            for c, t in contrasts:
                if timers:
                    A.reset_timings(); B.reset_timings()
                t0 = T(); ra = route_a(A, c, t); da = (T() - t0) * 1e3
                t0 = T(); rb = route_b(B, c, t); db = (T() - t0) * 1e3
                if not (ra[1] == rb[1] and ra[2] == rb[2] and np.array_equal(ra[0], rb[0], equal_nan=True)):
                    say("  round %d contrast (%d, %d): the two routes DIFFER" % (r, c, t))
                    return 1
                if timers:
                    ka, kb = A.timings(), B.timings()
                    say("  timers (%d, %d): route A K1 %.3f ms, transform %.3f ms | route B K1 %.3f ms, transform %.3f ms | %d passes, %d DEGs"
                        % (c, t, ka["k1_ms"], ka["transform_ms"], kb["k1_ms"], kb["transform_ms"], ra[1], ra[2][-1][0]))
                else:
                    ta[c, t].append(da); tb[c, t].append(db)
                    say("  round %d (%d, %d)  contrast %9.3f ms   columns + build_pairs %9.3f ms" % (r, c, t, da, db))
        info = A.info()
        say("  route A holds %d bytes of per-group counts (%d planes), shared_group_counts = %d"
            % (info["group_count_bytes"], C + 1, info["shared_group_counts"]))
    first = ta[contrasts[0]][0]
    say("  first contrast of route A (ranking + counting every group + classification + passes): %.3f ms" % first)
    alla = [v for ct in contrasts for v in ta[ct][1:]]
    allb = [v for ct in contrasts for v in tb[ct][1:]]
    for ct in contrasts:
        say("  (%d, %d)  contrast median %9.3f ms (%.3f .. %.3f)   columns + build_pairs median %9.3f ms (%.3f .. %.3f)"
            % (ct + (float(np.median(ta[ct][1:])), min(ta[ct][1:]), max(ta[ct][1:]), float(np.median(tb[ct][1:])), min(tb[ct][1:]), max(tb[ct][1:]))))
    say("  ms per contrast over rounds 1..%d: route A median %.3f (%.3f .. %.3f), route B median %.3f (%.3f .. %.3f)"
        % (rounds - 1, float(np.median(alla)), min(alla), max(alla), float(np.median(allb)), min(allb), max(allb)))
    for r in range(rounds):
        say("  round %d, all six contrasts: route A %.3f ms, route B %.3f ms" % (r, sum(ta[ct][r] for ct in contrasts), sum(tb[ct][r] for ct in contrasts)))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "contrasts_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/contrasts_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
