"""The label-permutation null two ways at config 3 size: 20 000 genes x 1 000 samples (T0 ranks, tie-free, the groups of synth.groups),
B = 64 permutations, ONE process, under a time limit of its own.
  batched  reo_perm_null on the resident table of comparison 0: the whole call on a host clock, and the launches of the permuted pair
           kernel between HIP events (reo_get_info 35), with the batch width it chose (reo_get_info 34)
  parent   the route that already works without the entry point, per permutation on a second context whose matrix stays resident:
           reo_set_groups(1 - row) + reo_compute_thresholds (set_groups drops them; host arithmetic) + reo_build_pairs(0), which ranks and
           slices the resident matrix again under the new labels, + reo_identify_degs(n_iter = 1); whole calls on a host clock, the
           transform and K1 stage timers beside it.  Group ids are numbered by first appearance, so the rows of this tool all put the first
           sample on side A (1 - row starts with 0); both legs get the same rows
The parent route is the baseline; it is never another variant of the new code.  The first `check` permutations of both legs must give the
same delta1, bit for bit, or the tool fails.  Writes profiles/perm_null_ab.txt.
python tools/perm_null_ab.py [B] [time limit in seconds]"""
import os
import signal
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0C99
T = time.perf_counter


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    signal.alarm(int(sys.argv[2]) if len(sys.argv) > 2 else 400)   # the tool ends itself: nothing is retried
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S = 20000, 1000
    X = np.asfortranarray(pkg.synth.t0_ranks(G, S, seed).astype(np.float64))
    gid = pkg.encode_groups(pkg.synth.groups(S))[0]
    ref = pkg.synth.ref_mask(G, 3000, seed)
    rows = pkg.permuted_labels(gid, 0, 4 * B + 16, seed=1)
    rows = rows[rows[:, 0] == 1][:B]                                                # (the parent route needs the first sample on side A)
    assert rows.shape[0] == B
    say("%d x %d Float64 T0 ranks, sides of %d / %d samples, B = %d permutations, reference set of %d genes held fixed, one pass each"
        % (G, S, int((gid == 0).sum()), int((gid != 0).sum()), B, int(ref.sum())))

    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 2)
        ctx.compute_thresholds(0.01)
        ctx.set_matrix(X)
        ctx.build_pairs(0)
        ctx.identify_degs(ref, 1.0, 0.05, 1, 0)
        ctx.permutation_null(rows[:2], ref_mask=ref)                                  # warm-up: buffers, code objects
        t0 = T()
        pn = ctx.permutation_null(rows, ref_mask=ref, keep_null=True)
        t_batched = (T() - t0) * 1e3
        info = ctx.info()
    k_ms = info["perm_kernel_us"] / 1e3
    say("batched  reo_perm_null: %.1f ms for the whole call (%.2f ms per permutation); batch width %d; permuted pair kernel %.2f ms in all "
        "= %.3f ms per permutation (HIP events)" % (t_batched, t_batched / B, info["perm_batch"], k_ms, k_ms / B))

    check = min(B, 4)
    t_parent, k1, tr = [], [], []
    with pkg.Context(device=0, seed=seed) as c2:
        c2.set_profiling(True)
        c2.set_matrix(X)
        for p in range(B + 1):                                                        # permutation 0 twice: the first round warms up
            row = rows[max(p - 1, 0)]
            gid2 = (1 - row).astype(np.int32)
            c2.reset_timings()
            t0 = T()
            c2.set_groups(gid2, 2)
            c2.compute_thresholds(0.01)
            c2.build_pairs(0)
            res = c2.identify_degs(ref, 1.0, 0.05, 1, 0)[0]
            dt = (T() - t0) * 1e3
            if p == 0:
                continue
            t_parent.append(dt)
            tm = c2.timings()
            k1.append(tm["k1_ms"])
            tr.append(tm["transform_ms"])
            if p - 1 < check and not np.array_equal(res[:, 11], pn.delta1_null[p - 1]):
                say("permutation %d: the two routes DIFFER in delta1" % (p - 1))
                return 1
    say("parent   set_groups + compute_thresholds + build_pairs + identify_degs(n_iter = 1), matrix resident: %.1f ms for %d permutations, median "
        "%.2f ms per permutation (%.2f .. %.2f); stage timers, medians per build: transform %.3f ms, K1 %.3f ms"
        % (sum(t_parent), B, float(np.median(t_parent)), min(t_parent), max(t_parent), float(np.median(tr)), float(np.median(k1))))
    say("the first %d permutations give the same delta1 on both routes, bit for bit" % check)
    say("whole call: batched / parent = %.2f;  pair kernel per permutation: batched %.3f ms against K1 %.3f ms = %.2f"
        % (t_batched / sum(t_parent), k_ms / B, float(np.median(k1)), (k_ms / B) / max(float(np.median(k1)), 1e-9)))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "perm_null_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/perm_null_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
