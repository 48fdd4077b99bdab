"""The label-permutation null of the best pair score (reo_top_pairs_null) at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0
family, two groups of 500, the workload of bench.py), B = 64 permutations, each route in a PROCESS of its own (this script starts itself
once per route and repeat, alternating the two):
  new      Context.top_pairs_null(permuted_sides(..., 64)) on a resident matrix: wall time of the whole call, and the kernel per permutation
           from HIP events (reo_get_info 39 / 64);
  replaced the route the call replaces, on the entry points the library had before it: per permutation set_groups(relabelled) +
           top_pairs(1) on the resident matrix -- a fresh transform and a full recount per permutation; wall time of all 64, and the
           histogram passes per permutation from HIP events (reo_get_info 36) divided by the passes;
  the yardstick: one histogram pass of top_pairs(1) under the observed labels (reo_get_info 36 / passes), measured in the `new` process.
Both routes must give the same 64 maxima.  Every repeat is printed, the median and the spread are reported.  Data with ties and other
sizes: not measured here.
Writes profiles/top_pairs_null_ab.txt.
python tools/top_pairs_null_ab.py [repeats]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

seed = 0x5EED0003
G, S, B = 20000, 1000, 64
T = time.perf_counter


def problem(pkg):
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    rows = pkg.permuted_sides(gid, 0, None, B, seed=1)
    return X, gid, len(lev), rows


def child(route):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    X, gid, ng, rows = problem(pkg)
    out = {"route": route}
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, ng); ctx.set_matrix(X)
        tp = ctx.top_pairs(1)                                                    # (warms the planes, the code objects and the pools)
        out["pass_ms"] = ctx.info()["top_pairs_hist_us"] / 1e3 / max(tp.passes, 1)
        out["has_ties"] = ctx.info()["has_ties"]
        if route == "new":
            ctx.top_pairs_null(rows[:1])                                         # (warm-up of the kernel's code object)
            t0 = T(); null = ctx.top_pairs_null(rows); out["wall_ms"] = (T() - t0) * 1e3
            info = ctx.info()
            out["kernel_ms_per_perm"] = info["top_pairs_null_us"] / 1e3 / B
            out["batch"] = info["top_pairs_null_batch"]
            out["max"] = null.max_num.tolist()
        else:
            mx, hist_ms = [], 0.0
            t0 = T()
            for p in range(B):
                ctx.set_groups((rows[p] != rows[p, 0]).astype(np.int32), 2)      # (group ids are numbered in order of first appearance)
                tp = ctx.top_pairs(1, a=0 if rows[p, 0] == 1 else 1)             # side A is the group of the row's ones
                mx.append(abs(int(tp.num[0])))
                hist_ms += ctx.info()["top_pairs_hist_us"] / 1e3 / max(tp.passes, 1)
            out["wall_ms"] = (T() - t0) * 1e3
            out["kernel_ms_per_perm"] = hist_ms / B
            out["max"] = mx
    print("RESULT " + json.dumps(out), flush=True)
    return 0


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    res = {"new": [], "replaced": []}
    for r in range(reps):
        for route in ("new", "replaced"):
            run = subprocess.run([sys.executable, sys.argv[0], "--child", route], capture_output=True, text=True, timeout=900)
            got = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not got:
                say("route %s, repeat %d FAILED (exit %d): %s" % (route, r, run.returncode, run.stderr[-500:]))
                return 1
            res[route].append(json.loads(got[-1][7:]))
    if any(x["max"] != res["new"][0]["max"] for x in res["new"] + res["replaced"]):
        say("the two routes DIFFER in the maxima")
        return 1

    def stat(route, key):
        v = [x[key] for x in res[route]]
        return float(np.median(v)), min(v), max(v), ", ".join("%.3f" % t for t in v)
    say("config 3: %d x %d (T0, groups 500 / 500, has_ties = %d), B = %d permutations, %d processes per route, alternating"
        % (G, S, res["new"][0]["has_ties"], B, reps))
    y = stat("new", "pass_ms")
    say("  yardstick: one histogram pass of top_pairs(1) under the observed labels (HIP events): median %.3f ms (%s)" % (y[0], y[3]))
    w, k = stat("new", "wall_ms"), stat("new", "kernel_ms_per_perm")
    say("  new (reo_top_pairs_null, batch %d): whole call median %.3f ms (%.3f .. %.3f; %s) = %.3f ms per permutation; kernel %.3f ms per "
        "permutation (%.3f .. %.3f; HIP events) = %.3f of one histogram pass"
        % (res["new"][0]["batch"], w[0], w[1], w[2], w[3], w[0] / B, k[0], k[1], k[2], k[0] / y[0]))
    w2, k2 = stat("replaced", "wall_ms"), stat("replaced", "kernel_ms_per_perm")
    say("  replaced (set_groups + top_pairs(1) per permutation): all %d median %.3f ms (%.3f .. %.3f; %s) = %.3f ms per permutation, of which "
        "the histogram passes %.3f ms per pass (%.3f .. %.3f; HIP events)" % (B, w2[0], w2[1], w2[2], w2[3], w2[0] / B, k2[0], k2[1], k2[2]))
    say("  whole call: %.1f x; the same %d maxima from both routes (largest |N| %d, smallest %d; 2 S_A S_B = %d)"
        % (w2[0] / w[0], B, max(res["new"][0]["max"]), min(res["new"][0]["max"]), 2 * 500 * 500))
    say("  data with ties, other sizes, other B: not measured")
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "top_pairs_null_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/top_pairs_null_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
