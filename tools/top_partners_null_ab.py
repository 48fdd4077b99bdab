"""The label-permutation null of a gene's best partner score (reo_top_partners_null) at BASELINE config 3 (synthetic 20 000 genes x 1 000
samples, T0 family, two groups of 500, the workload of bench.py), B = 64 permutations, for (a) 300 query genes and (b) all genes, each
route in a PROCESS of its own (this script starts itself once per route and repeat, alternating the two):
  new      Context.top_partners_null(permuted_sides(..., 64), genes) on a resident matrix: wall time of the whole call, and the kernel per
           permutation from HIP events (reo_get_info 45 / 64);
  replaced the route the call replaces, on the entry points the library had before it: per permutation set_groups(relabelled) +
           top_partners(genes, 1) on the resident matrix -- a fresh transform and a full recount per permutation; wall time of all 64;
  the yardstick: reo_top_pairs_null's kernel per permutation on the same context and rows (reo_get_info 39 / 64), measured in the `new`
           process: it walks half the square, so all genes here should cost about twice it;
  ties     once, in a process of its own: the new route on the same ranks divided by 4 (ties everywhere: the le chain and the eq counters).
Both routes must give the same maxima: asserted per process before anything is timed (the `replaced` process runs the new call once for
that).  Every repeat is printed, the median and the spread are reported.
Writes profiles/top_partners_null_ab.txt.
python tools/top_partners_null_ab.py [repeats]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

seed = 0x5EED0003
G, S, B, Q = 20000, 1000, 64, 300
T = time.perf_counter


def problem(pkg, ties=False):
    X = pkg.synth.t0_ranks(G, S, seed)
    if ties:
        X = np.asfortranarray(np.asarray(X) // 4)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    rows = pkg.permuted_sides(gid, 0, None, B, seed=1)
    few = np.sort(np.random.default_rng(7).choice(G, Q, replace=False)).astype(np.int32)
    return X, gid, len(lev), rows, few


def old_route(ctx, rows, genes):
    mx = np.zeros((rows.shape[0], G if genes is None else genes.size), dtype=np.int64)
    for p in range(rows.shape[0]):
        ctx.set_groups((rows[p] != rows[p, 0]).astype(np.int32), 2)              # (group ids are numbered in order of first appearance)
        tp = ctx.top_partners(genes, 1, a=0 if rows[p, 0] == 1 else 1)           # side A is the group of the row's ones
        mx[p] = np.abs(tp.num[:, 0])
    return mx


def child(route):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    X, gid, ng, rows, few = problem(pkg, ties=route == "ties")
    out = {"route": route}
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, ng); ctx.set_matrix(X)
        ctx.top_partners_null(rows[:1], few)                                     # (warms the planes, the code objects and the pools)
        out["has_ties"] = ctx.info()["has_ties"]
        ref = {"few": ctx.top_partners_null(rows, few).max_num, "all": ctx.top_partners_null(rows).max_num}
        if route == "replaced":                                                  # equal maxima before anything is timed
            for key, genes in (("few", few), ("all", None)):
                assert np.array_equal(old_route(ctx, rows[:2], genes), ref[key][:2]), key
            ctx.set_groups(gid, ng)
        if route in ("new", "ties"):
            ctx.top_pairs_null(rows[:1])
            ctx.top_pairs_null(rows)
            out["yard_ms_per_perm"] = ctx.info()["top_pairs_null_us"] / 1e3 / B
            for key, genes in (("few", few), ("all", None)):
                t0 = T(); null = ctx.top_partners_null(rows, genes); out[key + "_wall_ms"] = (T() - t0) * 1e3
                info = ctx.info()
                out[key + "_kernel_ms_per_perm"] = info["top_partners_null_us"] / 1e3 / B
                out["batch"] = info["top_partners_null_batch"]
                assert np.array_equal(null.max_num, ref[key])
                out[key + "_sum"] = int(null.max_num.sum())
        else:
            for key, genes in (("few", few), ("all", None)):
                t0 = T(); mx = old_route(ctx, rows, genes); out[key + "_wall_ms"] = (T() - t0) * 1e3
                assert np.array_equal(mx, ref[key]), key
                out[key + "_sum"] = int(mx.sum())
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

    def run_child(route):
        run = subprocess.run([sys.executable, sys.argv[0], "--child", route], capture_output=True, text=True, timeout=900)
        got = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
        if run.returncode != 0 or not got:
            say("route %s FAILED (exit %d): %s" % (route, run.returncode, run.stderr[-500:]))
            return None
        return json.loads(got[-1][7:])

    res = {"new": [], "replaced": []}
    for r in range(reps):
        for route in ("new", "replaced"):
            one = run_child(route)
            if one is None:
                return 1
            res[route].append(one)
    if any(x[k] != res["new"][0][k] for x in res["new"] + res["replaced"] for k in ("few_sum", "all_sum")):
        say("the two routes DIFFER in the maxima")
        return 1

    def stat(route, key):
        v = [x[key] for x in res[route]]
        return float(np.median(v)), min(v), max(v), ", ".join("%.3f" % t for t in v)
    say("config 3: %d x %d (T0, groups 500 / 500, has_ties = %d), B = %d permutations, %d processes per route, alternating"
        % (G, S, res["new"][0]["has_ties"], B, reps))
    y = stat("new", "yard_ms_per_perm")
    say("  yardstick: k_top_pairs_null per permutation on the same context and rows (HIP events): median %.3f ms (%s)" % (y[0], y[3]))
    for key, what in (("few", "%d query genes" % Q), ("all", "all %d genes" % G)):
        w, k = stat("new", key + "_wall_ms"), stat("new", key + "_kernel_ms_per_perm")
        say("  new (reo_top_partners_null, batch %d), %s: whole call median %.3f ms (%.3f .. %.3f; %s) = %.3f ms per permutation; kernel %.3f ms "
            "per permutation (%.3f .. %.3f; HIP events) = %.2f x the yardstick"
            % (res["new"][0]["batch"], what, w[0], w[1], w[2], w[3], w[0] / B, k[0], k[1], k[2], k[0] / y[0]))
        w2 = stat("replaced", key + "_wall_ms")
        say("  replaced (set_groups + top_partners(genes, 1) per permutation), %s: all %d median %.3f ms (%.3f .. %.3f; %s) = %.3f ms per "
            "permutation; whole call %.1f x; the same %d x %d maxima from both routes"
            % (what, B, w2[0], w2[1], w2[2], w2[3], w2[0] / B, w2[0] / w[0], B, Q if key == "few" else G))
    t = run_child("ties")
    if t is None:
        say("  data with ties: not timed")
    else:
        say("  data with ties (the same ranks divided by 4, has_ties = %d), one process: %d query genes whole call %.3f ms, kernel %.3f ms per "
            "permutation; all genes whole call %.3f ms, kernel %.3f ms per permutation = %.2f x k_top_pairs_null's %.3f ms on that data"
            % (t["has_ties"], Q, t["few_wall_ms"], t["few_kernel_ms_per_perm"], t["all_wall_ms"], t["all_kernel_ms_per_perm"],
               t["all_kernel_ms_per_perm"] / t["yard_ms_per_perm"], t["yard_ms_per_perm"]))
    say("  one size, nothing tuned; other sizes, other B: not measured")
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "top_partners_null_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/top_partners_null_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
