"""The top partners of a gene (reo_top_partners) at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, tie-free T0 ranks, two
groups of 500, the size of tools/top_pairs_ab.py), each route in a PROCESS of its own (this script starts itself once per route and
repeat, alternating the two):
  new      on a resident matrix: Context.top_partners(300 seeded query genes, m = 10) and Context.top_partners(all genes, m = 1) -- wall
           time of each whole call and its two kernels from HIP events (reo_get_info 42 / 43: the launches of k_top_partners_count and of
           k_top_partners_select) -- and, for comparison, one histogram pass of top_pairs(1) of the same context (reo_get_info 36 /
           passes): the count kernel for all genes walks twice the pairs of such a pass and stores a cell per pair;
  replaced the route the 300-gene call replaces, on the entry points the library had before it: reo_pair_counts in strips over the query
           rows (one strip of one row and all columns per query gene) plus N, Gamma from rank_shift and a numpy sort per row.
The 300 rows of the two routes must be equal: partner, N and Gamma.  Every repeat is printed, the median and the spread are reported.
Data with ties and other sizes: not measured here.
Writes profiles/top_partners_ab.txt.
python tools/top_partners_ab.py [repeats]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

seed = 0x5EED0003
G, S, Q, M = 20000, 1000, 300, 10
T = time.perf_counter


def child(route):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    s_a = int((gid == 0).sum())
    s_b = S - s_a
    genes = np.sort(np.random.default_rng(seed).choice(G, size=Q, replace=False)).astype(np.int32)
    out = {"route": route}
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.set_matrix(X); ctx.compute_thresholds(0.01)
        one = ctx.top_pairs(1)                                                   # (warms the planes, the code objects and the pools)
        out["has_ties"] = ctx.info()["has_ties"]
        if route == "new":
            one = ctx.top_pairs(1)
            info = ctx.info()
            out["hist_pass_ms"], out["passes"] = info["top_pairs_hist_us"] / 1e3 / max(one.passes, 1), one.passes
            ctx.top_partners(genes[:8], 1)                                       # (warm-up of the two kernels' code objects)
            t0 = T(); tp = ctx.top_partners(genes, M); out["wall_ms"] = (T() - t0) * 1e3
            info = ctx.info()
            out["count_ms"], out["select_ms"] = info["top_partners_count_us"] / 1e3, info["top_partners_select_us"] / 1e3
            t0 = T(); every = ctx.top_partners(); out["all_wall_ms"] = (T() - t0) * 1e3
            info = ctx.info()
            out["all_count_ms"], out["all_select_ms"] = info["top_partners_count_us"] / 1e3, info["top_partners_select_us"] / 1e3
            pairs = every.pairs()
            out["best_is_top_pair"] = bool((pairs.gene_i[0], pairs.gene_j[0], pairs.num[0]) == (one.gene_i[0], one.gene_j[0], one.num[0]))
            rows = (tp.partner, tp.num, tp.rank_num)
        else:
            ctx.pair_counts(0, 1, 0, G)                                          # (warm-up)
            t0 = T()
            D = ctx.rank_shift()
            partner, num, gam = [], [], []
            for q in genes:
                gt, eq = ctx.pair_counts(int(q), int(q) + 1, 0, G)
                gt, eq = gt[0].astype(np.int64), eq[0].astype(np.int64)
                N = (2 * gt[:, 0] + eq[:, 0] - s_a) * s_b - (2 * gt[:, 1] + eq[:, 1] - s_b) * s_a
                Gam = np.abs(D[q] - D)
                p = np.delete(np.arange(G), q)
                order = p[np.lexsort((p, -Gam[p], -np.abs(N[p])))][:M]
                partner.append(order); num.append(N[order]); gam.append(Gam[order])
            out["wall_ms"] = (T() - t0) * 1e3
            rows = (np.stack(partner), np.stack(num), np.stack(gam))
        out["rows"] = [np.asarray(r).astype(np.int64).tolist() for r in rows]
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
            run = subprocess.run([sys.executable, sys.argv[0], "--child", route], capture_output=True, text=True, timeout=400)
            got = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
            if run.returncode != 0 or not got:
                say("route %s, repeat %d FAILED (exit %d): %s" % (route, r, run.returncode, run.stderr[-800:]))
                return 1
            res[route].append(json.loads(got[-1][7:]))
    if any(x["rows"] != res["new"][0]["rows"] for x in res["new"] + res["replaced"]):
        say("the two routes DIFFER in the %d rows" % Q)
        return 1

    def stat(route, key):
        v = [x[key] for x in res[route]]
        return float(np.median(v)), min(v), max(v), ", ".join("%.3f" % t for t in v)
    new = res["new"][0]
    say("config 3: %d x %d (T0, groups 500 / 500, has_ties = %d), %d processes per route, alternating" % (G, S, new["has_ties"], reps))
    w, kc, ks = stat("new", "wall_ms"), stat("new", "count_ms"), stat("new", "select_ms")
    say("  new (reo_top_partners), %d query genes, m = %d: whole call median %.3f ms (%.3f .. %.3f; %s)" % (Q, M, w[0], w[1], w[2], w[3]))
    say("    of which k_top_partners_count %.3f ms (%.3f .. %.3f), k_top_partners_select %.3f ms (%.3f .. %.3f) (HIP events); the rest, %.3f ms, "
        "is the rank shift, the copies and the host" % (kc[0], kc[1], kc[2], ks[0], ks[1], ks[2], w[0] - kc[0] - ks[0]))
    w, kc, ks = stat("new", "all_wall_ms"), stat("new", "all_count_ms"), stat("new", "all_select_ms")
    say("  new, all %d genes, m = 1: whole call median %.3f ms (%.3f .. %.3f; %s)" % (G, w[0], w[1], w[2], w[3]))
    say("    of which k_top_partners_count %.3f ms (%.3f .. %.3f), k_top_partners_select %.3f ms (%.3f .. %.3f) (HIP events)"
        % (kc[0], kc[1], kc[2], ks[0], ks[1], ks[2]))
    h = stat("new", "hist_pass_ms")
    say("  for comparison: one histogram pass of top_pairs(1) (%d passes) %.3f ms (%.3f .. %.3f); the count kernel for all genes walks twice its "
        "pairs and stores a cell per pair: %.2f x that pass" % (new["passes"], h[0], h[1], h[2], kc[0] / h[0]))
    say("  the first pair of top_partners(all genes, m = 1).pairs() is top_pairs(1)'s pair: %s" % all(x["best_is_top_pair"] for x in res["new"]))
    w2 = stat("replaced", "wall_ms")
    say("  replaced (rank_shift + reo_pair_counts, one strip per query row, + numpy N, Gamma and a sort per row), %d query genes: median %.3f ms "
        "(%.3f .. %.3f; %s)" % (Q, w2[0], w2[1], w2[2], w2[3]))
    say("  whole call against the replaced route: %.1f x; the %d rows are equal (partner, N, Gamma)" % (w2[0] / stat("new", "wall_ms")[0], Q))
    say("  one size, tie-free data, nothing tuned; data with ties, other sizes, other m: not measured")
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "top_partners_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/top_partners_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
