"""Leave-one-out cross-validation of the k-TSP selection (reo_top_pairs_loo) at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples,
tie-free T0 ranks, two groups of 500, the size of tools/top_pairs_ab.py), kmax = 9, each route in a PROCESS of its own (this script starts
itself once per route and repeat, alternating the two):
  new      Context.top_pairs_loo(9) on a resident matrix: wall time of the whole call, its two kernels from HIP events (reo_get_info 40 /
           41: k_loo_words, k_loo_select), the cut and the number of candidates; the rest of the wall time is step 1 (the full-data list
           that gives the cut), the emit pass and the copies;
  replaced the route the call replaces, on the entry points the library had before it, per fold: set_groups with the sample set aside in a
           group of its own + top_pairs(n) + disjoint(9) + pair_support(outcomes=True), n = the depth that step 1 of the new call needs
           (1 024 doubled until the full-data list holds 18 disjoint pairs).  Timed on the first FOLDS = 32 folds and SCALED to all 1 000
           (the folds cost the same: each is a fresh transform and a full search); the output says so.
The first 32 folds must be equal field by field.  Every repeat is printed, the median and the spread are reported.  Data with ties and
other sizes: not measured here.
Writes profiles/top_pairs_loo_ab.txt.
python tools/top_pairs_loo_ab.py [repeats]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")

seed = 0x5EED0003
G, S, KMAX, FOLDS = 20000, 1000, 9, 32
T = time.perf_counter


def depth(ctx):
    """the list depth at which the greedy walk of the full data yields 2 kmax disjoint pairs: what step 1 of the call runs"""
    n = 1024
    while n < 1 << 20 and ctx.top_pairs(n).disjoint(2 * KMAX).size < 2 * KMAX:
        n *= 2
    return n


def child(route):
    import __graft_entry__ as ge
    pkg = ge.load_pkg()
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    out = {"route": route}
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.set_matrix(X)
        t0 = T(); n = depth(ctx); out["depth"] = n                               # (warms the planes, the code objects and the pools)
        t0 = T(); ctx.top_pairs(n); out["top_pairs_ms"] = (T() - t0) * 1e3
        out["has_ties"] = ctx.info()["has_ties"]
        if route == "new":
            ctx.top_pairs_loo(1)                                                 # (warm-up of the two kernels' code objects)
            t0 = T(); loo = ctx.top_pairs_loo(KMAX); out["wall_ms"] = (T() - t0) * 1e3
            info = ctx.info()
            out["words_ms"], out["select_ms"] = info["top_pairs_loo_words_us"] / 1e3, info["top_pairs_loo_select_us"] / 1e3
            out["cut"], out["n_candidates"] = loo.cut, loo.n_candidates
            out["errors"] = {k: v.tolist() for k, v in loo.errors().items()}
            out["best_k"] = loo.best_k()
            picks = (loo.gene_i[:FOLDS], loo.gene_j[:FOLDS], loo.num[:FOLDS], loo.rank_num[:FOLDS], loo.outcome[:FOLDS])
        else:
            rows = [[] for _ in range(5)]
            t0 = T()
            for s in range(FOLDS):
                g = np.where(gid == 0, 0, 1).astype(np.int32)
                g[s] = 2
                _, first = np.unique(g, return_index=True)                       # (group ids are numbered in order of first appearance)
                number = np.empty(3, dtype=np.int32)
                number[np.argsort(first)] = np.arange(3)
                ctx.set_groups(number[g], 3)
                tp = ctx.top_pairs(n, a=int(number[0]), b=int(number[1]))
                at = tp.disjoint(KMAX)
                ps = ctx.pair_support((tp.gene_i[at], np.arange(at.size + 1, dtype=np.int64), tp.gene_j[at]), outcomes=True)
                for q, v in enumerate((tp.gene_i[at], tp.gene_j[at], tp.num[at], tp.rank_num[at], ps.outcome[:, s].astype(np.int64) - 1)):
                    rows[q].append(v)
            out["wall_ms"] = (T() - t0) * 1e3
            picks = [np.stack(r) for r in rows]
        out["picks"] = [np.asarray(p).astype(np.int64).tolist() for p in picks]
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
    if any(x["picks"] != res["new"][0]["picks"] for x in res["new"] + res["replaced"]):
        say("the two routes DIFFER in the first %d folds" % FOLDS)
        return 1

    def stat(route, key):
        v = [x[key] for x in res[route]]
        return float(np.median(v)), min(v), max(v), ", ".join("%.3f" % t for t in v)
    new = res["new"][0]
    say("config 3: %d x %d (T0, groups 500 / 500, has_ties = %d), kmax = %d, %d folds, %d processes per route, alternating"
        % (G, S, new["has_ties"], KMAX, S, reps))
    say("  step 1 needs a full-data list of n = %d pairs for %d disjoint ones; one top_pairs(n) takes %.3f ms (median, whole call)"
        % (new["depth"], 2 * KMAX, stat("new", "top_pairs_ms")[0]))
    w, kw, ks = stat("new", "wall_ms"), stat("new", "words_ms"), stat("new", "select_ms")
    say("  new (reo_top_pairs_loo): cut T = %d, %d candidates of %d pairs; whole call median %.3f ms (%.3f .. %.3f; %s) = %.3f ms per fold"
        % (new["cut"], new["n_candidates"], G * (G - 1) // 2, w[0], w[1], w[2], w[3], w[0] / S))
    say("    of which k_loo_words %.3f ms (%.3f .. %.3f), k_loo_select %.3f ms (%.3f .. %.3f) (HIP events); the rest, %.3f ms, is step 1, the "
        "emit pass and the copies" % (kw[0], kw[1], kw[2], ks[0], ks[1], ks[2], w[0] - kw[0] - ks[0]))
    w2 = stat("replaced", "wall_ms")
    say("  replaced (set_groups + top_pairs(%d) + disjoint(%d) + pair_support per fold): %d folds median %.3f ms (%.3f .. %.3f; %s) = %.3f ms "
        "per fold; SCALED to %d folds: %.1f ms (not run in full)" % (new["depth"], KMAX, FOLDS, w2[0], w2[1], w2[2], w2[3], w2[0] / FOLDS, S, w2[0] / FOLDS * S))
    say("  whole call against the scaled per-fold route: %.1f x; the first %d folds are equal field by field" % (w2[0] / FOLDS * S / w[0], FOLDS))
    e = new["errors"]
    say("  the read-out: leave-one-out errors (wrong + undecided) of k = 1 .. %d: %s of %d folds; best odd k = %d"
        % (KMAX, [a + b for a, b in zip(e["n_wrong"], e["n_undecided"])], e["n_folds"][0], new["best_k"]))
    say("  one size, tie-free data, nothing tuned; data with ties, other sizes, other kmax: not measured")
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "top_pairs_loo_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/top_pairs_loo_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
