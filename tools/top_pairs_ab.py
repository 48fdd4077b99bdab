"""The top-scoring-pair search (reo_top_pairs) at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family, two groups of 500, the
workload of bench.py), n = 100 and n = 100 000, in ONE process on one context:
  whole call      wall time of Context.top_pairs (rank shift, histogram passes, emit pass, copies, host sort), every repeat (the first
                  dropped) and the median;
  passes          histogram passes of the selection, and the same call with REO_TOP_PAIRS_CAP = n (the deepest refinement);
  per pass        device time of the histogram passes and of the emit pass by HIP events (reo_get_info 36, 37), divided by the passes;
  the yardstick   the pair kernel of a plain reo_build_pairs(0) on the same context (stage timer k1_ms): what one pass repeats.
The host route it replaces: reo_pair_counts in row strips plus a numpy top-k of |N| over them, timed at the first 4 000 genes of the same
matrix (its |N| must equal the search's) and scaled by (20 000 / 4 000)^2 -- labelled "extrapolated", not measured.
Writes profiles/top_pairs_ab.txt.
python tools/top_pairs_ab.py [repeats]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter


def host_route(ctx, G, n, s_a, s_b, strip=500):
    """the n largest |N| over i < j through reo_pair_counts strips and numpy; returns them sorted descending"""
    best = np.zeros(0, dtype=np.int64)
    for i0 in range(0, G, strip):
        i1 = min(G, i0 + strip)
        gt, eq = ctx.pair_counts(i0, i1, 0, G)
        gt, eq = gt.astype(np.int64), eq.astype(np.int64)
        N = (2 * gt[:, :, 0] + eq[:, :, 0] - s_a) * s_b - (2 * gt[:, :, 1] + eq[:, :, 1] - s_b) * s_a
        upper = np.arange(G)[None, :] > np.arange(i0, i1)[:, None]
        a = np.abs(N[upper])
        if a.size > n:
            a = a[np.argpartition(a, a.size - n)[a.size - n:]]
        best = np.concatenate([best, a])
        if best.size > n:
            best = best[np.argpartition(best, best.size - n)[best.size - n:]]
    return np.sort(best)[::-1]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S, Gs = 20000, 1000, 4000
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    s_a = int((gid == 0).sum())
    s_b = S - s_a
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_profiling(True)
        ctx.set_matrix(X); ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01)
        k1 = []
        for r in range(reps):
            ctx.reset_timings()
            ctx.build_pairs(0)
            ctx.get_codes(0, 1, 0, 2)                                            # (waits for the build)
            k1.append(float(ctx.timings()["k1_ms"]))
        k1_ms = float(np.median(k1[1:] if len(k1) > 1 else k1))
        say("config 3: %d x %d (T0, groups %d / %d), %d repeats, the first dropped" % (G, S, s_a, s_b, reps))
        say("  yardstick: the pair kernel of a plain reo_build_pairs(0), stage timer k1_ms: median %.3f ms (%s)"
            % (k1_ms, ", ".join("%.3f" % v for v in k1)))
        for n in (100, 100000):
            for cap in (None, n):
                if cap is None:
                    os.environ.pop("REO_TOP_PAIRS_CAP", None)
                else:
                    os.environ["REO_TOP_PAIRS_CAP"] = str(cap)
                wall, hist_us, emit_us, passes = [], [], [], 0
                first = None
                for r in range(reps):
                    t0 = T(); tp = ctx.top_pairs(n); wall.append((T() - t0) * 1e3)
                    info = ctx.info()
                    hist_us.append(info["top_pairs_hist_us"]); emit_us.append(info["top_pairs_emit_us"]); passes = tp.passes
                    if first is None:
                        first = tp
                    elif not all(np.array_equal(getattr(tp, f), getattr(first, f)) for f in ("gene_i", "gene_j", "n_gt", "n_eq", "num", "rank_num")):
                        say("  n = %d: two calls DIFFER" % n)
                        return 1
                w = wall[1:] if len(wall) > 1 else wall
                h = float(np.median(hist_us[1:] if len(hist_us) > 1 else hist_us)) / 1e3
                e = float(np.median(emit_us[1:] if len(emit_us) > 1 else emit_us)) / 1e3
                say("  n = %6d, %s: whole call median %9.3f ms (%.3f .. %.3f); %d histogram passes, %.3f ms on the device = %.3f ms per pass = "
                    "%.2f plain pair kernels; emit pass %.3f ms; score of the first pair %.4f, of the last %.4f"
                    % (n, "default capacity" if cap is None else "REO_TOP_PAIRS_CAP = n", float(np.median(w)), min(w), max(w), passes, h,
                       h / max(passes, 1), h / max(passes, 1) / k1_ms, e, tp.score[0], tp.score[-1]))
        os.environ.pop("REO_TOP_PAIRS_CAP", None)
    # the host route, at the first Gs genes of the same matrix
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_matrix(np.asfortranarray(X[:Gs])); ctx.set_groups(gid, len(lev))
        t_host, t_dev = [], []
        for r in range(max(2, reps // 2)):
            t0 = T(); best = host_route(ctx, Gs, 100, s_a, s_b); t_host.append((T() - t0) * 1e3)
            t0 = T(); tp = ctx.top_pairs(100); t_dev.append((T() - t0) * 1e3)
            if not np.array_equal(best, np.abs(tp.num)):
                say("  the host route and the search DIFFER at %d genes" % Gs)
                return 1
        th, td = float(np.median(t_host[1:])) if len(t_host) > 1 else t_host[0], float(np.median(t_dev[1:])) if len(t_dev) > 1 else t_dev[0]
        say("  host route (reo_pair_counts strips of 500 rows + numpy top-k of |N|, n = 100) at %d genes: %.1f ms measured; the search there: %.3f ms, "
            "the same |N|" % (Gs, th, td))
        say("  host route at %d genes: %.1f s extrapolated (x %d, the square of the gene ratio; not measured)" % (G, th * (G / Gs) ** 2 / 1e3, int((G / Gs) ** 2)))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "top_pairs_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/top_pairs_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
