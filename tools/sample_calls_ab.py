"""Per-sample calls of ALL genes at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family, the workload of bench.py), after a
real identify_degs (n_iter = 128, n_conv = 5), formed two ways that alternate in ONE process on one context:
  route A   sample_tests(counts=False).calls(pval_deg, padj_deg): both tails copied back as doubles (320 MB), then the two-sided value,
            Benjamini-Hochberg down every sample column (an argsort per column) and the thresholds in numpy;
  route B   sample_calls(pval_deg, padj_deg): reo_sample_calls -- the same tails stay on the device, rank / cut / emit there, one byte per
            cell comes back (20 MB).
The calls must be equal byte for byte, and the cuts equal the host's counts of padj <= padj_deg; the run stops otherwise.  Route A's two
halves (the device call with its copies, the numpy step) are timed apart as well.
No speed is promised and none is asserted.  Whole calls are timed -- uploads, launches, copies back, waits; the kernels alone are not timed.
With a built checkout of the parent commit as the second argument, bench.py --gpus 1 --steps 20 --warmup 5 is then run with this
build and in that checkout in turn, each run a process of its own, and both spreads are recorded: the headline must not move.
Writes profiles/sample_calls_ab.txt.
python tools/sample_calls_ab.py [repeats] [built checkout of the parent] [bench rounds]"""
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter
PVAL_DEG, PADJ_DEG = 1.0, 0.05


def bench_value(tree):
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=tree, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise RuntimeError("bench.py ended with %d: %s" % (out.returncode, out.stderr[-500:]))
    return float(json.loads(out.stdout.strip().splitlines()[-1])["value"])


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    parent = sys.argv[2] if len(sys.argv) > 2 else None
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
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
        result, iters, trace = ctx.identify_degs(ref0, PVAL_DEG, PADJ_DEG, 128, 5)
        ref = ctx.ref_mask()
        say("config 3: %d x %d, %d passes, %d reference genes in the last pass; all %d genes queried at pval_deg %g, padj_deg %g; "
            "%d repeats of each route in turn, the first dropped" % (G, S, iters, int(ref.sum()), G, PVAL_DEG, PADJ_DEG, reps))
        t = {"A device call": [], "A numpy step": [], "A whole": [], "B whole": []}
        for r in range(reps):
            t0 = T(); st = ctx.sample_tests(counts=False); t1 = T(); host = st.calls(PVAL_DEG, PADJ_DEG); t2 = T()
            t["A device call"].append((t1 - t0) * 1e3); t["A numpy step"].append((t2 - t1) * 1e3); t["A whole"].append((t2 - t0) * 1e3)
            t0 = T(); dev = ctx.sample_calls(PVAL_DEG, PADJ_DEG); t["B whole"].append((T() - t0) * 1e3)
            if np.ascontiguousarray(dev.calls).tobytes() != host.tobytes():
                say("  repeat %d: the calls of the two routes DIFFER in %d cells" % (r, int((dev.calls != host).sum())))
                return 1
            say("  repeat %d  A: sample_tests(counts=False) %10.3f ms + .calls %10.3f ms = %10.3f ms   B: sample_calls %10.3f ms"
                % (r, t["A device call"][-1], t["A numpy step"][-1], t["A whole"][-1], t["B whole"][-1]))
        cut = (st.padj() <= PADJ_DEG).sum(axis=0)
        if not (np.array_equal(dev.cut, cut) and np.array_equal(dev.n_up, (host == 1).sum(axis=0)) and np.array_equal(dev.n_down, (host == -1).sum(axis=0))):
            say("  the cuts or the counts of the two routes DIFFER")
            return 1
        say("  equal byte for byte in every repeat: %d up, %d down of %d cells; %d genes with at least one call; cuts between %d and %d of %d rows"
            % (int(dev.n_up.sum()), int(dev.n_down.sum()), host.size, int((host != 0).any(axis=1).sum()), int(dev.cut.min()), int(dev.cut.max()), G))
        say("  bytes to the host per call: route A %d (two tails), route B %d (calls) + %d (cut, n_up, n_down); resident on the device during "
            "route B: %d bytes of cell words" % (st.p_up.nbytes * 2, dev.calls.nbytes, 3 * dev.cut.nbytes, 4 * ((G + 31) // 32 * 32) * S))
        for k in ("A device call", "A numpy step", "A whole", "B whole"):
            v = t[k][1:] if len(t[k]) > 1 else t[k]
            say("  median %-14s %12.3f ms (%.3f .. %.3f)" % (k, float(np.median(v)), min(v), max(v)))
        say("  whole calls were timed (uploads, launches, copies back, waits); the kernels alone were not timed; no speed is promised")
    if parent:
        vals = {"this build": [], "parent": []}
        for r in range(rounds):
            for name, tree in (("parent", parent), ("this build", ".")) if r % 2 == 0 else (("this build", "."), ("parent", parent)):
                vals[name].append(bench_value(tree))
                say("  bench round %d  %-10s %.4e comparisons/s" % (r, name, vals[name][-1]))
        for name in ("parent", "this build"):
            v = vals[name]
            say("  bench.py --gpus 1 --steps 20 --warmup 5, %-10s median %.4e (%.4e .. %.4e), %d runs in turn" % (name, float(np.median(v)), min(v), max(v), len(v)))
        lo, hi = min(vals["parent"]), max(vals["parent"])
        m = float(np.median(vals["this build"]))
        say("  this build's median lies %s the parent's spread" % ("inside" if lo <= m <= hi else ("ABOVE" if m > hi else "BELOW")))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "sample_calls_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/sample_calls_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
