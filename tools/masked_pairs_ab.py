"""The masked build against the plain pair kernel on the same matrix: 10 000 genes x 400 samples, two groups of 200, Float64 (T0 family:
per-sample ranks, tie-free), 20 % of the cells missing at random -- and the same with an all-ones mask.  In ONE process and on ONE
context the two builds alternate round by round:
  plain    reo_build_pairs(0)            (thresholds of pval_reo = 0.01; the hand-scheduled pair kernel, slot order)
  masked   reo_build_pairs_masked(0, 0.01, default min_complete)
Each timing is a host clock around the WHOLE call and a one-row reo_get_codes behind it, which ends in a wait for the context's stream
(the builds return with their kernel in flight; the library's stream is its own, so no event of the caller's brackets it).  The matrix,
the mask, the bit planes and -- after the warm-up round -- the validity words and threshold tables are on the device before anything is
timed.  With the all-ones mask the two tables must be equal row strip by row strip, or the tool fails.
Reported: ms per build for both (median and range over the rounds after the first) and the ratio of the medians.
Writes profiles/masked_pairs_ab.txt.
python tools/masked_pairs_ab.py [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0B30
T = time.perf_counter


def main():
    rounds = max(int(sys.argv[1]) if len(sys.argv) > 1 else 6, 4)   # the first round warms up; at least three are measured
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S = 10000, 400
    X = pkg.synth.t0_ranks(G, S, seed).astype(np.float64)
    gid = (np.arange(S) >= S // 2).astype(np.int32)
    rng = np.random.default_rng(seed)
    masks = (("20 % missing", rng.random((G, S)) >= 0.20), ("all-ones mask", np.ones((G, S), dtype=bool)))
    say("%d x %d Float64, two groups of %d, T0 ranks; %d rounds per mask, the first apart; whole calls up to a stream wait" % (G, S, S // 2, rounds))

    def timed(fn, ctx):
        t0 = T()
        fn()
        ctx.get_codes(0, 1, 0, 2)   # (the wait)
        return (T() - t0) * 1e3

    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 2)
        ctx.set_matrix(X)
        ctx.compute_thresholds(0.01)
        for name, V in masks:
            ctx.set_valid_mask(V)
            tp, tm = [], []
            for r in range(rounds):
                tp.append(timed(lambda: ctx.build_pairs(0), ctx))
                slot = ctx.info()["k1_slot_order"]
                tm.append(timed(lambda: ctx.build_pairs_masked(0, 0.01), ctx))
                say("  %-14s round %d  plain %9.3f ms (slot order %d)   masked %9.3f ms" % (name, r, tp[-1], slot, tm[-1]))
            if V.all():
                for i0 in range(0, G, 2000):
                    masked = ctx.get_codes(i0, i0 + 2000, 0, G)
                    ctx.build_pairs(0)
                    same = np.array_equal(masked, ctx.get_codes(i0, i0 + 2000, 0, G))
                    ctx.build_pairs_masked(0, 0.01)
                    if not same:
                        say("  all-ones mask: the tables DIFFER in rows %d .. %d" % (i0, i0 + 2000))
                        return 1
                say("  all-ones mask: the masked table equals the plain one, all %d rows" % G)
            mp, mm = float(np.median(tp[1:])), float(np.median(tm[1:]))
            say("  %-14s plain median %.3f ms (%.3f .. %.3f)   masked median %.3f ms (%.3f .. %.3f)   ratio %.2f"
                % (name, mp, min(tp[1:]), max(tp[1:]), mm, min(tm[1:]), max(tm[1:]), mm / mp))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "masked_pairs_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/masked_pairs_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
