"""Float32 entry points against the Float64 path on the widened values, in one process, legs alternating, first repeat dropped.
  resident: a matrix already in HBM at the config-3 shape (20 000 x 1 000, synth.float_expr rounded to float32) -- transform time
            (stage timer 0, HIP events) and whole-step wall time of reo_set_matrix_dev_f32 against reo_set_matrix_dev_f64.  The
            margin is the spread between the repeats of the Float64 leg.
  drop-in:  a float32 numpy matrix in pageable host memory, config-3 and config-4 shapes -- the Float32 call against
            np.asfortranarray(X, dtype=np.float64) followed by the Float64 call (what a float32 matrix cost before), both parts timed,
            and the bytes on the link.
Prints a summary and writes profiles/f32_ab.json.  python tools/f32_ab.py [repeats] [shapes, e.g. 20000x1000,30000x4000]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
import torch

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
SHAPES = [tuple(int(v) for v in s.split("x")) for s in (sys.argv[2] if len(sys.argv) > 2 else "20000x1000,30000x4000").split(",")]
seed = 0x5EED0003
os.environ["REO_CYCLE"] = "0"
T = time.perf_counter
out = {"repeats_kept": REPS - 1}


def stats(v):
    v = np.asarray(v[1:], dtype=np.float64)   # the first repeat warms up
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max()), "spread": float(v.max() - v.min())}


def step(ctx, load, gid, ref0, passes=128):
    ctx.reset_timings(); torch.cuda.synchronize()
    t0 = T()
    ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
    t1 = T(); load(ctx); t2 = T()
    ctx.build_pairs(0)
    res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, passes, 0)   # (ends in a synchronise: the result is in host memory)
    t3 = T()
    tm = ctx.timings()
    return {"step_ms": (t3 - t0) * 1e3, "set_matrix_ms": (t2 - t1) * 1e3, "transform_ms": tm["transform_ms"], "k1_ms": tm["k1_ms"]}, res


# ---- resident matrix, config 3
G, S = 20000, 1000
X32 = np.asfortranarray(pkg.synth.float_expr(G, S, seed).astype(np.float32))
gid, _ = pkg.encode_groups(np.asarray(pkg.synth.groups(S)))
ref0 = pkg.synth.ref_mask(G, 3000, seed)
d32 = torch.from_numpy(np.ascontiguousarray(X32.T)).cuda()
d64 = d32.to(torch.float64)
torch.cuda.synchronize()
legs = {"f64": (d64, "f64"), "f32": (d32, "f32")}
ctxs = {k: pkg.Context(device=0, seed=seed) for k in legs}
for c in ctxs.values():
    c.set_profiling(True)
rows = {k: [] for k in legs}
for rep in range(REPS):
    for k, (t, name) in legs.items():
        r, _ = step(ctxs[k], lambda c, t=t, name=name: c.set_matrix_device(t.data_ptr(), G, S, G, name), gid, ref0)
        rows[k].append(r)
for c in ctxs.values():
    c.close()
res = {k: {f: stats([r[f] for r in rows[k]]) for f in ("transform_ms", "k1_ms", "step_ms")} for k in legs}
out["resident_20000x1000"] = res
for f in ("transform_ms", "step_ms"):
    a, b = res["f64"][f], res["f32"][f]
    verdict = "not slower" if b["median"] <= a["median"] + a["spread"] else "SLOWER by more than the Float64 leg's spread"
    print("resident 20000 x 1000 %-12s  f64 %.3f (spread %.3f)  f32 %.3f (spread %.3f)  -> f32 %s" % (f, a["median"], a["spread"], b["median"], b["spread"], verdict), flush=True)
del d32, d64

# ---- drop-in call from pageable host memory
for (G, S) in SHAPES:
    X32 = np.asfortranarray(pkg.synth.float_expr(G, S, seed).astype(np.float32))
    gid, _ = pkg.encode_groups(np.asarray(pkg.synth.groups(S)))
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    rows = {"f32": [], "widen_then_f64": []}
    link = {}
    for rep in range(REPS):
        for leg in rows:
            with pkg.Context(device=0, seed=seed) as ctx:   # a context per call, as the drop-in call makes one
                ctx.set_profiling(True)
                conv = 0.0
                M = X32
                if leg == "widen_then_f64":
                    t0 = T(); M = np.asfortranarray(X32, dtype=np.float64); conv = (T() - t0) * 1e3
                r, _ = step(ctx, lambda c, M=M: c.set_matrix(M), gid, ref0)
                r["host_convert_ms"] = conv
                r["call_ms"] = conv + r["step_ms"]
                link[leg] = ctx.info()["upload_link_bytes"]
                rows[leg].append(r)
                del M
    res = {leg: {f: stats([r[f] for r in rows[leg]]) for f in ("host_convert_ms", "set_matrix_ms", "step_ms", "call_ms", "transform_ms")} for leg in rows}
    for leg in rows:
        res[leg]["upload_link_bytes"] = int(link[leg])
    out["drop_in_%dx%d" % (G, S)] = res
    for leg in rows:
        q = res[leg]
        print("drop-in %d x %d %-15s host convert %.2f + library %.2f (set_matrix %.2f) = %.2f ms; %d bytes on the link (4 G S = %d)"
              % (G, S, leg, q["host_convert_ms"]["median"], q["step_ms"]["median"], q["set_matrix_ms"]["median"], q["call_ms"]["median"],
                 q["upload_link_bytes"], 4 * G * S), flush=True)

os.makedirs("profiles", exist_ok=True)
with open(os.path.join("profiles", "f32_ab.json"), "w") as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote profiles/f32_ab.json")
