"""Sparse host matrices: the drop-in call (run_identify_degs: groups and thresholds first, then the matrix) on the same data two ways.
  sparse         a scipy.sparse csc_matrix through reo_set_matrix_csc_* (densified on the device);
  dense          np.asfortranarray(M.toarray()) through the column-major entry -- the only route a sparse matrix had before --
                 timed WITHOUT the toarray() (the dense array made outside the timed region) and WITH it.
Int64 counts and, in a second pass, float32 counts, at densities of 7 % and 50 %, 20 000 x 4 000 (the dense form is 640 / 320 MB).
One leg per process: a leg never inherits another leg's staging slots, block cache or hardware queues; inside its process a leg runs
its call `repeats` times, one context alive at a time as the drop-in call makes and destroys one, the first repeat dropped.  Every
process prints one JSON line; the sparse and the dense result matrices must be equal bit for bit (a digest is compared).  The densify
kernel's own time comes from one more call with REO_UPLOAD_TIMES=1 (HIP events around every piece's copy and kernel, on the upload
stream) and is set against its write floor, G x S x sizeof(element) bytes.
Writes profiles/csc_ab.txt.  python tools/csc_ab.py [repeats] [cases, e.g. 20000x4000:i64:0.07,20000x4000:f32:0.5]"""
import hashlib
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0004
T = time.perf_counter
DT = {"i64": np.int64, "f32": np.float32, "f64": np.float64, "i32": np.int32}


def matrix(G, S, name, density):
    """counts thinned to `density` by a seeded mask, as a canonical csc_matrix of the element type"""
    rng = np.random.default_rng(seed)
    X = rng.geometric(0.02, size=(G, S))                         # counts with a tail, none of them zero: the mask alone sets the density
    M = sp.csc_matrix(np.where(rng.random((G, S)) < density, X, 0).astype(DT[name]))
    M.sort_indices()
    return M


def leg_child(G, S, name, density, leg, reps):
    M = matrix(G, S, name, density)
    group = pkg.synth.groups(S)
    names = [f"g{i}" for i in range(G)]
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    dense = np.asfortranarray(M.toarray()) if leg == "dense" else None
    walls, sets, conv = [], [], []
    run = None
    for _ in range(reps):
        t0 = T()
        if leg == "sparse":
            data = M
        elif leg == "dense":
            data = dense
        else:   # dense_with_toarray: what the caller of the parent commit pays
            data = np.asfortranarray(M.toarray())
        t1 = T()
        run = pkg.run_identify_degs(data, group, names, 0.01, 1.0, 0.05, ref0, 128, 0, seed=seed, device=0)
        walls.append((T() - t0) * 1e3); conv.append((t1 - t0) * 1e3)
        assert run.info["csc_upload"] == (1 if leg == "sparse" else 0)
    for _ in range(3):   # the host wall of reo_set_matrix_* itself: the library's own clock, read with profiling on (not part of the walls above)
        sets.append(pkg.run_identify_degs(M if leg == "sparse" else np.asfortranarray(M.toarray()) if dense is None else dense, group, names, 0.01, 1.0, 0.05,
                                          ref0, 2, 0, seed=seed, device=0, profile=True).timings["set_matrix_host_wall_ms"])
    out = dict(leg=leg, wall_ms=walls, toarray_ms=conv, set_matrix_host_wall_ms=sets, link_bytes=run.info["upload_link_bytes"], nnz=int(M.nnz),
               digest=hashlib.sha256(np.ascontiguousarray(run.result).tobytes()).hexdigest()[:16], passes=run.iters_run)
    if leg == "sparse":   # one more call with the per-piece HIP events (stderr of this process)
        os.environ["REO_UPLOAD_TIMES"] = "1"
        sys.stderr.write("csc_ab pieces begin\n"); sys.stderr.flush()
        pkg.run_identify_degs(M, group, names, 0.01, 1.0, 0.05, ref0, 2, 0, seed=seed, device=0)
    print("CSC_AB " + json.dumps(out), flush=True)


def stats(v):
    v = np.asarray(v[1:], dtype=np.float64)   # the first repeat warms up
    return float(np.median(v)), float(v.min()), float(v.max())


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        G, S = (int(v) for v in sys.argv[2].split("x"))
        return leg_child(G, S, sys.argv[3], float(sys.argv[4]), sys.argv[5], int(sys.argv[6]))
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    cases = (sys.argv[2] if len(sys.argv) > 2 else "20000x4000:i64:0.07,20000x4000:i64:0.5,20000x4000:f32:0.07,20000x4000:f32:0.5").split(",")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("csc_ab: run_identify_degs (groups first) from a host matrix, ms, median (min .. max) of %d repeats after one warm-up, one leg per process" % (reps - 1))
    for case in cases:
        shape, name, density = case.split(":")
        G, S = (int(v) for v in shape.split("x"))
        got = {}
        for leg in ("sparse", "dense", "dense_with_toarray"):
            env = dict(os.environ, REO_CYCLE="0")
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", shape, name, density, leg, str(reps)], env=env, capture_output=True, text=True)
            rec = [l for l in out.stdout.splitlines() if l.startswith("CSC_AB ")]
            if out.returncode != 0 or not rec:
                say("%s %s: the child failed (%d): %s" % (case, leg, out.returncode, out.stderr[-400:]))
                return 1   # nothing more is started on the GPU after a failed leg
            got[leg] = json.loads(rec[0][7:])
            if leg == "sparse":
                pieces = out.stderr.split("csc_ab pieces begin")[-1]
                got[leg]["densify_us"] = [float(v) for v in re.findall(r"densify ([0-9.]+) us", pieces)]
                got[leg]["copy_us"] = [float(v) for v in re.findall(r"copy ([0-9.]+) us", pieces)]
        for leg, r in got.items():
            m, lo, hi = stats(r["wall_ms"])
            say("%-22s %-19s call %8.2f (%8.2f .. %8.2f)   of it toarray %8.2f   set_matrix_host_wall %8.2f   link %12d bytes   nnz %d   passes %d"
                % (case, leg, m, lo, hi, stats(r["toarray_ms"])[0], float(np.median(r["set_matrix_host_wall_ms"])), r["link_bytes"], r["nnz"], r["passes"]))
        same = len({r["digest"] for r in got.values()}) == 1
        s, d, dt = (stats(got[k]["wall_ms"]) for k in ("sparse", "dense", "dense_with_toarray"))
        say("%-22s results %s; sparse - dense = %+.2f ms, sparse - dense_with_toarray = %+.2f ms (spreads %.2f / %.2f / %.2f); link sparse / dense = %.3f"
            % (case, "EQUAL" if same else "DIFFER", s[0] - d[0], s[0] - dt[0], s[2] - s[1], d[2] - d[1], dt[2] - dt[1],
               got["sparse"]["link_bytes"] / got["dense"]["link_bytes"]))
        k = got["sparse"]["densify_us"]
        if k:
            wbytes = G * S * (4 if name == "f32" else 8)
            say("%-22s densify kernel (t_csc_columns): %d launches, %.1f us in all for %.1f MB written = %.2f TB/s (the floor: that write alone); copies %.1f us"
                % (case, len(k), sum(k), wbytes * 1e-6, wbytes / (sum(k) * 1e-6) * 1e-12, sum(got["sparse"]["copy_us"])))
        else:
            say("%-22s densify kernel: no per-piece times came back" % case)
        if not same:
            return 1
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "csc_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/csc_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
