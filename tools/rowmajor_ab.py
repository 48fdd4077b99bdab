"""Row-major host matrices: the whole drop-in call (a pageable numpy matrix in, the result on the host out) three ways, in one
process, legs alternating, first repeat dropped, a context per call as the drop-in call makes one.
  (a) a C-ordered array with REO_ROWMAJOR=0: np.asfortranarray on the host, then the column-major entry -- what the parent commit does;
  (b) the same C-ordered array through reo_set_matrix_rm_* (REO_ROWMAJOR=1: read in place, transposed on the device);
  (c) the np.asfortranarray copy made OUTSIDE the timed region, through the column-major entry: the floor.
Config 3 (20 000 x 1 000) in Int64 and Float64, config 4 (30 000 x 4 000) in Int64 and Float32.  Leg (b) also runs with
REO_ROWMAJOR_COPY=2d (one 2-D copy per chunk from the pageable array instead of host threads packing the rows into pinned memory).
Then, in a child process per shape with REO_UPLOAD_TIMES=1, the HIP-event times of every chunk's copy and transposition.
Results must not differ between the legs: the result matrix of every call is compared with leg (c)'s.
Writes profiles/rowmajor_ab.txt.  python tools/rowmajor_ab.py [repeats] [cases, e.g. 20000x1000:i64,30000x4000:f32]"""
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
DT = {"i64": np.int64, "f64": np.float64, "f32": np.float32, "i32": np.int32}


def matrix(G, S, name):
    X = pkg.synth.t1_counts(G, S, seed) if name in ("i64", "i32") else pkg.synth.float_expr(G, S, seed)
    return np.ascontiguousarray(X.astype(DT[name]))


def call(X, gid, ref0, passes=128):
    """the drop-in call's library part: groups and thresholds first, the matrix, the table, the passes; ends with the result on the host"""
    t0 = T()
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
        t1 = T(); ctx.set_matrix(X); t2 = T()
        ctx.build_pairs(0)
        res, it, tr = ctx.identify_degs(ref0, 1.0, 0.05, passes, 0)   # (ends in a synchronise)
        info = ctx.info()
    return (T() - t0) * 1e3, (t2 - t1) * 1e3, res, info


def stats(v):
    v = np.asarray(v[1:], dtype=np.float64)   # the first repeat warms up
    return float(np.median(v)), float(v.min()), float(v.max())


def chunks_child(G, S, name):
    X = matrix(G, S, name)
    gid, _ = pkg.encode_groups(np.asarray(pkg.synth.groups(S)))
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    os.environ["REO_ROWMAJOR"] = "1"
    call(X, gid, ref0, 2)                       # warm
    os.environ["REO_UPLOAD_TIMES"] = "1"
    sys.stderr.write("chunks %d x %d %s\n" % (G, S, name)); sys.stderr.flush()
    call(X, gid, ref0, 2)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--chunks":
        G, S = (int(v) for v in sys.argv[2].split("x"))
        return chunks_child(G, S, sys.argv[3])
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    cases = (sys.argv[2] if len(sys.argv) > 2 else "20000x1000:i64,20000x1000:f64,30000x4000:i64,30000x4000:f32").split(",")
    os.environ["REO_CYCLE"] = "0"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("rowmajor_ab: whole drop-in call from a pageable host matrix, ms, median (min .. max) of %d repeats after one warm-up" % (reps - 1))
    for case in cases:
        shape, name = case.split(":")
        G, S = (int(v) for v in shape.split("x"))
        X = matrix(G, S, name)
        assert X.flags.c_contiguous
        XF = np.asfortranarray(X)
        gid, _ = pkg.encode_groups(np.asarray(pkg.synth.groups(S)))
        ref0 = pkg.synth.ref_mask(G, 3000, seed)
        legs = {"a_host_transpose": (X, {"REO_ROWMAJOR": "0"}), "b_rowmajor_pack": (X, {"REO_ROWMAJOR": "1", "REO_ROWMAJOR_COPY": "pack"}),
                "b_rowmajor_2d": (X, {"REO_ROWMAJOR": "1", "REO_ROWMAJOR_COPY": "2d"}), "c_colmajor_floor": (XF, {})}
        rows = {k: [] for k in legs}
        sm = {k: [] for k in legs}
        link, want = {}, None
        for rep in range(reps):
            for leg, (M, env) in legs.items():
                for k in ("REO_ROWMAJOR", "REO_ROWMAJOR_COPY"):
                    os.environ.pop(k, None)
                os.environ.update(env)
                ms, set_ms, res, info = call(M, gid, ref0)
                assert info["rowmajor_upload"] == (1 if leg.startswith("b_") else 0), (leg, info["rowmajor_upload"])
                if want is None and leg == "c_colmajor_floor":
                    want = res
                rows[leg].append(ms); sm[leg].append(set_ms); link[leg] = info["upload_link_bytes"]
                if want is not None:
                    assert np.array_equal(res, want, equal_nan=True), (case, leg, "results differ")
        for k in ("REO_ROWMAJOR", "REO_ROWMAJOR_COPY"):
            os.environ.pop(k, None)
        st = {leg: stats(rows[leg]) for leg in legs}
        for leg in legs:
            m, lo, hi = st[leg]
            say("%-14s %-17s call %8.2f (%8.2f .. %8.2f)   set_matrix %8.2f   link %d bytes" % (case, leg, m, lo, hi, stats(sm[leg])[0], link[leg]))
        a, b = st["a_host_transpose"], st[min(("b_rowmajor_pack", "b_rowmajor_2d"), key=lambda k: st[k][0])]
        bd = st["b_rowmajor_pack"]
        spread = (a[2] - a[1]) + (bd[2] - bd[1])
        say("%-14s (b, default) against (a): %.2f ms faster, spread of the two legs %.2f ms -> %s; (b) - (c) = %.2f ms; best (b) %.2f"
            % (case, a[0] - bd[0], spread, "FASTER" if a[0] - bd[0] > spread else "NOT faster by more than the spread", bd[0] - st["c_colmajor_floor"][0], b[0]))
        del X, XF
    say("")
    say("per chunk, HIP events on the upload stream (a child process per case, REO_UPLOAD_TIMES=1):")
    for case in cases:
        shape, name = case.split(":")
        env = dict(os.environ, REO_CYCLE="0")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--chunks", shape, name], env=env, capture_output=True, text=True)
        keep = [l for l in out.stderr.splitlines() if l.startswith("chunks ") or "upload chunk" in l]
        if out.returncode != 0 or not keep:
            say("%s: the child failed (%d): %s" % (case, out.returncode, out.stderr[-400:]))
        for l in keep:
            say(l)
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "rowmajor_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/rowmajor_ab.txt")


if __name__ == "__main__":
    main()
