"""A sparse matrix that is ALREADY ON THE GPU, three routes alternating in ONE process with the block cache and the contexts' handles warm:
  host         the scipy matrix through the host CSC entry (reo_set_matrix_pseudobulk_csc_* / reo_set_matrix_csc_*): checked and narrowed by
               the host threads, sent over the link -- the parent commit's only route, and the number to compare against;
  device       the torch sparse_csc tensor through the device entry (reo_set_matrix_pseudobulk_csc_dev_* / reo_set_matrix_csc_dev_*): index
               arrays checked by a kernel, nothing on the link;
  d2h + host   what a caller whose matrix lives in HBM paid before: the three arrays copied to the host, then the host route.
Two shapes: the config-5 cell matrix (20 000 x 50 000 at 6 %, pseudo-bulk into 64 + 64 profiles as the context's matrix) and config 3
(20 000 x 1 000 counts of synth.t1_counts) thinned to 10 % (set_matrix, then build_pairs).  Per call: wall time around the whole call and
the HIP-event time of a pair of events on torch's current stream around it (the library waits for its own stream inside the call, so the
pair brackets its device work; the wall time has the host side as well).  The resident matrices of the three routes must be equal bit
for bit.  Writes profiles/csc_device_ab.txt.  python tools/csc_device_ab.py [repeats]"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0005
T = time.perf_counter


def cells(G, C, dens):
    """tools/config5.py's cells: zero-inflated counts with heavy-tailed gene scales; cells of group 2 shift 10 % of the genes"""
    rng = np.random.default_rng(seed)
    scale = 2.0 ** rng.integers(0, 9, size=G)
    nnz_per_cell = rng.binomial(G, dens, size=C)
    indptr = np.concatenate([[0], np.cumsum(nnz_per_cell)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(G, n, replace=False)) for n in nnz_per_cell]).astype(np.int32)
    eff = np.where(rng.random(G) < 0.1, rng.choice([0.5, 2.0], size=G), 1.0)
    cell_of = np.repeat(np.arange(C), nnz_per_cell)
    vals = 1 + rng.poisson(scale[rows] * np.where(cell_of >= C // 2, eff[rows], 1.0))
    return sp.csc_matrix((vals.astype(np.int64), rows, indptr), shape=(G, C))


def thinned(G, S, dens):
    X = pkg.synth.t1_counts(G, S, seed)
    keep = np.random.default_rng(seed).random((G, S)) < dens
    return sp.csc_matrix(np.where(keep, X, 0))


def on_device(M):
    cp = torch.from_numpy(M.indptr.astype(np.int64)).cuda()
    ri = torch.from_numpy(M.indices.astype(np.int64)).cuda()   # torch's default index width
    va = torch.from_numpy(M.data).cuda()
    return torch.sparse_csc_tensor(cp, ri, va, size=M.shape)


def to_host(t):
    """the device tensor as a scipy matrix: three device-to-host copies (pageable), what the caller of the host route pays first"""
    cp, ri, va = t.ccol_indices().cpu().numpy(), t.row_indices().cpu().numpy(), t.values().cpu().numpy()
    return sp.csc_matrix((va, ri.astype(np.int32), cp), shape=tuple(t.shape))


def timed(fn):
    """(result, wall ms, HIP-event ms) of one call"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = T()
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, (T() - t0) * 1e3, a.elapsed_time(b)


def bench(say, title, M, reps, put, after):
    """put(ctx, matrix): the call under test; after(ctx): what follows it before the resident matrix is compared"""
    t = on_device(M)
    say("%s: %d x %d, %d nnz (%.1f %%), %d index + value MB on the device; %d alternating repeats, the first dropped"
        % (title, M.shape[0], M.shape[1], M.nnz, 100.0 * M.nnz / (M.shape[0] * M.shape[1]), (M.nnz * 16 + 8 * (M.shape[1] + 1)) >> 20, reps))
    legs = {"host": lambda ctx: put(ctx, M), "device": lambda ctx: put(ctx, t), "d2h + host": lambda ctx: put(ctx, to_host(t))}
    times = {k: [] for k in legs}
    for r in range(reps):
        got = {}
        for name, leg in legs.items():
            with pkg.Context(device=0, seed=seed) as ctx:
                _, wall, ev = timed(lambda: leg(ctx))
                after(ctx)
                got[name] = ctx.get_matrix().tobytes(order="F") if r == 0 else None
                info = ctx.info()
            times[name].append((wall, ev))
            say("  repeat %d  %-11s wall %9.2f ms   events %9.2f ms   link %d bytes" % (r, name, wall, ev, info["upload_link_bytes"]))
        if r == 0 and not (got["host"] == got["device"] == got["d2h + host"]):
            say("  resident matrices DIFFER")
            return 1
    for name, v in times.items():
        w, e = np.asarray([x[0] for x in v[1:]]), np.asarray([x[1] for x in v[1:]])
        say("  median %-11s wall %9.2f ms (%.2f .. %.2f)   events %9.2f ms (%.2f .. %.2f)" % (name, np.median(w), w.min(), w.max(), np.median(e), e.min(), e.max()))
    return 0


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, C, n_pseudo = 20000, 50000, 64
    X = cells(G, C, 0.06)
    labels = ["g1"] * (C // 2) + ["g2"] * (C - C // 2)
    order, ptr, _, _ = pkg.cells_partition(labels, n_pseudo, seed)
    rc = bench(say, "config 5 cells -> 64 + 64 resident profiles (set_matrix_pseudobulk)", X, reps,
               lambda ctx, m: ctx.set_matrix_pseudobulk(m, order, ptr), lambda ctx: None)
    if rc:
        return rc
    S = 1000
    M = thinned(G, S, 0.10)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))

    def put(ctx, m):
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01)
        (ctx.set_matrix_tensor if pkg._ffi.is_device_sparse(m) else ctx.set_matrix)(m)
        ctx.build_pairs(0)
    rc = bench(say, "config 3 thinned to 10 % (groups, set_matrix, build_pairs)", M, reps, put, lambda ctx: None)
    if rc:
        return rc
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "csc_device_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/csc_device_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
