"""Cells to DEGs at BASELINE config 5 (20 000 genes x 50 000 sparse cells -> 64 + 64 pseudo-bulk profiles -> identify_degs), two ways,
alternating in ONE process with the block cache and the contexts' handles warm:
  host      today's three steps: Context.pseudobulk (the profiles come to the host), numpy filters (src/RankCompV3.jl:618, :626, at 0)
            and a contiguous copy, run_identify_degs (the copy goes up again);
  resident  identify_degs_cells: the sums written into the context's matrix, filtered on the device, no host trip for the profiles.
The expected difference is one 20 MB download, the host filter copy and one 20 MB upload.  The result matrices must be equal bit for bit.
Writes the per-call times to profiles/cells_resident_ab.txt.  python tools/cells_ab.py [repeats]"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
G, C, seed, dens, n_pseudo = 20000, 50000, 0x5EED0005, 0.06, 64
T = time.perf_counter


def cells():
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


def host_route(X, labels, names):
    t0 = T()
    order, ptr, pnames, pgroups = pkg.cells_partition(labels, n_pseudo, seed)
    with pkg.Context(device=0, seed=seed) as ctx:
        pb = ctx.pseudobulk(X, order, ptr)
    t1 = T()
    pk = (pb > 0).sum(axis=0) > 0
    kept = pb[:, pk]
    gk = (kept > 0).sum(axis=1) > 0
    pbk = np.ascontiguousarray(kept[gk])
    Gk = pbk.shape[0]
    t2 = T()
    run = pkg.run_identify_degs(pbk, [g for g, k in zip(pgroups, pk) if k], [n for n, k in zip(names, gk) if k], 0.01, 1.0, 0.05,
                                pkg.synth.ref_mask(Gk, min(Gk, 3000), seed), 128, 5, seed=seed, device=0)
    t3 = T()
    return run, [(t3 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3]


def resident_route(X, labels, names):
    t0 = T()
    got = pkg.identify_degs_cells(X, labels, names, n_pseudo, 0.01, 1.0, 0.05, None, 128, 5, seed=seed, device=0)
    return got.run, [(T() - t0) * 1e3]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    t0 = T()
    X = cells()
    labels = ["g1"] * (C // 2) + ["g2"] * (C - C // 2)
    names = [f"g{i}" for i in range(G)]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("cells_ab: config 5, %d x %d cells, %d nnz (%.1f %%), n_pseudo %d per group; ms per call, %d alternating repeats in one process, the first dropped"
        % (G, C, X.nnz, 100.0 * X.nnz / (G * C), n_pseudo, reps))
    print("generated in %.1f s" % (T() - t0), flush=True)
    host, res = [], []
    for r in range(reps):
        run_h, th = host_route(X, labels, names)
        run_r, tr = resident_route(X, labels, names)
        same = (run_h.result.tobytes(order="F") == run_r.result.tobytes(order="F") and run_h.iters_run == run_r.iters_run and run_h.trace == run_r.trace
                and list(run_h.gene_names) == list(run_r.gene_names))
        say("repeat %d: host %8.2f (pseudobulk %7.2f, numpy filters + copy %6.2f, run_identify_degs %7.2f)   resident %8.2f   results %s, %d x %d, passes %d"
            % (r, th[0], th[1], th[2], th[3], tr[0], "EQUAL" if same else "DIFFER", run_r.info["G"], run_r.info["S"], run_r.iters_run))
        if not same:
            return 1
        host.append(th[0]); res.append(tr[0])
    h, q = np.asarray(host[1:]), np.asarray(res[1:])
    say("median host %.2f ms (%.2f .. %.2f), resident %.2f ms (%.2f .. %.2f): resident - host = %+.2f ms"
        % (np.median(h), h.min(), h.max(), np.median(q), q.min(), q.max(), np.median(q) - np.median(h)))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "cells_resident_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/cells_resident_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
