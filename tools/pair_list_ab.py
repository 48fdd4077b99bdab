"""The reversed-pair lists (n13, n31) of every DEG at BASELINE config 3 (synthetic 20 000 genes x 1 000 samples, T0 family, the workload of
bench.py), after a real identify_degs (n_iter = 128, n_conv = 5), built two ways that alternate in ONE process on one context:
  pair_list   reo_pair_list with the NULL mask: count pass, prefix sums on the host, fill pass, the CSR copied back;
  get_codes   the only route there was before: reo_get_codes over the DEG rows in blocks (one byte per ordered pair to the host), then
              numpy -- the code bytes against the class mask and the reference set, nonzero.
The two CSRs must be equal.  Per route: wall time of every repeat (the first dropped) and the median.  For the count pass alone (count only:
partner = NULL) the bytes it must read -- n_genes * 4 planes * Wp words * 4 bytes, plus the mask as bits -- and the rate those bytes give
against the HBM peak (8.0 TB/s specified, 6.29 TB/s measured with a float4 copy).  Writes profiles/pair_list_ab.txt.
python tools/pair_list_ab.py [repeats] [rows per get_codes block]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import __graft_entry__ as ge

pkg = ge.load_pkg()
seed = 0x5EED0003
T = time.perf_counter
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def by_get_codes(ctx, degs, ref, mask, block):
    """(rowptr, partner, code) through reo_get_codes: DEG rows in runs of consecutive genes, at most `block` rows per call"""
    G = ref.size
    lut = np.zeros(256, dtype=bool)
    lut[:9] = [(mask >> c) & 1 for c in range(9)]
    rowptr, partner, code = [0], [], []
    k = 0
    while k < degs.size:
        e = k
        while e + 1 < degs.size and degs[e + 1] == degs[e] + 1 and e + 1 - k < block:
            e += 1
        i0, i1 = int(degs[k]), int(degs[e]) + 1
        c = ctx.get_codes(i0, i1, 0, G)
        sel = lut[c] & ref[None, :]
        for r in range(i1 - i0):
            j = np.flatnonzero(sel[r])
            partner.append(j.astype(np.int32)); code.append(c[r, j])
            rowptr.append(rowptr[-1] + j.size)
        k = e + 1
    return np.asarray(rowptr, dtype=np.int64), np.concatenate(partner), np.concatenate(code)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    block = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    G, S = 20000, 1000
    X = pkg.synth.t0_ranks(G, S, seed)
    gid, lev = pkg.encode_groups(pkg.synth.groups(S))
    ref0 = pkg.synth.ref_mask(G, 3000, seed)
    mask = pkg._ffi.class_mask("reversed")
    with pkg.Context(device=0, seed=seed) as ctx:
        ctx.set_groups(gid, len(lev)); ctx.compute_thresholds(0.01); ctx.set_matrix(X); ctx.build_pairs(0)
        result, iters, trace = ctx.identify_degs(ref0, 1.0, 0.05, 128, 5)
        labels = pkg.label_genes(result, 1.0, 0.05)
        degs = np.flatnonzero(labels != "no change").astype(np.int32)
        ref = ctx.ref_mask()
        Wp = ctx.info()["Gp"] // 32
        say("config 3: %d x %d, %d passes, %d DEGs, %d reference genes in the last pass; classes n13 | n31; %d repeats, the first dropped, "
            "get_codes in blocks of at most %d rows" % (G, S, iters, degs.size, int(ref.sum()), reps, block))
        if degs.size == 0:
            say("no DEGs: nothing to list")
            return 1
        t = {"pair_list": [], "get_codes": [], "count only": []}
        for r in range(reps):
            t0 = T(); pl = ctx.pair_list(degs, mask); t["pair_list"].append((T() - t0) * 1e3)
            t0 = T(); old = by_get_codes(ctx, degs, ref, mask, block); t["get_codes"].append((T() - t0) * 1e3)
            rowptr = np.zeros(degs.size + 1, dtype=np.int64)
            t0 = T(); ctx.pair_list_raw(degs, mask, None, rowptr, None, None, 0); t["count only"].append((T() - t0) * 1e3)
            if not (np.array_equal(pl.rowptr, old[0]) and np.array_equal(pl.partner, old[1]) and np.array_equal(pl.code, old[2])
                    and np.array_equal(rowptr, old[0])):
                say("  repeat %d: the two routes DIFFER" % r)
                return 1
            say("  repeat %d  pair_list %9.3f ms   get_codes + numpy %9.3f ms   count only %9.3f ms" % (r, t["pair_list"][-1], t["get_codes"][-1], t["count only"][-1]))
        assert np.array_equal(np.diff(pl.rowptr), (result[degs, 4] + result[degs, 8]).astype(np.int64))
        say("  %d pairs listed (%.1f per DEG); get_codes moved %d bytes to the host per repeat, pair_list %d"
            % (pl.partner.size, pl.partner.size / degs.size, degs.size * G, pl.partner.size * 5 + 4 * degs.size))
        med = {k: float(np.median(v[1:] if len(v) > 1 else v)) for k, v in t.items()}
        for k in ("pair_list", "get_codes", "count only"):
            v = t[k][1:] if len(t[k]) > 1 else t[k]
            say("  median %-10s %9.3f ms (%.3f .. %.3f)" % (k, med[k], min(v), max(v)))
        nbytes = degs.size * 4 * Wp * 4 + Wp * 4
        rate = nbytes / (med["count only"] * 1e-3)
        say("  count pass: %d rows x 4 planes x %d words x 4 bytes + the mask = %d bytes; over the WHOLE count-only call (upload of the gene list, "
            "kernel, counts back, waits) that is %.3f GB/s = %.2f %% of the 8.0 TB/s HBM peak (%.2f %% of the 6.29 TB/s a float4 copy reaches)"
            % (degs.size, Wp, nbytes, rate / 1e9, 100.0 * rate / HBM_SPEC, 100.0 * rate / HBM_COPY))
    os.makedirs("profiles", exist_ok=True)
    with open(os.path.join("profiles", "pair_list_ab.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote profiles/pair_list_ab.txt")
    return 0


if __name__ == "__main__":
    sys.exit(main())
