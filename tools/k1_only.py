"""Runs only transform + K1 (3 x build_pairs) on the bench workload, or on G x S of it (python tools/k1_only.py t0 60000 64: a shape
whose column un-permute takes the narrow word form); a target for rocprofv3 --kernel-trace or --pmc."""
import sys, numpy as np
sys.path.insert(0, '.')
import __graft_entry__ as ge
pkg = ge.load_pkg()
seed = 0x5EED0003
fam = sys.argv[1] if len(sys.argv) > 1 else "t0"
G, S = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (20000, 1000)
X = pkg.synth.t0_ranks(G, S, seed) if fam == "t0" else pkg.synth.t1_counts(G, S, seed)
gid, _ = pkg.encode_groups(np.asarray(pkg.synth.groups(S)))
with pkg.Context(device=0, seed=seed) as ctx:
    ctx.set_matrix(X); ctx.set_groups(gid, 2); ctx.compute_thresholds(0.01)
    for rep in range(3):
        ctx.build_pairs(0)
    print("done", G, S, "k1_slot_order", ctx.info()["k1_slot_order"], "k1_unslot_form", ctx.info().get("k1_unslot_form"))
