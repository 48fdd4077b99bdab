"""Registers, scratch and LDS of the per-sample ranking kernels, one line per instantiation, the Float32 ones next to their Float64 /
Int64 twins: compiles csrc/transform.hip for gfx950 with -Rpass-analysis=kernel-resource-usage (no GPU needed).
usage: python tools/transform_resources.py > profiles/f32_kernel_registers.txt"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rankcompv3.jl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
       "-c", "-o", os.devnull, os.path.join(CSRC, "transform.hip"), "-Rpass-analysis=kernel-resource-usage"]
err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
rows = []
for b in re.split(r"remark: [^\n]*Function Name: ", err)[1:]:
    name = subprocess.run(["c++filt", b.split()[0]], capture_output=True, text=True).stdout.strip()
    m = re.search(r"(t_sample_wide|t_sample_big|t_widen_cols|t_widen)<([^>]*)>", name)
    if not m:
        continue
    g = lambda k: int(re.search(re.escape(k) + r": (\d+)", b).group(1))
    args = [a.strip() for a in m.group(2).split(",")]
    rows.append((m.group(1), tuple(args[1:]), args[0], g("VGPRs"), g("AGPRs"), g("SGPRs"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"),
                 g("LDS Size [bytes/block]")))
print("# hipcc " + " ".join(a.replace(ROOT + os.sep, "") for a in cmd[1:]))
print("# (LDS: the static part; the ranking kernels take theirs dynamically, by the number of genes, the same for every element type)")
print("%-16s %-14s %-10s %5s %5s %5s %8s %10s %5s" % ("kernel", "form", "element", "vgpr", "agpr", "sgpr", "scratch", "occupancy", "lds"))
bad = 0
for r in sorted(rows):
    print("%-16s %-14s %-10s %5d %5d %5d %8d %10d %5d" % (r[0], ",".join(r[1]), r[2], *r[3:]))
for r in rows:   # no Float32 instantiation may use scratch that its Float64 twin does not
    if r[2] == "float" and r[0].startswith("t_sample"):
        twin = [q for q in rows if q[:2] == r[:2] and q[2] == "double"]
        if not twin or r[6] > twin[0][6]:
            bad += 1
            print("# FAIL: %s<%s> float uses %d bytes of scratch, its double twin %s" % (r[0], ",".join(r[1]), r[6], twin[0][6] if twin else "is missing"))
print("# float instantiations with more scratch than their double twin: %d" % bad)
sys.exit(1 if bad else 0)
