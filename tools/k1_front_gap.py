"""What lies in front of the K1 stage of a slot build, from a kernel trace: per step the span from the end of t_sample to the start of
k1_slot_part (the first kernel of k1_slots_front), the kernels inside it and how long the device idles there -- the wait for the
transform's flags shows as idle time here if the table's clearing no longer covers it.
   rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python3 bench.py --gpus 1 --steps 8 --warmup 2
   python3 tools/k1_front_gap.py DIR/<host>/<pid>_kernel_trace.csv"""
import csv
import sys

rows = []
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()
gaps, busy, seen = [], [], {}
last_sample = None
for i, (s, e, n) in enumerate(rows):
    if "t_sample" in n:
        last_sample = i
    if "k1_slot_part" in n and last_sample is not None:
        between = rows[last_sample + 1:i]
        gaps.append(s - rows[last_sample][1])
        busy.append(sum(b[1] - b[0] for b in between))
        for b in between:
            key = b[2].split("(")[0][-40:]
            seen.setdefault(key, []).append(b[1] - b[0])
        last_sample = None
n = len(gaps)
if n:
    g, b = sorted(gaps)[n // 2] / 1e3, sorted(busy)[n // 2] / 1e3
    print(f"{n} steps: t_sample end -> k1_slot_part start, median {g:.1f} us, of which kernels ran {b:.1f} us (median), idle {g - b:.1f} us")
    for k, v in seen.items():
        print(f"   {k}: {len(v) / n:.1f} per step, mean {sum(v) / len(v) / 1e3:.1f} us")
