#!/usr/bin/env python3
"""Per-launch times of the persistent Winograd kernels and the slab reductions from two rocprofv3 kernel traces of
`TMF_STREAMS=1 python bench.py --steps 40 --warmup 5` (75 steps with the set-up steps), side by side:
    python tools/kernel_trace_per_launch.py PARENT_kernel_trace.csv NEW_kernel_trace.csv
A row is one launch position (slot) of a kernel within a step: its grid in workgroups and the mean us over the last 40 steps."""
import csv, collections, re, sys
def load(f):
    per = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"]
        m = re.search(r"(conv3d_wino_wgrad_p_kernel<\d>|conv3d_wino_p_kernel<\d, \d>|conv3d_winox_kernel<\d>|slab_reduce\w*|reduce_slabs\w*)", n)
        if not m: continue
        per[m.group(1)].append((int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), int(r["Grid_Size_Y"]) // int(r["Workgroup_Size_Y"]),
                                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    return per
steps = 75
a, b = load(sys.argv[1]), load(sys.argv[2])
print(f"{'kernel':34s} {'slot':>4s} {'grid':>9s} {'parent us':>10s} {'new us':>10s} {'new/parent':>10s}")
tot = [0.0, 0.0]
for k in sorted(a):
    n = len(a[k]) // steps
    for s in range(n):
        pa = [a[k][i] for i in range(s, len(a[k]), n)][-40:]
        pb = [b[k][i] for i in range(s, len(b[k]), n)][-40:]
        ma, mb = sum(x[2] for x in pa) / len(pa), sum(x[2] for x in pb) / len(pb)
        tot[0] += ma; tot[1] += mb
        print(f"{k:34s} {s:4d} {pa[0][0]:5d}x{pa[0][1]:<3d} {ma:10.1f} {mb:10.1f} {mb / ma:10.3f}")
print(f"{'sum per step':34s} {'':4s} {'':9s} {tot[0]:10.1f} {tot[1]:10.1f} {tot[1] / tot[0]:10.3f}")
