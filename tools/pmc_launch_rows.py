#!/usr/bin/env python3
"""Per-launch HBM traffic of the Winograd kernels from a FETCH_SIZE and a WRITE_SIZE pass: consecutive dispatches of one
(kernel, grid) are one row of bench.py's roofline loop (layer order conv2.0, conv2.3, conv3.0, conv3.3, conv4.0; fwd, dgrad, wgrad).
    python tools/pmc_launch_rows.py FETCH_DIR WRITE_DIR        (the two rocprofv3 -d directories; FETCH_SIZE counts x 2 as in pmc_traffic.py)"""
import csv, glob, os, re, sys, collections
def collect(d, counter):
    disp = collections.OrderedDict()
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != counter: continue
            m = re.search(r"(conv3d_wino_wgrad_p_kernel<\d>|conv3d_wino_p_kernel<\d, \d>|conv3d_winox_kernel<\d>)", r["Kernel_Name"])
            if not m: continue
            k = int(r["Dispatch_Id"])
            e = disp.setdefault(k, [m.group(1), int(r["Grid_Size"]) // max(int(r["Workgroup_Size"]), 1), 0.0])
            e[2] += float(r["Counter_Value"])
    runs = []
    for k in sorted(disp):
        n, g, v = disp[k]
        if runs and runs[-1][0] == n and runs[-1][1] == g: runs[-1][2].append(v)
        else: runs.append([n, g, [v]])
    return runs
fe, wr = collect(sys.argv[1], "FETCH_SIZE"), collect(sys.argv[2], "WRITE_SIZE")
print(f"{'kernel':32s} {'workgroups':>10s} {'launches':>8s} {'fetch x2 MB':>12s} {'write MB':>10s} {'total MB':>10s}")
for i, (n, g, v) in enumerate(fe):
    f = sum(v) / len(v) * 1024 * 2 / 1e6
    w = wr[i] if i < len(wr) and wr[i][0] == n and wr[i][1] == g else None
    wm = sum(w[2]) / len(w[2]) * 1024 / 1e6 if w else float("nan")
    print(f"{n:32s} {g:10d} {len(v):8d} {f:12.1f} {wm:10.1f} {f + wm:10.1f}")
