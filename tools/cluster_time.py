#!/usr/bin/env python3
"""Connected clusters and the cluster table on one device: transmf_ad_amd.clusters (tmf_cluster_label + tmf_cluster_table) beside
clusters_torch on the device (shifted minima, pointer jumping, scatter ops - with one host read per round) and, where scipy
imports, beside the loop it replaces: a device-to-host copy and scipy.ndimage.label per sample.  B = 8 maps of 96^3: seven smooth
random fields (a box filter run three times over white noise, so the clusters are blobs) and one map of white noise; top = 0.01
and 0.05 at connectivity 6 and 26.  Each call between two device events after a warm-up (the scipy loop: wall clock), the median
of the timed calls.  clusters() is timed with max_clusters given (no host read) and without (one host read of n.max()); the two
entries are timed on their own as well.
    python tools/cluster_time.py [--size 96] [--batch 8] [--calls 20] [--out FILE]
    python tools/cluster_time.py --sequence empty|noise|blobs      one tmf_cluster_label + tmf_cluster_table call, for a kernel trace"""
import argparse
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transmf_ad_amd as T  # noqa: E402
from transmf_ad_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--out")
ap.add_argument("--sequence", choices=("empty", "noise", "blobs"))
args = ap.parse_args()
if args.calls < 10:
    ap.error("--calls must be at least 10")
DEV = "cuda:0"
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, calls, warm=2):
    """[us] of `calls` single calls, each between two device events, after `warm` warm-up calls."""
    for _ in range(warm):
        fn()
    res = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b) * 1e3)
    return res


def fields(B, N):
    """B - 1 smooth fields and one map of white noise, each scaled to unit variance."""
    x = torch.randn((B, 1, N, N, N), device=DEV)
    s = x[:-1] if B > 1 else x
    for _ in range(3):
        s = torch.nn.functional.avg_pool3d(s, 7, stride=1, padding=3, count_include_pad=False)
    maps = torch.cat([s, x[-1:]]) if B > 1 else s
    return (maps / maps.flatten(1).std(1).view(-1, 1, 1, 1, 1))[:, 0].contiguous()


torch.manual_seed(0)
N, B = args.size, args.batch
V = N ** 3
a = fields(B, N)

if args.sequence:
    x = {"empty": torch.full_like(a, -1.0), "noise": torch.randn_like(a), "blobs": a}[args.sequence]
    thr = torch.zeros((B,), device=DEV)
    labels, n = ops.cluster_label(x, thr, "pos", 26, 1)
    ops.cluster_table(x, labels, "pos", 64)
    torch.cuda.synchronize()
    print(f"{args.sequence}: n = {n.tolist()}")
    sys.exit(0)

try:
    from scipy import ndimage
except ImportError:
    ndimage = None

say(f"clusters on B = {B} maps of {N}^3 float32 ({B - 1} smooth fields, 1 white noise), us per call: median (min .. max) of "
    f"{args.calls} calls after 2 warm-up calls")
lost = []
for top in (0.01, 0.05):
    for conn in (6, 26):
        cl = T.clusters(a, top=top, connectivity=conn)
        ct = T.clusters_torch(a, top=top, connectivity=conn)
        equal = all(torch.equal(getattr(cl, f), getattr(ct, f)) for f in ("labels", "n", "size", "argmax", "coord_sum", "bbox")) \
            and torch.equal(cl.peak.view(torch.int32), ct.peak.view(torch.int32))
        nn = cl.n.tolist()
        say(f"top = {top}, connectivity = {conn}: clusters per map {nn}; kernels and torch ops give identical results: {equal}")
        K = max(nn)
        thr = ops.rank_thresholds(a.view(B, V), [min(V, max(1, math.ceil(top * V)))])[0][:, 0].contiguous()
        labels = cl.labels
        struct = None if ndimage is None else ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[conn])

        def scipy_loop():
            host = a.cpu().numpy()
            t = thr.cpu().numpy()
            return [ndimage.label(host[b] >= t[b], struct) for b in range(B)]

        res = {}
        rows = [("clusters(top, max_clusters=K): rank_thresholds + label + table, no host read", lambda: T.clusters(a, top=top, connectivity=conn, max_clusters=K)),
                ("clusters(top): the same + one host read of n.max()                          ", lambda: T.clusters(a, top=top, connectivity=conn)),
                ("  tmf_cluster_label alone (8 stream operations)                             ", lambda: ops.cluster_label(a, thr, "pos", conn, 1)),
                ("  tmf_cluster_table alone (3 launches)                                      ", lambda: ops.cluster_table(a, labels, "pos", K)),
                ("clusters_torch on the device (stock ops, one host read per round)           ", lambda: T.clusters_torch(a, top=top, connectivity=conn))]
        for name, fn in rows:
            us = timed(fn, args.calls)
            res[name] = statistics.median(us)
            say(f"  {name}: {res[name]:10.1f} ({min(us):.1f} .. {max(us):.1f}) us")
        k, t = res[rows[1][0]], res[rows[4][0]]
        say(f"  clusters / clusters_torch = {k / t:.3f}")
        if k > t:
            lost.append((top, conn))
        if ndimage is not None:
            wall = []
            for _ in range(5):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                scipy_loop()
                wall.append((time.perf_counter() - t0) * 1e6)
            say(f"  device-to-host copy + scipy.ndimage.label per sample (labels only, wall clock, 5 calls)  : "
                f"{statistics.median(wall):10.1f} ({min(wall):.1f} .. {max(wall):.1f}) us")
        else:
            say("  scipy does not import here: the host loop was not timed")
say("clusters() is slower than clusters_torch on the device at: " + (", ".join(f"top = {t}, connectivity = {c}" for t, c in lost) if lost else "no setting"))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
