#!/usr/bin/env python3
"""Atlas region statistics on one device: transmf_ad_amd.region_stats (tmf_region_stats) beside region_stats_torch (bincount,
index_add_, scatter_reduce - the stock ops it replaces) on the same tensors, each call between two device events after a
warm-up, the median of the timed calls; beside each time the byte floor (B*V + V) * 4 bytes - the map and the atlas read once -
over the HBM rate.  B = 8 at 96^3 with R = 116 (an AAL-like atlas of coherent bricks), R = 1 and R = the kernels' limit; the
group accumulator's update beside its torch ops.
    python tools/region_time.py [--size 96] [--batch 8] [--calls 30] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transmf_ad_amd as T  # noqa: E402
from transmf_ad_amd import ops  # noqa: E402

HBM_TBS = 8.0               # HBM3E peak of the MI355X; a float4 copy reaches 6.3 TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--out")
args = ap.parse_args()
if args.calls < 20:
    ap.error("--calls must be at least 20")
DEV = "cuda:0"
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, calls):
    """[us] of `calls` single calls, each between two device events, after three warm-up calls."""
    for _ in range(3):
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


def bricks(N, R, side):
    """Coherent bricks of `side`^3 voxels, labels 1..R in brick order, background outside the inner 3/4 of each axis."""
    i = torch.arange(N) // side
    n = (N + side - 1) // side
    z, y, x = torch.meshgrid(i, i, i, indexing="ij")
    lab = ((z * n + y) * n + x) % R + 1
    lo, hi = N // 8, N - N // 8
    inner = torch.zeros((N, N, N), dtype=torch.bool)
    inner[lo:hi, lo:hi, lo:hi] = True
    return torch.where(inner, lab, torch.zeros_like(lab)).to(torch.int32)


torch.manual_seed(0)
N, B = args.size, args.batch
V = N ** 3
a = torch.randn((B, N, N, N), device=DEV)
floor_us = (B * V + V) * 4 / (HBM_TBS * 1e12) * 1e6
say(f"region_stats on B = {B} maps of {N}^3 float32, us per call: median (min .. max) of {args.calls} calls after 3 warm-up calls; byte "
    f"floor (B*V + V) * 4 = {(B * V + V) * 4 / 1e6:.1f} MB at {HBM_TBS} TB/s = {floor_us:.1f} us")
lost = []
for R, side, what in ((116, 12, "bricks of 12^3"), (1, N, "one region"), (ops.REGION_MAX, 6, "bricks of 6^3"),
                      (116, 1, "a different label at every voxel")):
    atlas = bricks(N, R, side).to(DEV)
    flat = atlas.view(-1)
    res = {}
    for name, fn in (("region_stats (tmf_region_stats)", lambda: ops.region_stats(a.view(B, V), flat, R)),
                     ("region_stats_torch (stock ops)  ", lambda: ops.region_stats_torch(a.view(B, V), flat, R))):
        us = timed(fn, args.calls)
        res[name] = statistics.median(us)
        say(f"  R = {R:4d}, {what}: {name}: {res[name]:9.1f} ({min(us):.1f} .. {max(us):.1f}) us = {res[name] / floor_us:7.1f} x the byte floor")
    k, t = res.values()
    say(f"  R = {R:4d}, {what}: kernel / stock ops = {k / t:.3f}")
    if k > t:
        lost.append((R, what))
    rs, rt = T.region_stats(a, atlas, R), T.region_stats_torch(a, atlas, R)
    err = max(float((getattr(rs, n) - getattr(rt, n)).abs().max() / getattr(rt, n).abs().max().clamp(min=1e-30))
              for n in ("sum", "abs_sum", "pos_sum"))
    say(f"  R = {R:4d}, {what}: max |kernel - stock ops| / max |stock ops| of the sums {err:.2e}; count, max, argmax equal: "
        f"{torch.equal(rs.count, rt.count) and torch.equal(rs.max, rt.max) and torch.equal(rs.argmax, rt.argmax)}")
say("the kernel path is slower than the stock ops on: " + (", ".join(f"R = {R} ({w})" for R, w in lost) if lost else "no shape"))

R, C = 116, 2
vals = torch.rand((B, R + 1), device=DEV)
cls = torch.randint(0, C, (B,), device=DEV)
state = torch.zeros((C, R + 1, 3), device=DEV, dtype=torch.float64)
for name, fn in (("region_group_update (tmf_region_group_update, one launch)", lambda: ops.region_group_update(state, vals, cls)),
                 ("the same sums by index_add_ in float64", lambda: ops.region_group_update(state, vals.double(), cls))):
    us = timed(fn, args.calls)
    say(f"  group update, B = {B}, R = {R}, C = {C}: {name}: {statistics.median(us):.1f} ({min(us):.1f} .. {max(us):.1f}) us")

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
