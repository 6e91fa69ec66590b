#!/usr/bin/env python3
"""Gaussian smoothing on one device: transmf_ad_amd.ops.gaussian_smooth (tmf_gaussian_smooth) beside ops.gaussian_smooth_torch
(one index_select, multiply and add per tap and axis - the stock-op loop it replaces) on the same device tensors, each call
between two device events after three warm-up calls, the median of the timed calls, everything in one process; beside each time
the byte floor 2 * B*V*4 bytes - the maps read once and written once - over the HBM rate.  B = 8 at 96^3; sigma 1 (r = 4), 2.265
(FWHM 8 mm at 1.5 mm, r = 9) and 4 (r = 16); without a mask and with a brick mask of density 0.5.  The tool repeats its table
(--repeats, default 3) so that the spread between runs stands next to every difference it reports.
    python tools/smooth_time.py [--size 96] [--batch 8] [--calls 30] [--repeats 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transmf_ad_amd import ops  # noqa: E402

HBM_TBS = 8.0               # HBM3E peak of the MI355X; a float4 copy reaches 6.3 TB/s

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--repeats", type=int, default=3)
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


def brick_mask(N, side=12):
    """Bricks of side^3 voxels, every other one inside (a 3-D chequerboard): density 0.5, coherent like a brain mask."""
    i = torch.arange(N) // side
    z, y, x = torch.meshgrid(i, i, i, indexing="ij")
    return ((z + y + x) % 2).to(torch.int32)


torch.manual_seed(0)
N, B = args.size, args.batch
V = N ** 3
a = torch.randn((B, N, N, N), device=DEV)
mask = brick_mask(N).to(DEV)
dst = torch.empty_like(a)
floor_us = 2 * B * V * 4 / (HBM_TBS * 1e12) * 1e6
say(f"gaussian_smooth on B = {B} maps of {N}^3 float32, reflect mode, us per call: median (min .. max) of {args.calls} calls after 3 "
    f"warm-up calls; byte floor 2 * B*V*4 = {2 * B * V * 4 / 1e6:.1f} MB at {HBM_TBS} TB/s = {floor_us:.1f} us; mask density "
    f"{float(mask.float().mean()):.2f}")
ratios = {}
for rep in range(args.repeats):
    say(f"run {rep + 1} of {args.repeats}")
    for sigma in (1.0, 2.265, 4.0):
        sig = (sigma,) * 3
        r = (ops.gaussian_taps(sigma).numel() - 1) // 2
        for m, what in ((None, "no mask"), (mask, "brick mask")):
            res = {}
            for name, fn in (("gaussian_smooth (tmf_gaussian_smooth)", lambda: ops.gaussian_smooth(a, sig, 4.0, "reflect", m, out=dst)),
                             ("gaussian_smooth_torch (stock ops)    ", lambda: ops.gaussian_smooth_torch(a, sig, 4.0, "reflect", m))):
                us = timed(fn, args.calls)
                res[name] = statistics.median(us)
                say(f"  sigma {sigma:5.3f} (r = {r:2d}), {what:10s}: {name}: {res[name]:9.1f} ({min(us):.1f} .. {max(us):.1f}) us = "
                    f"{res[name] / floor_us:7.1f} x the byte floor")
            k, t = res.values()
            ratios.setdefault((sigma, what), []).append(k / t)
            say(f"  sigma {sigma:5.3f} (r = {r:2d}), {what:10s}: kernel / stock ops = {k / t:.4f}")
            if rep == 0:
                got, twin = ops.gaussian_smooth(a, sig, 4.0, "reflect", m), ops.gaussian_smooth_torch(a, sig, 4.0, "reflect", m)
                say(f"  sigma {sigma:5.3f} (r = {r:2d}), {what:10s}: max |kernel - stock ops| / max |a| = "
                    f"{float((got - twin).abs().max() / a.abs().max()):.2e}")
say(f"kernel / stock ops over the {args.repeats} runs, lowest .. highest:")
lost = []
for (sigma, what), rs in ratios.items():
    say(f"  sigma {sigma:5.3f}, {what:10s}: {min(rs):.4f} .. {max(rs):.4f}")
    if max(rs) >= 1.0:
        lost.append(f"sigma {sigma} ({what})")
say("the kernel path is not faster than the stock ops in every run on: " + (", ".join(lost) if lost else "no row"))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
