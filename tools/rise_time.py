#!/usr/bin/env python3
"""RISE on one device: the kernels of csrc/rise.hip beside their stock-torch twins on the same device tensors, each call between
two device events after three warm-up calls, the median of the timed calls, everything in one process.
  rise_apply       one chunk of 32 jobs of 96^3 (tmf_rise_apply) against ops.rise_apply_torch; floor: the chunk written and the
                   two samples it straddles read once, (K + 2) * V * 4 bytes over the HBM rate.
  rise_accumulate  B = 1 and 8, N = 2000 masks, cells 8 (tmf_rise_accumulate) against ops.rise_accumulate_torch; floor: N * V
                   mask evaluations at the vector instructions one evaluation takes in the kernel's listing (VALU_PER_EVAL:
                   the mask loop of the B = 1 and of the B = 8 instantiation, blocks skipped by a wave-uniform branch left out)
                   over the chip's lane rate.
  rise             the whole rise(model_ad.eval(), mri, pet, masks=N) against rise_torch, one timed call each per run after a
                   short warm-up call, and the share of the call that is the network's forward on the chunks.
The tool repeats its table (--repeats, default 3) so that the spread between runs stands next to every difference it reports.
    python tools/rise_time.py [--size 96] [--masks 2000] [--calls 30] [--repeats 3] [--whole-masks 2000] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transmf_ad_amd as T  # noqa: E402
from transmf_ad_amd import ops  # noqa: E402

HBM_TBS = 8.0               # HBM3E peak of the MI355X; a float4 copy reaches 6.3 TB/s
LANE_RATE = 256 * 4 * 16 * 2.4e9        # compute units x SIMDs x lanes per cycle x clock: fp32 vector instructions per second per lane
VALU_PER_EVAL = {1: 56, 8: 70}          # vector instructions per mask evaluation in the mask loop of rise_accumulate_kernel<true>

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--masks", type=int, default=2000)
ap.add_argument("--cells", type=int, default=8)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--twin-calls", type=int, default=5, help="timed calls of rise_accumulate_torch (seconds each)")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--whole-masks", type=int, default=2000)
ap.add_argument("--out")
args = ap.parse_args()
DEV = "cuda:0"
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, calls, warm=3):
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


torch.manual_seed(0)
S, N, K = args.size, args.masks, args.chunk
size, cells, V = (S, S, S), (args.cells,) * 3, S ** 3
nodes, shifts = ops.rise_masks(size, cells, 0.5, 0, 0, N, DEV)
vol8 = torch.rand((8, 1) + size, device=DEV)
fill8 = torch.zeros(8, device=DEV)
buf = torch.empty((K, 1) + size, device=DEV)
j0 = N - K // 2                                            # a chunk that straddles two samples
say(f"RISE at {S}^3 float32, cells {args.cells}, N = {N} masks, us per call: median (min .. max) after warm-up calls")
ratios = {}
for rep in range(args.repeats):
    say(f"run {rep + 1} of {args.repeats}")
    floor = (K + 2) * V * 4 / (HBM_TBS * 1e12) * 1e6
    res = {}
    for name, fn, calls in (("rise_apply (tmf_rise_apply)      ", lambda: ops.rise_apply(vol8, nodes, shifts, fill8, size, cells, j0, K, out=buf), args.calls),
                            ("rise_apply_torch (stock ops)     ", lambda: ops.rise_apply_torch(vol8, nodes, shifts, fill8, size, cells, j0, K, out=buf), args.calls)):
        us = timed(fn, calls)
        res[name] = statistics.median(us)
        say(f"  chunk of {K} jobs: {name}: {res[name]:11.1f} ({min(us):.1f} .. {max(us):.1f}) us = {res[name] / floor:8.1f} x the byte "
            f"floor ({floor:.1f} us)")
    k, t = res.values()
    ratios.setdefault("rise_apply", []).append(k / t)
    say(f"  chunk of {K} jobs: kernel / stock ops = {k / t:.4f}")
    if rep == 0:
        a = ops.rise_apply(vol8, nodes, shifts, fill8, size, cells, j0, K).clone()
        say(f"  chunk of {K} jobs: the kernel's bits equal the stock ops': {torch.equal(a, ops.rise_apply_torch(vol8, nodes, shifts, fill8, size, cells, j0, K))}")
    for B in (1, 8):
        scores = torch.rand((B, N), device=DEV)
        floor = N * V * VALU_PER_EVAL[B] / LANE_RATE * 1e6
        res = {}
        for name, fn, calls in (("rise_accumulate (tmf_rise_accumulate)", lambda: ops.rise_accumulate(scores, nodes, shifts, size, cells, 1.0 / N), args.calls),
                                ("rise_accumulate_torch (stock ops)    ", lambda: ops.rise_accumulate_torch(scores, nodes, shifts, size, cells, 1.0 / N), args.twin_calls)):
            us = timed(fn, calls, warm=3 if calls >= 20 else 1)
            res[name] = statistics.median(us)
            say(f"  B = {B}: {name}: {res[name]:11.1f} ({min(us):.1f} .. {max(us):.1f}) us of {calls} calls = {res[name] / floor:6.2f} x "
                f"the instruction floor ({floor:.1f} us at {VALU_PER_EVAL[B]} vector instructions per evaluation)")
        k, t = res.values()
        ratios.setdefault(f"rise_accumulate B = {B}", []).append(k / t)
        say(f"  B = {B}: kernel / stock ops = {k / t:.4f}")
        if rep == 0:
            a, b = ops.rise_accumulate(scores, nodes, shifts, size, cells, 1.0 / N), ops.rise_accumulate_torch(scores, nodes, shifts, size, cells, 1.0 / N)
            say(f"  B = {B}: max |kernel - stock ops| / max |map| = {float((a - b).abs().max() / b.abs().max()):.2e}")

# the whole call on the workload's model
torch.manual_seed(1)
net = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.).to(DEV).eval()
mri, pet = torch.rand((1, 1) + size, device=DEV), torch.rand((1, 1) + size, device=DEV)
Nw = args.whole_masks


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


with torch.no_grad():
    batch = (torch.rand((K, 1) + size, device=DEV), torch.rand((K, 1) + size, device=DEV))
    fwd = statistics.median(timed(lambda: net(*batch), 10)) / 1e6
chunks = 2 * -(-Nw // K)
say(f"rise(model_ad.eval(), mri, pet, masks={Nw}) at {S}^3, B = 1, chunk {K}: seconds per call (one call per run after a warm-up call "
    f"with masks={2 * K}); the model's forward on one chunk of {K}: {fwd * 1e3:.1f} ms, {chunks} chunks per call with both encoders "
    f"(reuse=False) = {chunks * fwd:.2f} s")
for fn in (T.rise, T.rise_torch):
    fn(net, mri, pet, masks=2 * K, chunk=K)
for rep in range(args.repeats):
    k = wall(lambda: T.rise(net, mri, pet, masks=Nw, chunk=K))
    k0 = wall(lambda: T.rise(net, mri, pet, masks=Nw, chunk=K, reuse=False))
    t = wall(lambda: T.rise_torch(net, mri, pet, masks=Nw, chunk=K))
    ratios.setdefault("rise reuse=False / rise_torch", []).append(k0 / t)
    ratios.setdefault("rise reuse=True / rise_torch", []).append(k / t)
    say(f"  run {rep + 1}: rise reuse=True {k:.3f} s, rise reuse=False {k0:.3f} s (the forward's share {chunks * fwd / k0:.2f}), "
        f"rise_torch {t:.3f} s (the forward's share {chunks * fwd / t:.2f}); rise / rise_torch = {k / t:.4f}, reuse=False {k0 / t:.4f}")
say(f"kernel path / stock ops over the {args.repeats} runs, lowest .. highest:")
lost = []
for what, rs in ratios.items():
    say(f"  {what}: {min(rs):.4f} .. {max(rs):.4f}")
    if max(rs) >= 1.0:
        lost.append(what)
say("the kernel path is not faster than the stock ops in every run on: " + (", ".join(lost) if lost else "no row"))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
