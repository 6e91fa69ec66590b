#!/usr/bin/env python3
"""tmf_cam (csrc/cam.hip) beside the torch formula at B = 8 on the three useful layers of the 96^3 configuration: device events
around windows of calls, the two alternating, buffer sets rotated so that a window streams more than the 256 MB of last-level
cache.   python tools/cam_time.py [--out FILE] [--reps N]     (--reps: calls per window, for a short run under a profiler)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transmf_ad_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out")
ap.add_argument("--reps", type=int, default=0)
args = ap.parse_args()
DEV = "cuda:0"
SHAPES = [(8, 24 ** 3, 64), (8, 12 ** 3, 128), (8, 48 ** 3, 32)]
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def torch_formula(A, G, method):
    cam = ((A * G.mean(1, keepdim=True)) if method == 0 else (A * G)).sum(-1).relu()
    m = cam.amax(1, keepdim=True)
    return torch.where(m > 0, cam / m, torch.zeros_like(cam))


def window(fn, sets, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(reps):
        fn(sets[i % len(sets)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


for B, V, C in SHAPES:
    nbytes = B * V * C * 4
    nsets = max(2, -(-(600 << 20) // (2 * nbytes)))
    g = torch.Generator(device=DEV).manual_seed(1)
    sets = [(torch.randn((B, V, C), device=DEV, generator=g), torch.randn((B, V, C), device=DEV, generator=g)) for _ in range(nsets)]
    cam = torch.empty((B, V), device=DEV)
    w, peak = torch.empty((B, C), device=DEV), torch.empty((B,), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    for method, name in ((0, "gradcam"), (1, "hirescam")):
        nws = _lib.query("tmf_cam_workspace_bytes", B, V, C, method)
        ws = torch.empty(nws, device=DEV, dtype=torch.uint8)

        def kernel(s):
            _lib.call("tmf_cam", s[0].data_ptr(), s[1].data_ptr(), cam.data_ptr(), w.data_ptr() if method == 0 else None,
                      peak.data_ptr(), ws.data_ptr(), nws, B, V, C, method, 3, st)

        def formula(s):
            return torch_formula(s[0], s[1], method)

        kernel(sets[0])
        ref = formula(sets[0])
        torch.cuda.synchronize()
        err = float((cam - ref).abs().max())
        reps = args.reps or max(50, min(2000, (64 << 30) // (2 * nbytes)))
        for fn in (kernel, formula):
            window(fn, sets, 10)
        rounds = [(window(kernel, sets, reps), window(formula, sets, reps)) for _ in range(3)]
        k, f = min(r[0] for r in rounds), min(r[1] for r in rounds)
        say(f"B={B} V={V} C={C} {name}: tmf_cam " + " / ".join(f"{r[0]:.1f}" for r in rounds) + " us, torch formula "
            + " / ".join(f"{r[1]:.1f}" for r in rounds) + f" us per call ({reps} calls per window, {nsets} buffer sets of "
            f"{2 * nbytes / 2 ** 20:.0f} MB); A + G = {2 * nbytes / 1e6:.1f} MB -> {2 * nbytes / k / 1e6:.2f} TB/s at the best "
            f"window; torch / kernel = {f / k:.1f}; max |kernel - torch| = {err:.2e}")
    del sets

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
