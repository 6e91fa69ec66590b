#!/usr/bin/env python3
"""Occlusion sensitivity on one device, timed with device events after a warm-up, in one process:
  the whole call transmf_ad_amd.occlusion_sensitivity with reuse=True and with reuse=False;
  the user's loop - the same chunks built with clone() and slice assignment through the same model, drops by torch ops and the
  voxel map by a scatter-add per window - which stands for what the library offered without this call;
  the two kernels alone (tmf_occlude_windows on one chunk, tmf_occlusion_volume on the batch) with their achieved bytes/s,
  beside one forward of the model on a chunk.
    python tools/occlusion_time.py [--size 96] [--patch 12] [--batch 1] [--chunk 32] [--model ad|cnn] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transmf_ad_amd as T  # noqa: E402
from transmf_ad_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--patch", type=int, default=12)
ap.add_argument("--batch", type=int, default=1)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--model", choices=("ad", "cnn"), default="ad")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out")
args = ap.parse_args()
DEV = "cuda:0"
out = []


def say(s):
    print(s, flush=True)
    out.append(s)


def timed(fn, rounds):
    """[ms] of `rounds` single calls, each between two device events."""
    res = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        res.append(a.elapsed_time(b))
    return res


torch.manual_seed(0)
if args.model == "ad":
    net = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.)
else:
    net = T.model_CNN_ad(dim=128)
net = net.to(DEV).eval()
S, p, B, chunk = args.size, args.patch, args.batch, args.chunk
size, patch = (S, S, S), (p, p, p)
mri, pet = torch.rand((B, 1) + size, device=DEV), torch.rand((B, 1) + size, device=DEV)
grid = ops.occlusion_grid(size, patch, patch)
nW = grid[0] * grid[1] * grid[2]
windows = [ops.occlusion_window(size, patch, patch, w) for w in range(nW)]


def users_loop():
    vols = [mri, pet]
    with torch.no_grad():
        base = net(*vols)[0]
        target = base.argmax(1)
        score = base.gather(1, target.view(-1, 1))[:, 0]
        maps = []
        for i in (0, 1):
            drops = torch.empty((B * nW,), device=DEV)
            for j0 in range(0, B * nW, chunk):
                jobs = range(j0, min(j0 + chunk, B * nW))
                rows = torch.tensor([j // nW for j in jobs], device=DEV)
                batch = [v.index_select(0, rows) for v in vols]
                batch[i] = batch[i].clone()
                for k, j in enumerate(jobs):
                    batch[i][k][(..., *windows[j % nW])] = 0.0
                lo = net(*batch)[0]
                drops[j0:j0 + len(jobs)] = score[rows] - lo.gather(1, target[rows].view(-1, 1))[:, 0]
            drops = drops.view(B, nW)
            acc, cnt = torch.zeros((B,) + size, device=DEV), torch.zeros(size, device=DEV)
            for w, win in enumerate(windows):
                acc[(slice(None), *win)] += drops[:, w].view(B, 1, 1, 1)
                cnt[win] += 1
            maps.append(acc / cnt)
    return maps


say(f"model_{args.model} (dim 128) eval, B = {B}, {S}^3 volumes, {p}^3 windows: nW = {nW} per volume, {2 * B * nW} jobs in chunks of "
    f"{chunk}; ms per whole call, {args.rounds} calls each after one warm-up call")
variants = [("occlusion_sensitivity reuse=True ", lambda: T.occlusion_sensitivity(net, mri, pet, patch=p, chunk=chunk, reuse=True)),
            ("occlusion_sensitivity reuse=False", lambda: T.occlusion_sensitivity(net, mri, pet, patch=p, chunk=chunk, reuse=False)),
            ("the user's loop (torch batches)  ", users_loop)]
best = {}
for name, fn in variants:
    fn()
    ms = timed(fn, args.rounds)
    best[name] = min(ms)
    say(f"  {name}: " + " / ".join(f"{m:.1f}" for m in ms) + " ms")
names = [n for n, _f in variants]
say(f"  reuse=True / reuse=False = {best[names[0]] / best[names[1]]:.3f}; reuse=True / user's loop = {best[names[0]] / best[names[2]]:.3f}; "
    f"reuse=False / user's loop = {best[names[1]] / best[names[2]]:.3f}")
a, b = T.occlusion_sensitivity(net, mri, pet, patch=p, chunk=chunk, reuse=True), users_loop()
say("  max |voxel map - user's loop| = " + ", ".join(f"{float((a.volume(i) - b[i]).abs().max()):.2e}" for i in (0, 1))
    + "; max |drop| = " + ", ".join(f"{float(a.drops(i).abs().max()):.2e}" for i in (0, 1)))

# the kernels alone, beside one forward on a chunk
K = min(chunk, B * nW)
fill = torch.zeros(B, device=DEV)
nbuf = max(2, -(-(600 << 20) // (K * S ** 3 * 4)))            # rotate outputs: more than the 256 MB of last-level cache
bufs = [torch.empty((K, 1) + size, device=DEV) for _ in range(nbuf)]
state = {"i": 0}


def occlude():
    state["i"] += 1
    ops.occlude_windows(mri, fill, patch, patch, 0, K, out=bufs[state["i"] % nbuf])


def clone_assign():
    x = mri.index_select(0, torch.zeros(K, dtype=torch.long, device=DEV)).clone()
    for k in range(K):
        x[k][(..., *windows[k % nW])] = 0.0
    return x


drops = torch.randn((B, nW), device=DEV)
with torch.no_grad():
    rows = torch.zeros(K, dtype=torch.long, device=DEV)
    pet_rows = pet.index_select(0, rows)
    fwd = lambda: net(bufs[0], pet_rows)
    for name, fn, nbytes in (("tmf_occlude_windows, one chunk", occlude, (K + 1) * S ** 3 * 4),
                             ("clone() + slice assignment, one chunk", clone_assign, None),
                             ("tmf_occlusion_volume", lambda: ops.occlusion_volume(drops, size, patch, patch), B * S ** 3 * 4),
                             (f"model forward on one chunk of {K}", fwd, None)):
        fn()
        reps = 20
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        say(f"  {name}: {us:.1f} us per call ({reps} calls)" + (f", {nbytes / 1e6:.1f} MB -> {nbytes / us / 1e6:.2f} TB/s" if nbytes else ""))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
