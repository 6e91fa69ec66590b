#!/usr/bin/env python3
"""Deletion / insertion curves on one device, timed with device events after a warm-up, in one process:
  the whole call transmf_ad_amd.faithfulness_curve with reuse=True and with reuse=False, both modes;
  the user's loop - torch.sort of the attribution, torch.where per step, one model call per chunk, scores by torch ops -
  which stands for what the library offered without this call;
  the two entries alone (tmf_rank_thresholds on the batch, tmf_mask_by_rank on one chunk) with the bytes they move, beside
  torch.sort, the torch.where loop of a chunk and one forward of the model on a chunk.
    python tools/faithfulness_time.py [--size 96] [--steps 20] [--batch 1] [--chunk 32] [--model ad|cnn] [--out FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import transmf_ad_amd as T  # noqa: E402
from transmf_ad_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--steps", type=int, default=20)
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
N, S, B, chunk = args.size, args.steps, args.batch, args.chunk
size, V = (N, N, N), N ** 3
mri, pet = torch.rand((B, 1) + size, device=DEV), torch.rand((B, 1) + size, device=DEV)
attr = torch.rand((B,) + size, device=DEV)              # distinct values for all practical purposes: the sort has no shortcut
counts = ops.rank_counts(V, S)
nJ = B * (S + 1)


def users_loop(mode):
    vols = [mri, pet]
    with torch.no_grad():
        base = net(*vols)[0]
        target = base.argmax(1)
        a = attr.reshape(B, V)
        srt = torch.sort(a, 1, descending=True).values
        thr = srt[:, torch.tensor(counts, device=DEV) - 1]
        scores = torch.empty((nJ,), device=DEV)
        zero = torch.zeros((), device=DEV)
        for j0 in range(0, nJ, chunk):
            jobs = range(j0, min(j0 + chunk, nJ))
            rows = torch.tensor([j // (S + 1) for j in jobs], device=DEV)
            xs = []
            for j in jobs:
                b, s = divmod(j, S + 1)
                m = (a[b] >= thr[b, s - 1] if s else torch.zeros_like(a[b], dtype=torch.bool)).view(mri.shape[1:])
                xs.append(torch.where(m, zero, mri[b]) if mode == "deletion" else torch.where(m, mri[b], zero))
            lo = net(torch.stack(xs), pet.index_select(0, rows))[0]
            scores[j0:j0 + len(jobs)] = torch.softmax(lo, 1).gather(1, target[rows].view(-1, 1))[:, 0]
    return scores.view(B, S + 1)


say(f"model_{args.model} (dim 128) eval, B = {B}, {N}^3 volumes, steps = {S}: {nJ} jobs of the MRI in chunks of {chunk}; ms per whole "
    f"call, {args.rounds} calls each after one warm-up call")
for mode in ("deletion", "insertion"):
    curve = lambda reuse: T.faithfulness_curve(net, mri, pet, attribution=attr, volume=0, steps=S, mode=mode, chunk=chunk, reuse=reuse)
    variants = [("faithfulness_curve reuse=True ", lambda: curve(True)), ("faithfulness_curve reuse=False", lambda: curve(False)),
                ("the user's loop (sort + where)", lambda: users_loop(mode))]
    best = {}
    for name, fn in variants:
        fn()
        ms = timed(fn, args.rounds)
        best[name] = min(ms)
        say(f"  {mode:9s} {name}: " + " / ".join(f"{m:.2f}" for m in ms) + " ms")
    names = [n for n, _f in variants]
    say(f"  {mode:9s} reuse=True / reuse=False = {best[names[0]] / best[names[1]]:.3f}; reuse=True / user's loop = "
        f"{best[names[0]] / best[names[2]]:.3f}; reuse=False / user's loop = {best[names[1]] / best[names[2]]:.3f}")
    a, b = curve(True), users_loop(mode)
    say(f"  {mode:9s} max |scores - user's loop| = {float((a.scores - b).abs().max()):.2e}; range of the curve "
        f"{float((b.amax(1) - b.amin(1)).min()):.2e}; auc {a.auc.tolist()}")

# the entries alone, beside what they replace and one forward on a chunk
K = min(chunk, nJ)
fill = torch.zeros(B, device=DEV)
thr, _removed = ops.rank_thresholds(attr, counts)
nbuf = max(2, -(-(600 << 20) // (K * V * 4)))            # rotate outputs: more than the 256 MB of last-level cache
bufs = [torch.empty((K, 1) + size, device=DEV) for _ in range(nbuf)]
state = {"i": 0}


def mask():
    state["i"] += 1
    ops.mask_by_rank(mri, attr, thr, fill, "deletion", 0, K, out=bufs[state["i"] % nbuf])


def where_loop():
    a, zero = attr.reshape(B, V), torch.zeros((), device=DEV)
    xs = []
    for j in range(K):
        b, s = divmod(j, S + 1)
        m = (a[b] >= thr[b, s - 1] if s else torch.zeros_like(a[b], dtype=torch.bool)).view(mri.shape[1:])
        xs.append(torch.where(m, zero, mri[b]))
    return torch.stack(xs)


with torch.no_grad():
    rows = torch.zeros(K, dtype=torch.long, device=DEV)
    pet_rows = pet.index_select(0, rows)
    fwd = lambda: net(bufs[0], pet_rows)
    for name, fn, nbytes in ((f"tmf_rank_thresholds, B = {B}, S = {S} (attr read once per digit: three times)", lambda: ops.rank_thresholds(attr, counts),
                              3 * B * V * 4),
                             ("torch.sort(descending=True) + gather", lambda: torch.sort(attr.reshape(B, V), 1, descending=True), None),
                             (f"tmf_mask_by_rank, one chunk of {K} (K volumes written, vol and attr read through the caches)", mask, (K + 2 * B) * V * 4),
                             (f"torch.where per job + stack, one chunk of {K}", where_loop, None),
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
