#!/usr/bin/env python3
"""Region Shapley values on one device: the kernels of csrc/shap.hip beside their stock-torch twins on the same device tensors,
each call between two device events after three warm-up calls, the median of the timed calls, everything in one process.
  shap_apply   one chunk of 32 jobs of 96^3 under an atlas of R = 116 regions (tmf_shap_apply) against ops.shap_apply_torch and
               against tmf_occlude_labels at the same K, which writes the same bytes; floor: the chunk written, K * V * 4 bytes,
               over the HBM rate.
  shap_gram    (P, N) = (116, 2048), (232, 2048), (1024, 4096), B = 1 (tmf_shap_gram) against ops.shap_gram_torch.
  shap_solve   the same (P, N), B = 1 (tmf_shap_solve) against ops.shap_solve_torch (torch.linalg on the device).
  region_shap  the whole region_shap(model_ad.eval(), mri, pet, atlas=..., samples=N) against region_shap_torch, one timed call
               each per run after a short warm-up call, and the share of the call that is the network's forward on the chunks.
The tool repeats its table (--repeats, default 3) so that the spread between runs stands next to every difference it reports.
    python tools/shap_time.py [--size 96] [--regions 116] [--samples 2048] [--calls 30] [--repeats 3] [--out FILE]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=96)
ap.add_argument("--regions", type=int, default=116)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--repeats", type=int, default=3)
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


def row(what, name, us, floor=None):
    med = statistics.median(us)
    say(f"  {what}: {name}: {med:11.1f} ({min(us):.1f} .. {max(us):.1f}) us"
        + (f" = {med / floor:6.2f} x the byte floor ({floor:.1f} us)" if floor else ""))
    return med


torch.manual_seed(0)
S, R, N, K = args.size, args.regions, args.samples, args.chunk
size, V = (S, S, S), S ** 3
g = torch.Generator().manual_seed(2)
side = max(2, round(R ** (1 / 3) + 0.5))                   # a block atlas of about R regions, some background
idx = [torch.div(torch.arange(S) * side, S, rounding_mode="floor") for _ in range(3)]
atlas = ((idx[0].view(-1, 1, 1) * side + idx[1].view(1, -1, 1)) * side + idx[2].view(1, 1, -1) + 1).to(torch.int32)
atlas = torch.where(atlas > R, torch.zeros_like(atlas), atlas).to(DEV).contiguous()
P2 = 2 * R
coal = ops.shap_coalitions(P2, True, 0, 0, N, DEV)
rows = torch.cat([coal, torch.zeros((1, coal.shape[1]), device=DEV, dtype=coal.dtype)])
vol8 = torch.rand((8, 1) + size, device=DEV)
fill8 = torch.zeros(8, device=DEV)
buf = torch.empty((K, 1) + size, device=DEV)
j0 = 3 * (N + 1) + 5                                       # a chunk inside one sample, as nearly every chunk of a call is
say(f"region Shapley values at {S}^3 float32, R = {R} regions (P = {P2} jointly), N = {N} coalitions, us per call: median (min .. max) "
    f"after warm-up calls")
ratios = {}
for rep in range(args.repeats):
    say(f"run {rep + 1} of {args.repeats}")
    floor = K * V * 4 / (HBM_TBS * 1e12) * 1e6
    what = f"chunk of {K} jobs"
    k = row(what, "shap_apply (tmf_shap_apply)         ", timed(lambda: ops.shap_apply(vol8, atlas, rows, fill8, R, R, P2, j0, K, out=buf), args.calls), floor)
    t = row(what, "shap_apply_torch (stock ops)        ", timed(lambda: ops.shap_apply_torch(vol8, atlas, rows, fill8, R, R, P2, j0, K, out=buf), args.calls), floor)
    o = row(what, "occlude_labels (tmf_occlude_labels) ", timed(lambda: ops.occlude_labels(vol8, atlas, fill8, R, 3 * R + 5, K, out=buf), args.calls), floor)
    ratios.setdefault("shap_apply / shap_apply_torch", []).append(k / t)
    ratios.setdefault("shap_apply / occlude_labels", []).append(k / o)
    say(f"  {what}: kernel / stock ops = {k / t:.4f}, kernel / tmf_occlude_labels = {k / o:.4f}")
    if rep == 0:
        a = ops.shap_apply(vol8, atlas, rows, fill8, R, R, P2, j0, K).clone()
        say(f"  {what}: the kernel's bits equal the stock ops': {torch.equal(a, ops.shap_apply_torch(vol8, atlas, rows, fill8, R, R, P2, j0, K))}")
    for P, n in ((R, N), (2 * R, N), (1024, 2 * N)):
        c = ops.shap_coalitions(P, True, 0, 0, n, DEV)
        scores, empty = torch.rand((1, n), device=DEV), torch.rand((1,), device=DEV)
        what = f"P = {P}, N = {n}"
        k = row(what, "shap_gram (tmf_shap_gram)           ", timed(lambda: ops.shap_gram(c, scores, empty, P), args.calls))
        t = row(what, "shap_gram_torch (stock ops)         ", timed(lambda: ops.shap_gram_torch(c, scores, empty, P), args.calls))
        ratios.setdefault(f"shap_gram P = {P}", []).append(k / t)
        A, rhs = ops.shap_gram(c, scores, empty, P)
        delta = torch.ones((1,), device=DEV, dtype=torch.float64)
        k = row(what, "shap_solve (tmf_shap_solve)         ", timed(lambda: ops.shap_solve(A, rhs, delta), args.calls))
        t = row(what, "shap_solve_torch (torch.linalg)     ", timed(lambda: ops.shap_solve_torch(A, rhs, delta), args.calls))
        ratios.setdefault(f"shap_solve P = {P}", []).append(k / t)
        if rep == 0:
            a, b = ops.shap_solve(A, rhs, delta), ops.shap_solve_torch(A, rhs, delta)
            say(f"  {what}: info {int(a[1])} / {int(b[1])}, max |kernel - stock ops| / max |phi| = "
                f"{float((a[0] - b[0]).abs().max() / b[0].abs().max()):.2e}")

# the whole call on the workload's model
torch.manual_seed(1)
net = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.).to(DEV).eval()
mri, pet = torch.rand((1, 1) + size, device=DEV), torch.rand((1, 1) + size, device=DEV)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


with torch.no_grad():
    batch = (torch.rand((K, 1) + size, device=DEV), torch.rand((K, 1) + size, device=DEV))
    fwd = statistics.median(timed(lambda: net(*batch), 10)) / 1e6
chunks = -(-(N + 1) // K)
say(f"region_shap(model_ad.eval(), mri, pet, atlas, samples={N}) at {S}^3, B = 1, joint, chunk {K}: seconds per call (one call per run "
    f"after a warm-up call with samples={2 * P2}); the model's forward on one chunk of {K}: {fwd * 1e3:.1f} ms, {chunks} chunks per "
    f"call = {chunks * fwd:.2f} s")
for fn in (T.region_shap, T.region_shap_torch):
    fn(net, mri, pet, atlas=atlas, samples=2 * P2, chunk=K)
for rep in range(args.repeats):
    k = wall(lambda: T.region_shap(net, mri, pet, atlas=atlas, samples=N, chunk=K))
    t = wall(lambda: T.region_shap_torch(net, mri, pet, atlas=atlas, samples=N, chunk=K))
    ratios.setdefault("region_shap / region_shap_torch", []).append(k / t)
    say(f"  run {rep + 1}: region_shap {k:.3f} s (the forward's share {chunks * fwd / k:.2f}), region_shap_torch {t:.3f} s (the forward's "
        f"share {chunks * fwd / t:.2f}); region_shap / region_shap_torch = {k / t:.4f}")
say(f"kernel path / the other path over the {args.repeats} runs, lowest .. highest:")
lost = []
for what, rs in ratios.items():
    say(f"  {what}: {min(rs):.4f} .. {max(rs):.4f}")
    if max(rs) >= 1.0:
        lost.append(what)
say("the kernel path is not faster in every run on: " + (", ".join(lost) if lost else "no row"))

if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(out) + "\n")
