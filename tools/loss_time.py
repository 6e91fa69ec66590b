#!/usr/bin/env python3
"""FALoss / SupConLoss: kernel path against the torch-op path of the same call on the same GPU, per fixture shape.

The torch-op path (losses.fa_loss_torch / supcon_loss_torch) is the reference's op sequence on stock ROCm torch, i.e. the
baseline.  Per shape and path: forward + backward time (device events around `reps` back-to-back calls, best of 5 windows,
after a warm-up of the shape), device kernels per call (torch.profiler, one call, in a pass of its own) and the peak memory
growth of one call.  Shapes whose torch-op path would need more than --max-gb of similarity matrices are timed on the
kernel path only.

    python tools/loss_time.py [--reps 20] [--max-gb 8]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _loss_inputs as LI                      # noqa: E402
from transmf_ad_amd import losses as L         # noqa: E402

DEV = torch.device("cuda")


def window(fn, reps):
    best = 1e30
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _i in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps)
    return best * 1e3                           # us


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def measure(fn, reps):
    fn()
    fn()
    torch.cuda.synchronize()
    t = window(fn, reps)
    return t, launches(fn), peak(fn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-gb", type=float, default=8.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("loss_time.py needs a GPU")
    one = torch.ones((), device=DEV)
    print(f"device: {torch.cuda.get_device_name(0)}; forward + backward per call, best of 5 windows of {args.reps} calls")
    print(f"{'case':24s} {'layout':6s} {'path':8s} {'us/call':>10s} {'kernels':>8s} {'peak MiB':>9s}")
    for name, (B, C, spatial) in LI.FA_CASES.items():
        a, b = LI.fa_inputs(B, C, spatial)
        N = int(np.prod(spatial))
        for layout in ("ncdhw", "cl"):
            x, y = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
            if layout == "cl":
                lx = x.permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True)
                ly = y.permute(0, 2, 3, 4, 1).contiguous().requires_grad_(True)
                x, y = lx.permute(0, 4, 1, 2, 3), ly.permute(0, 4, 1, 2, 3)
            else:
                lx, ly = x.requires_grad_(True), y.requires_grad_(True)
            assert L.fa_kernel_ok(x, y)
            paths = [("kernel", L.FALoss())]
            if 5 * B * N * N * 4 / 2 ** 30 <= args.max_gb:
                paths.append(("torch", L.fa_loss_torch))
            for tag, loss_fn in paths:
                def call():
                    lx.grad = ly.grad = None
                    loss_fn(x, y).backward(one)
                t, n, p = measure(call, args.reps if N < 8192 else max(3, args.reps // 5))
                print(f"{name:24s} {layout:6s} {tag:8s} {t:10.1f} {n:8d} {p:9.1f}", flush=True)
            if len(paths) == 1:
                print(f"{name:24s} {layout:6s} torch    not run: needs about {5 * B * N * N * 4 / 2 ** 30:.0f} GiB of N x N matrices")
    for name, (bs, views, d, positives, mode, shape) in LI.SC_CASES.items():
        f, labels, mask = LI.sc_inputs(bs, views, d, positives, shape)
        x = torch.from_numpy(f).to(DEV).requires_grad_(True)
        lab = None if labels is None else torch.from_numpy(labels).to(DEV)
        msk = None if mask is None else torch.from_numpy(mask).to(DEV)
        assert L.supcon_kernel_ok(x)
        mod = L.SupConLoss(contrast_mode=mode)
        base = (torch.eq(lab.view(-1, 1), lab.view(1, -1)).float() if lab is not None else msk if msk is not None
                else torch.eye(bs, device=DEV))

        def kernel_call():
            x.grad = None
            mod(x, labels=lab, mask=msk).backward(one)

        def torch_call():
            x.grad = None
            L.supcon_loss_torch(x.reshape(bs, views, -1), base, mode == "all", 0.07, 0.07).backward(one)
        for tag, call in (("kernel", kernel_call), ("torch", torch_call)):
            t, n, p = measure(call, args.reps)
            print(f"{name:24s} {'-':6s} {tag:8s} {t:10.1f} {n:8d} {p:9.1f}", flush=True)


if __name__ == "__main__":
    main()
