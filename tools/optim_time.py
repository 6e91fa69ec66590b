#!/usr/bin/env python3
"""Step time of the one-launch SGD against torch.optim.SGD on the same GPU, same parameters, same gradients.

Parameters: the 156 tensors of model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0) (4.17 M floats), each
candidate on a copy of its own, with fixed random gradients.  Candidates: optim.SGD, torch.optim.SGD in its default
(multi-tensor) form and with fused=True where this torch build offers it, each with momentum 0 and 0.9, and optim.Adam as the
known yardstick.  All in ONE process: every candidate is warmed up first, then the candidates take turns,
one window of --steps optimizer steps each (host clock around the window, which ends in a device synchronise), --windows
rounds; per candidate the median window and the spread (min .. max) are reported as microseconds per step.  The number of
device kernels per step is counted by torch.profiler in a pass of its own after the timing.

    python tools/optim_time.py [--steps 200] [--windows 5]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import transmf_ad_amd as T                     # noqa: E402

DEV = torch.device("cuda")


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    # (the record_function range torch puts around Optimizer.step shows up on the device side as a user annotation)
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA and not e.is_user_annotation
               and not e.name.lower().startswith(("memcpy", "memset")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="optimizer steps per window")
    ap.add_argument("--windows", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("optim_time.py needs a GPU")
    torch.manual_seed(0)
    net = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.)
    base = [p.detach().to(DEV) for p in net.parameters()]
    grads = [torch.randn_like(p) * 1e-3 for p in base]
    numel = sum(p.numel() for p in base)

    def candidate(make):
        ps = [torch.nn.Parameter(p.clone()) for p in base]
        for p, g in zip(ps, grads):
            p.grad = g
        return make(ps)

    cands = []                                  # (label, optimizer | None, bytes per parameter, note)
    for mom in (0.0, 0.9):
        bpp = 20 if mom else 12                 # p read + g read + p written (+ buffer read + written)
        cands.append((f"optim.SGD momentum={mom:g}", candidate(lambda ps: T.optim.SGD(ps, lr=1e-4, momentum=mom)), bpp, ""))
        cands.append((f"torch.optim.SGD momentum={mom:g} (default)", candidate(lambda ps: torch.optim.SGD(ps, lr=1e-4, momentum=mom)), bpp, ""))
        try:
            fused = candidate(lambda ps: torch.optim.SGD(ps, lr=1e-4, momentum=mom, fused=True))
            fused.step()
            torch.cuda.synchronize()
            cands.append((f"torch.optim.SGD momentum={mom:g} fused=True", fused, bpp, ""))
        except Exception as e:                  # this build does not offer it
            cands.append((f"torch.optim.SGD momentum={mom:g} fused=True", None, bpp, f"not offered: {type(e).__name__}: {e}"))
    cands.append(("optim.Adam (yardstick)", candidate(lambda ps: T.optim.Adam(ps, lr=1e-4)), 28, ""))

    live = [c for c in cands if c[1] is not None]
    for _label, opt, _b, _n in live:            # warm-up of every candidate: state allocation, code objects, allocator
        for _ in range(20):
            opt.step()
    torch.cuda.synchronize()
    times = {label: [] for label, *_ in live}
    for _w in range(args.windows):              # alternating: one window per candidate per round
        for label, opt, _b, _n in live:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                opt.step()
            torch.cuda.synchronize()
            times[label].append((time.perf_counter() - t0) / args.steps * 1e6)
    print(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; {len(base)} tensors, {numel} floats "
          f"({numel * 4 / 1e6:.1f} MB per array); {args.windows} alternating windows of {args.steps} steps per candidate, "
          "host clock around a window that ends in a device synchronise")
    print(f"{'candidate':48s} {'median us/step':>14s} {'min':>8s} {'max':>8s} {'kernels/step':>13s} {'B/param':>8s} {'GB/s at median':>15s}")
    for label, opt, bpp, note in cands:
        if opt is None:
            print(f"{label:48s} {note}")
            continue
        t = times[label]
        med = statistics.median(t)
        print(f"{label:48s} {med:14.1f} {min(t):8.1f} {max(t):8.1f} {launches(opt.step):13d} {bpp:8d} {numel * bpp / med / 1e3:15.0f}",
              flush=True)
    print("GB/s: the bytes the update rule needs (B/param x floats) over the median step time, host overhead included; a step "
          "of this size is launch- and latency-bound, so the time is the headline, not a share of peak bandwidth")


if __name__ == "__main__":
    main()
