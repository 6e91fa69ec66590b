#!/usr/bin/env python3
"""The tail of a train step alone: from the three heads' batch-8 logits to their three gradients, including what the trainer
reads back — two forms, alternating in one process:

  (a) the stock sequence of bench.py:726-732: three torch.nn.CrossEntropyLoss calls, the two .item() reads of the reference
      (kfold_train_adversarial.py:127-128), the sum, backward;
  (b) losses.AdversarialCriterion + metrics.TrainMetrics.update, the sum, backward: nothing is read back, the losses stay
      on the device until the epoch's compute().

Per form: device kernels per call (torch.profiler, one call, in a pass of its own) and, over --windows alternating windows
of --reps calls, the median and the minimum time per call in microseconds — host clock around a window that ends in a
device synchronise, so the idle time around the host reads of (a) is inside the span.  The spread between the windows of
one form is printed: a difference between the forms below it is no difference.

    python tools/tail_time.py [--reps 200] [--windows 7] [--batch 8]
"""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from transmf_ad_amd import losses as L          # noqa: E402
from transmf_ad_amd import metrics as M         # noqa: E402

DEV = torch.device("cuda")


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tail_time.py needs a GPU")
    B = args.batch
    torch.manual_seed(0)
    lo = torch.randn(B, 2, device=DEV, requires_grad=True)
    dm = torch.randn(B, 2, device=DEV, requires_grad=True)
    dp = torch.randn(B, 2, device=DEV, requires_grad=True)
    label = torch.randint(0, 2, (B,), device=DEV)
    ones, zeros = torch.ones_like(label), torch.zeros_like(label)
    crit = torch.nn.CrossEntropyLoss()
    ours, tm = L.AdversarialCriterion(), M.TrainMetrics()
    assert L.adversarial_kernel_ok(lo, dm, dp, label)

    def stock():
        lo.grad = dm.grad = dp.grad = None
        ce_loss = crit(lo, label)
        ad_loss = (crit(dm, ones) + crit(dp, zeros)) / 2
        ce_loss.item()
        ad_loss.item()
        loss = ad_loss + ce_loss
        loss.backward()

    def fused():
        lo.grad = dm.grad = dp.grad = None
        ce_loss, ad_loss = ours(lo, dm, dp, label)
        tm.update(ce_loss, ad_loss, lo, dm, dp, label)
        loss = ad_loss + ce_loss
        loss.backward()

    forms = (("(a) stock CE x3 + two .item()", stock), ("(b) AdversarialCriterion + TrainMetrics", fused))
    for _name, fn in forms:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    counts = [launches(fn) for _name, fn in forms]
    times = [[], []]
    for _w in range(args.windows):
        for k, (_name, fn) in enumerate(forms):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _i in range(args.reps):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / args.reps * 1e6)
    print(f"device: {torch.cuda.get_device_name(0)}; batch {B}; logits -> three logit gradients; {args.windows} alternating "
          f"windows of {args.reps} calls, host clock, us per call")
    print(f"{'form':44s} {'kernels':>8s} {'median us':>10s} {'min us':>8s} {'max us':>8s}")
    for (name, _fn), n, t in zip(forms, counts, times):
        print(f"{name:44s} {n:8d} {statistics.median(t):10.1f} {min(t):8.1f} {max(t):8.1f}")
    spread = max(max(t) - min(t) for t in times)
    gain = statistics.median(times[0]) - statistics.median(times[1])
    print(f"median (a) - median (b) = {gain:.1f} us; largest spread between the windows of one form = {spread:.1f} us")
    print(f"epoch read-back of (b): {tm.compute()}")


if __name__ == "__main__":
    main()
