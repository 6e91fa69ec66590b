#!/usr/bin/env python3
"""The fusion block under torch.no_grad() — val_step (kfold_train_adversarial.py:144-161), the test run after training
(:229-250), bench.py --eval — two routes, alternating in one process by flipping ops.FUSION_INFER_ONE_CALL:

  old  the block walks its Transformer modules: per instance seven launches and the separate "+ tokens" add, then the pool;
  new  ops.fusion_infer: ONE library call that keeps nothing (tmf_fusion_infer_fwd).

Cases: (a) the block alone at B = 8, N = 216, dim 128, depth 3, heads 4 x 32 and 8 x 16 (the fused per-instance kernels);
(b) the same at dim 64 and 256 (one launch per op); (c) model_ad's whole eval forward at B = 8, 96^3.

Per case and route: device kernels per call (torch.profiler, one call, in a pass of its own) and, after a warm-up of both
routes, --windows alternating windows of --reps calls timed with device events (us per call): every window, the median
and the spread of each route, and whether the new route is below the old one in EVERY window pair.

    python tools/fusion_infer_time.py [--reps 100] [--windows 7] [--skip-model]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import transmf_ad_amd as T                      # noqa: E402
from transmf_ad_amd import networks, ops        # noqa: E402

DEV = torch.device("cuda")


def launches(fn):
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA
               and not e.name.lower().startswith(("memcpy", "memset")))


def window(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def compare(title, fn, reps, windows):
    """fn() under both settings of the switch: kernel counts, alternating windows."""
    def route(on):
        def run():
            ops.FUSION_INFER_ONE_CALL = on
            with torch.no_grad():
                return fn()
        return run
    forms = (("old (module walk)", route(False)), ("new (one call)", route(True)))
    try:
        for _name, run in forms:
            for _ in range(10):
                run()
        torch.cuda.synchronize()
        out = [run().float() for _name, run in forms]
        torch.cuda.synchronize()
        counts = [launches(run) for _name, run in forms]
        times = [[], []]
        for _w in range(windows):
            for k, (_name, run) in enumerate(forms):
                times[k].append(window(run, reps))
    finally:
        ops.FUSION_INFER_ONE_CALL = True
    print(f"\n{title}")
    print(f"  {'route':20s} {'kernels':>8s} {'median us':>10s} {'min us':>9s} {'max us':>9s}   windows (us per call)")
    for (name, _run), n, t in zip(forms, counts, times):
        print(f"  {name:20s} {n:8d} {statistics.median(t):10.1f} {min(t):9.1f} {max(t):9.1f}   " + " ".join(f"{v:.1f}" for v in t))
    below = all(n < o for o, n in zip(*times))
    spread = max(max(t) - min(t) for t in times)
    print(f"  median old - median new = {statistics.median(times[0]) - statistics.median(times[1]):.1f} us; largest spread between "
          f"the windows of one route = {spread:.1f} us; new below old in every window: {'yes' if below else 'NO'}; "
          f"max |old - new| of the outputs = {(out[0] - out[1]).abs().max().item():.2e}")
    return below


def block_case(dim, heads, B, N, depth):
    torch.manual_seed(0)
    fz = networks.CrossTransformer_MOD_AVG(dim, depth, heads, dim // heads, 4 * dim, 0.).to(DEV).eval()
    mri, pet = torch.randn(B, N, dim, device=DEV), torch.randn(B, N, dim, device=DEV)
    return lambda: fz(mri, pet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--skip-model", action="store_true", help="leave out (c), the whole model_ad eval forward")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("fusion_infer_time.py needs a GPU")
    B, N, depth = 8, 216, 3
    print(f"device: {torch.cuda.get_device_name(0)}; fusion block under no_grad, B = {B}, N = {N}, depth = {depth}; {args.windows} "
          f"alternating windows of {args.reps} calls, device events")
    verdict = {}
    for tag, dim, heads in (("(a)", 128, 4), ("(a)", 128, 8), ("(b)", 64, 4), ("(b)", 256, 4)):
        title = f"{tag} fusion block alone, dim {dim}, heads {heads} x {dim // heads}"
        verdict[title] = compare(title, block_case(dim, heads, B, N, depth), args.reps, args.windows)
    if not args.skip_model:
        torch.manual_seed(0)
        net = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.).to(DEV).eval()
        mri, pet = torch.rand(B, 1, 96, 96, 96, device=DEV), torch.rand(B, 1, 96, 96, 96, device=DEV)
        title = f"(c) model_ad eval forward, B = {B}, 96^3, dim 128, heads 4 x 32 (logits compared)"
        verdict[title] = compare(title, lambda: net(mri, pet)[0], max(args.reps // 5, 5), args.windows)
    print("\nnew route below the old one in every alternating window:")
    for k, v in verdict.items():
        print(f"  {'yes' if v else 'NO '}  {k}")


if __name__ == "__main__":
    main()
