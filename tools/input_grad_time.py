"""Time and peak memory of the input-volume gradient (d score / d volume, parameters frozen) on the GPU.

    python tools/input_grad_time.py [--batch 8 --size 96 --dim 128 --iters 10 --warmup 3] [--tree DIR]

Cases: model_ad in eval mode and in train mode (two volumes), one sNet in train mode.  One timed item is the whole thing a
saliency call costs: forward with a graph on the volumes, the score, torch.autograd.grad back to the volumes - between two device
events, median over --iters after --warmup; the peak is torch.cuda.max_memory_allocated over the timed iterations.  The script
uses nothing newer than the model classes and autograd, so the same file runs on an older tree (--tree: import the package from
there), where the first block's data gradient goes through the generic route that writes the conv output.  One JSON line per
case.

    python tools/input_grad_time.py --kernel [--channels 32]      tmf_c1_bwd_dgrad alone, direct calls, c1_split 1 / 0 x train / eval
    python tools/input_grad_time.py --table a.jsonl [b.jsonl ...]  the JSON lines of such runs as the table of
                                                                   profiles/input_grad_mi355x.txt (no GPU needed)"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--label", default="")
    ap.add_argument("--kernel", action="store_true", help="time tmf_c1_bwd_dgrad alone (direct calls) instead of the models")
    ap.add_argument("--channels", type=int, default=32, help="--kernel: channels of the first block (dim / 4)")
    ap.add_argument("--table", nargs="+", metavar="JSONL", help="format the JSON lines of earlier runs, in file order")
    args = ap.parse_args()
    if args.table:
        return table(args.table)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("input_grad_time.py measures on the GPU; none found")
    import transmf_ad_amd as T
    dev = "cuda:0"
    B, S = args.batch, args.size
    if args.kernel:
        return kernel_alone(torch, T, args, dev)
    g = torch.Generator().manual_seed(1)
    vols = [torch.randn((B, 1, S, S, S), generator=g).to(dev) for _ in range(2)]

    def freeze(m):
        for p in m.parameters():
            p.requires_grad_(False)
        return m

    def model_ad(train):
        torch.manual_seed(2)
        m = freeze(T.model_ad(dim=args.dim, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.0).to(dev))
        m.train(train)

        def run():
            leaves = [v.detach().requires_grad_(True) for v in vols]
            logits = m(*leaves)[0]
            return torch.autograd.grad(logits[:, 1].sum(), leaves)
        return run

    def snet():
        torch.manual_seed(3)
        m = freeze(T.sNet(args.dim).to(dev)).train()
        R = torch.randn((B, args.dim, 1, 1, 1), generator=g).to(dev)

        def run():
            leaf = vols[0].detach().requires_grad_(True)
            return torch.autograd.grad((m(leaf) * R).sum(), [leaf])
        return run

    for name, make in (("model_ad eval", lambda: model_ad(False)), ("model_ad train", lambda: model_ad(True)), ("sNet train", snet)):
        run = make()
        for _ in range(args.warmup):
            out = run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(args.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = run()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        ok = all(bool(torch.isfinite(o).all()) for o in out)
        print(json.dumps(dict(label=args.label, case=name, batch=B, size=S, dim=args.dim, median_ms=round(times[len(times) // 2], 3),
                              min_ms=round(times[0], 3), max_ms=round(times[-1], 3), iters=args.iters,
                              peak_mib=round(torch.cuda.max_memory_allocated() / 2 ** 20, 1), finite=ok,
                              grad_abs_sum=float(sum(o.double().abs().sum() for o in out)))), flush=True)
        del run, out
        torch.cuda.empty_cache()


def kernel_alone(torch, T, args, dev):
    """tmf_c1_bwd_dgrad on random data, B x size^3 x channels: train = non-zero coef (the BatchNorm stencil runs), eval = zero coef."""
    from transmf_ad_amd import _lib
    B, S, C = args.batch, args.size, args.channels
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, S, S, S), generator=g).to(dev)
    w = (0.2 * torch.randn((27, C), generator=g)).to(dev)
    scale, shift = (0.5 + torch.rand(C, generator=g)).to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    mean, invstd = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dpool = torch.randn((B, S // 2, S // 2, S // 2, C), generator=g).to(dev)
    dx = torch.empty_like(x)
    nb = _lib.query("tmf_c1_bwd_dgrad_workspace_bytes", B, S, S, S, C)
    ws = torch.empty(max(nb, 16) // 4, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    try:
        for split in (1, 0):
            _lib.call("tmf_set_option", b"c1_split", split)
            for mode, coef in (("train", (1e-3 * torch.randn((2, C), generator=g)).to(dev)), ("eval", torch.zeros((2, C), device=dev))):
                def run():
                    _lib.call("tmf_c1_bwd_dgrad", x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                              invstd.data_ptr(), coef.data_ptr(), dpool.data_ptr(), dx.data_ptr(), ws.data_ptr(), nb, B, S, S, S, C, 0.01, st)
                for _ in range(args.warmup):
                    run()
                torch.cuda.synchronize()
                times = []
                for _ in range(args.iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
                times.sort()
                print(json.dumps(dict(label=args.label, kernel="tmf_c1_bwd_dgrad", c1_split=split, mode=mode, batch=B, size=S, channels=C,
                                      median_ms=round(times[len(times) // 2], 4), min_ms=round(times[0], 4), max_ms=round(times[-1], 4),
                                      iters=args.iters, finite=bool(torch.isfinite(dx).all()))), flush=True)
    finally:
        _lib.call("tmf_set_option", b"c1_split", 1)


def table(paths):
    rows = [json.loads(line) for p in paths for line in open(p) if line.strip().startswith("{")]
    cases = [r for r in rows if "case" in r]
    if cases:
        print("  case              tree     run  median ms   min ms   max ms   peak MiB   sum |gradient|")
        seen = {}
        for r in cases:
            key = (r["case"], r["label"])
            seen[key] = seen.get(key, 0) + 1
            print(f"  {r['case']:<16}  {r['label']:<7}  {seen[key]:>3}  {r['median_ms']:>9.3f}  {r['min_ms']:>7.3f}  {r['max_ms']:>7.3f}  "
                  f"{r['peak_mib']:>9.1f}   {r['grad_abs_sum']:.6e}")
        print()
        for case in dict.fromkeys(r["case"] for r in cases):
            for label in dict.fromkeys(r["label"] for r in cases):
                sel = [r for r in cases if r["case"] == case and r["label"] == label]
                if sel:
                    print(f"  {case:<16}  {label:<7}  medians {min(r['median_ms'] for r in sel):.3f} .. {max(r['median_ms'] for r in sel):.3f} ms, "
                          f"iterations {min(r['min_ms'] for r in sel):.3f} .. {max(r['max_ms'] for r in sel):.3f} ms, peak {sel[0]['peak_mib']:.0f} MiB")
        print()
    for r in rows:
        if "kernel" in r:
            print(f"  {r['kernel']}  {r['label']:<7}  B = {r['batch']}, {r['size']}^3, C = {r['channels']}  c1_split {r['c1_split']}  {r['mode']:<5}  "
                  f"median {r['median_ms']:.3f} ms  (min {r['min_ms']:.3f}, max {r['max_ms']:.3f})")


if __name__ == "__main__":
    main()
