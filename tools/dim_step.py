#!/usr/bin/env python3
"""Train step of model_ad(dim = 64 / 128 / 256, depth 3, 4 heads of dim / 4, mlp 4 dim) at B = 8, 96^3, fp32 — the
reference's step (kfold_train_adversarial.py:119-131: forward, CE + adversarial CE, the two loss.item() host syncs, backward,
Adam) — with the fusion block on each of its three paths:

    one_call       default: the whole fusion block is one library call per pass (ops.FusionTrain)
    per_block      TMF_FUSION_C=0: one ops.TransformerLayer per Transformer, Linears on the token GEMMs
    torch_linear   TMF_FUSE_TOKENS=0: both predicates off — nn.Linear (hipBLASLt / rocBLAS), torch GELU and adds

Every (dim, setting) runs as a fresh child process under its own `timeout`, the settings in alternating order per round;
each child prints one JSON line (ms per step, pairs/s, the path its fusion block took, its F.linear calls per step).

    python tools/dim_step.py [--dims 64 256] [--rounds 2] [--steps 30] [--warmup 10] [--dropout P]

--dropout P builds the model with the fusion block's Dropout at P (options/option.py:39); the default 0 is the
dropout-free step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"one_call": {}, "per_block": {"TMF_FUSION_C": "0"}, "torch_linear": {"TMF_FUSE_TOKENS": "0"}}


def child(args):
    import torch
    import torch.nn.functional as F
    sys.path.insert(0, ROOT)
    import transmf_ad_amd as T
    from transmf_ad_amd.optim import Adam

    B, dim, dev = args.batch, args.dim, "cuda"
    torch.manual_seed(0)
    net = T.model_ad(dim=dim, depth=3, heads=4, dim_head=dim // 4, mlp_dim=4 * dim, dropout=args.dropout).to(dev).train()
    opt = Adam(net.parameters(), lr=1e-4)
    mri, pet = torch.rand(B, 1, 96, 96, 96, device=dev), torch.rand(B, 1, 96, 96, 96, device=dev)
    y = torch.arange(B, device=dev) % 2
    ones, zeros = torch.ones_like(y), torch.zeros_like(y)
    crit = torch.nn.CrossEntropyLoss()
    seen = {}

    def step():
        opt.zero_grad()
        lo, dm, dp = net(mri, pet)
        seen["logits"] = lo
        ce, ad = crit(lo, y), (crit(dm, ones) + crit(dp, zeros)) / 2
        ce.item()
        ad.item()
        (ad + ce).backward()
        opt.step()

    n_lin = [0]
    real = F.linear

    def counted(*a, **k):
        n_lin[0] += 1
        return real(*a, **k)
    torch.nn.functional.linear = counted
    step()
    torch.nn.functional.linear = real
    names, todo, done = set(), [seen["logits"].grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in done:
            continue
        done.add(fn)
        names.add(type(fn).__name__)
        todo.extend(nf for nf, _ in fn.next_functions)
    path = ("one_call" if "FusionTrainBackward" in names else
            "per_block" if "TransformerLayerBackward" in names else "torch_linear")
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps(dict(dim=dim, setting=args.setting, ms_per_step=round(ms, 3), pairs_per_s=round(B / ms * 1e3, 1),
                          path=path, f_linear_calls_per_step=n_lin[0], steps=args.steps, batch=B, dropout=args.dropout)),
          flush=True)


def parent(args):
    rows = []
    order = list(SETTINGS)
    for r in range(args.rounds):
        for dim in args.dims:
            for s in (order if r % 2 == 0 else order[::-1]):
                env = dict(os.environ, **SETTINGS[s])
                cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child",
                       "--dim", str(dim), "--setting", s, "--steps", str(args.steps), "--warmup", str(args.warmup),
                       "--batch", str(args.batch), "--dropout", str(args.dropout)]
                p = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True)
                if p.returncode != 0:
                    sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                    print(f"dim {dim} {s}: exit status {p.returncode}; stopping", flush=True)
                    return 1
                row = json.loads(p.stdout.strip().splitlines()[-1])
                row["round"] = r
                rows.append(row)
                print(json.dumps(row), flush=True)
    print("\nsummary (median over rounds):")
    for dim in args.dims:
        for s in order:
            ms = [x["ms_per_step"] for x in rows if x["dim"] == dim and x["setting"] == s]
            print(f"  dim {dim:3d}  {s:12s}  {statistics.median(ms):8.2f} ms/step  {args.batch / statistics.median(ms) * 1e3:7.1f} "
                  f"pairs/s  (runs: {', '.join(f'{v:.2f}' for v in ms)})")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dropout", type=float, default=0.0, help="the fusion block's Dropout p (0: off)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--dim", type=int)
    ap.add_argument("--setting", choices=list(SETTINGS))
    a = ap.parse_args()
    if a.child:
        child(a)
    else:
        sys.exit(parent(a))
