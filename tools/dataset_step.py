#!/usr/bin/env python3
"""What feeding the training step from a device-resident data set costs.

One process, one GPU, model_ad at the bench shape (batch 8, 96^3, dim 128, one-launch Adam, the reference's train_step with
its two loss.item() host syncs: kfold_train_adversarial.py:101-136).  Three feeds, timed for --steps steps each after
warm-up with a host clock around a final device synchronise, in the order A B C A so that the repeated A shows the spread:
  A  one fixed batch resident in HBM (bench.py's configuration)
  B  a DeviceDataset loader over --subjects synthetic subjects (one tmf_batch_augment launch per batch)
  C  DevicePrefetcher over the same subjects held as host arrays
Then the batch-augment kernel alone (device events around next(); achieved bytes/s counted as read-once + write-once
bytes of the batch over that time) and the one-time cost of DeviceDataset.from_nifti on --subjects written .nii.gz pairs.

    python tools/dataset_step.py [--steps 200] [--warmup 10] [--subjects 64] [--size 96] [--batch 8]
"""
import argparse
import itertools
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--subjects", type=int, default=64)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dim", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dataset_step.py measures on a HIP device; none is available")
    import transmf_ad_amd as T
    from transmf_ad_amd.optim import Adam

    dev = torch.device("cuda:0")
    B, S, N = args.batch, args.size, args.subjects
    vol = (S, S, S)
    rs = np.random.RandomState(1234)
    mri = (rs.rand(N, 1, *vol) * 4000.0).astype(np.float32)          # raw intensities, as bench.py --from-host
    pet = (rs.rand(N, 1, *vol) * 9.0).astype(np.float32)
    labels = (np.arange(N) % 2).astype(np.int64)

    torch.manual_seed(0)
    net = T.model_ad(dim=args.dim, depth=3, heads=4, dim_head=args.dim // 4, mlp_dim=4 * args.dim, dropout=0.0).to(dev).train()
    opt = Adam(net.parameters(), lr=1e-4)
    crit = torch.nn.CrossEntropyLoss()
    ones = torch.ones(B, dtype=torch.int64, device=dev)
    zeros = torch.zeros(B, dtype=torch.int64, device=dev)

    def train_step(batch):
        opt.zero_grad()
        lo, dm, dp = net(batch["MRI"], batch["PET"])
        ce_loss = crit(lo, batch["label"])
        ad_loss = (crit(dm, ones) + crit(dp, zeros)) / 2
        ce_loss.item()
        ad_loss.item()
        (ad_loss + ce_loss).backward()
        opt.step()

    t0 = time.perf_counter()
    ds = T.DeviceDataset.from_arrays(mri, pet, labels, dev)
    torch.cuda.synchronize()
    print(f"DeviceDataset.from_arrays: {N} subjects of {vol} in {time.perf_counter() - t0:.2f} s "
          f"({2 * N * S ** 3 * 4 / 1e9:.2f} GB resident)")

    def epochs(loader):                           # epoch after epoch
        while True:
            yield from loader

    fixed = next(iter(ds.loader(batch_size=B, train=False)))
    host = [dict(MRI=mri[s:s + B], PET=pet[s:s + B], label=labels[s:s + B]) for s in range(0, N - B + 1, B)]
    feeds = {
        "A": lambda: itertools.repeat(fixed),
        "B": lambda: epochs(ds.loader(batch_size=B, seed=0)),
        "C": lambda: iter(T.DevicePrefetcher(itertools.cycle(host), device=dev, seed=0)),
    }
    names = {"A": "one fixed resident batch", "B": "DeviceDataset loader", "C": "DevicePrefetcher from host arrays"}
    rates = []
    for key in ("A", "B", "C", "A"):
        feed = feeds[key]()
        for _ in range(args.warmup):
            train_step(next(feed))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            train_step(next(feed))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if hasattr(feed, "close"):
            feed.close()
        rates.append((key, B * args.steps / dt))
        print(f"feed {key} ({names[key]}): {args.steps} steps, {1e3 * dt / args.steps:.3f} ms/step, "
              f"{B * args.steps / dt:.1f} pairs/s", flush=True)
    a1, b, _c, a2 = (r for _k, r in rates)
    spread = abs(a1 - a2)
    print(f"A-A spread {spread:.1f} pairs/s ({100 * spread / max(a1, a2):.2f} %); B - mean(A) = {b - (a1 + a2) / 2:+.1f} pairs/s "
          f"({100 * (b - (a1 + a2) / 2) / ((a1 + a2) / 2):+.2f} %)")

    # the kernel alone: device events around next()
    feed = epochs(ds.loader(batch_size=B, seed=1))
    for _ in range(5):
        next(feed)
    torch.cuda.synchronize()
    n = 50
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        next(feed)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    med = ms[n // 2]
    nbytes = 2 * 2 * B * S ** 3 * 4              # both modalities, each voxel read once and written once
    print(f"tmf_batch_augment (batch {B}, {vol}): median {med:.4f} ms, min {ms[0]:.4f} ms over {n} calls; "
          f"{nbytes / 1e6:.1f} MB read-once + write-once -> {nbytes / (med * 1e-3) / 1e12:.3f} TB/s at the median")

    # one-time cost of building the data set from files
    with tempfile.TemporaryDirectory() as td:
        mp, pp = [], []
        for k in range(N):
            mp.append(os.path.join(td, f"m{k}.nii.gz"))
            pp.append(os.path.join(td, f"p{k}.nii.gz"))
            T.write_nifti(mp[-1], mri[k, 0])
            T.write_nifti(pp[-1], pet[k, 0])
        size = sum(os.path.getsize(p) for p in mp + pp)
        t0 = time.perf_counter()
        ds2 = T.DeviceDataset.from_nifti(mp, pp, labels, dev)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    same = torch.equal(ds2.mri, ds.mri) and torch.equal(ds2.pet, ds.pet)
    print(f"DeviceDataset.from_nifti: {2 * N} .nii.gz files ({size / 1e6:.0f} MB on disk) in {dt:.2f} s "
          f"({1e3 * dt / (2 * N):.1f} ms per file); equal to from_arrays: {same}")


if __name__ == "__main__":
    main()
