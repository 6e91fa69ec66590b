#!/usr/bin/env python3
"""Golden fixtures for FALoss and SupConLoss: the reference's models/losses.py run in fp64 and in fp32 on the inputs of
tests/_loss_inputs.py.  Per case: the seeds and shape (`meta`), the fp64 and fp32 loss, make_golden.gprobe of every input
gradient in fp64 and fp32 and, for SupConLoss, the full fp64 gradient and the reference's own fp32-versus-fp64 distances
(`ref_loss_err` absolute, `ref_grad_err` relative to the largest fp64 gradient entry).  Data only.  Usage:

    python tests/golden/make_golden_losses.py [case ...]      # default: all cases
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_golden import gprobe  # noqa: E402  (also puts the reference on sys.path)
import _loss_inputs as LI  # noqa: E402


def run_fa(name):
    from models.losses import FALoss
    B, C, spatial = LI.FA_CASES[name]
    a, b = LI.fa_inputs(B, C, spatial)
    out = {"meta": dict(kind="faloss", B=B, C=C, spatial=list(spatial), seed=LI.FA_SEED)}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        x = torch.from_numpy(a).to(dt).requires_grad_(True)
        y = torch.from_numpy(b).to(dt).requires_grad_(True)
        loss = FALoss()(x, y)
        loss.backward()
        out["loss" + tag] = np.float64(loss.item())
        out["g1_" + tag] = gprobe(x.grad)
        out["g2_" + tag] = gprobe(y.grad)
        del loss, x, y
    return out


def run_sc(name):
    from models.losses import SupConLoss
    bs, views, d, positives, mode, shape = LI.SC_CASES[name]
    f, labels, mask = LI.sc_inputs(bs, views, d, positives, shape)
    out = {"meta": dict(kind="supcon", bs=bs, views=views, d=d, positives=positives, contrast_mode=mode,
                        shape=list(shape) if shape else None, seed=LI.SC_SEED)}
    grads = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        x = torch.from_numpy(f).to(dt).requires_grad_(True)
        loss = SupConLoss(contrast_mode=mode)(x, labels=None if labels is None else torch.from_numpy(labels),
                                              mask=None if mask is None else torch.from_numpy(mask))
        loss.backward()
        out["loss" + tag] = np.float64(loss.item())
        out["g_" + tag] = gprobe(x.grad)
        grads[tag] = x.grad.double().numpy()
    out["grad64"] = grads["64"]
    out["ref_loss_err"] = np.float64(abs(out["loss32"] - out["loss64"]))
    out["ref_grad_err"] = np.float64(np.abs(grads["32"] - grads["64"]).max() / np.abs(grads["64"]).max())
    return out


def main(argv):
    names = argv or list(LI.FA_CASES) + list(LI.SC_CASES)
    for name in names:
        out = run_fa(name) if name in LI.FA_CASES else run_sc(name)
        out["meta"] = np.frombuffer(json.dumps(out["meta"]).encode(), dtype=np.uint8)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: loss64 {float(out['loss64']):.12g} loss32 {float(out['loss32']):.9g}  {os.path.getsize(path)} B", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
