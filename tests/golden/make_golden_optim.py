#!/usr/bin/env python3
"""Golden fixtures for the optimizers: the reference's utils.getOptimizer (SGD and Adam with their MultiStepLR) and the
SGD + MultiStepLR pair kfold_train_Mnet.py:85-86 builds, run in fp64 and in fp32 on the inputs of tests/_optim_inputs.py with
the scheduler stepped after every optimizer step.  (kfold_train_Mnet.py itself needs monai and ignite to import, so its two
torch objects are built here with its arguments.)  Per case: `meta` (seed, shapes, hyper-parameters, the optimizer's class
name and `defaults`, milestones, gamma, checkpoints), `lr` (the group's learning rate at every step), the fp64 parameters
after each checkpoint (`p<step>_<tensor>`), the fp64 state after the last step (`momentum_buffer_<tensor>` or
`exp_avg_<tensor>` / `exp_avg_sq_<tensor>` / `adam_steps`) and `ref_err[checkpoint][tensor]`: the reference's OWN fp32 run
against its fp64 run, max|p32 - p64| / max|p64| of that tensor.  Data only.  Usage:

    python tests/golden/make_golden_optim.py [case ...]      # default: all cases
"""
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402,F401  (puts the reference on sys.path)
import _optim_inputs as OI  # noqa: E402


def make(case, params):
    if case["make"] == "getOptimizer":
        from utils.utils import getOptimizer
        opt = SimpleNamespace(optimizer=case["optimizer"], lr=case["lr"], weight_decay=case["weight_decay"])
        return getOptimizer((p for p in params), opt)
    optimizer = torch.optim.SGD(params, lr=case["lr"], momentum=case["momentum"])
    return optimizer, torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=case["milestones"], gamma=OI.GAMMA)


def run(case, dtype):
    p0, grads = OI.initial_and_gradients(case["steps"])
    params = [torch.nn.Parameter(torch.from_numpy(a).to(dtype)) for a in p0]
    optimizer, scheduler = make(case, params)
    lrs, saved = [], {}
    for s, row in enumerate(grads, start=1):
        for p, g in zip(params, row):
            p.grad = None if g is None else torch.from_numpy(g).to(dtype)
        lrs.append(optimizer.param_groups[0]["lr"])
        optimizer.step()
        scheduler.step()
        if s in OI.checkpoints(case["steps"]):
            saved[s] = [p.detach().double().numpy().copy() for p in params]
    return params, optimizer, scheduler, lrs, saved


def main(argv):
    for name in argv or list(OI.CASES):
        case = OI.CASES[name]
        p64, opt64, sched64, lrs, saved64 = run(case, torch.float64)
        _p32, _o32, _s32, lrs32, saved32 = run(case, torch.float32)
        assert lrs == lrs32
        assert list(sched64.milestones) == case["milestones"] and sched64.gamma == OI.GAMMA
        cps = OI.checkpoints(case["steps"])
        out = {"lr": np.asarray(lrs, dtype=np.float64),
               "ref_err": np.asarray([[np.abs(a32 - a64).max() / np.abs(a64).max() for a32, a64 in zip(saved32[s], saved64[s])]
                                      for s in cps])}
        for s in cps:
            for i, a in enumerate(saved64[s]):
                out[f"p{s}_{i}"] = a
        steps = []
        for i, p in enumerate(p64):
            st = opt64.state.get(p, {})
            for key in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
                if st.get(key) is not None:
                    out[f"{key}_{i}"] = st[key].double().numpy()
            if "step" in st:
                steps.append(float(st["step"]))
        if steps:
            out["adam_steps"] = np.asarray(steps)
        meta = dict(seed=OI.SEED, shapes=[list(s) for s in OI.SHAPES], case=case, optimizer_class=type(opt64).__name__,
                    defaults=opt64.defaults, milestones=sorted(sched64.milestones), gamma=sched64.gamma, checkpoints=cps,
                    no_grad=list(OI.NO_GRAD), torch=torch.__version__)
        out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: largest ref_err per checkpoint {cps}: {[float(f'{e:.2g}') for e in out['ref_err'].max(axis=1)]}  "
              f"{os.path.getsize(path)} B", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
