"""Inputs of the optimizer fixtures (tests/golden/optim_*.npz), reproducible from one integer.  Shared by
tests/golden/make_golden_optim.py and the tests: the parameter tensors, one gradient per tensor per step and the rule for
the parameter that sits a step out."""
import numpy as np

SEED = 1234
# the last shape crosses a 2048-element workgroup chunk by one element and exercises the scalar tail
SHAPES = [(8, 4, 3, 3, 3), (8,), (16, 8), (5,), (1,), (2049,)]
NO_GRAD = (3, 3)                  # (tensor, step, counted from 1): tensor 3 has no gradient in step 3
CHECKPOINTS = (1, 4, 11)          # steps after which the parameters are recorded, besides the last one

# name: steps, how the optimizer is made, its hyper-parameters, the scheduler's milestones
CASES = {
    "optim_ref_sgd":  dict(steps=30, make="getOptimizer", optimizer="SGD", lr=1e-2, weight_decay=1e-3, milestones=[10, 26]),
    "optim_ref_adam": dict(steps=40, make="getOptimizer", optimizer="Adam", lr=1e-3, weight_decay=1e-3, milestones=[25, 36]),
    "optim_mnet_sgd": dict(steps=30, make="SGD", optimizer="SGD", lr=1e-3, momentum=0.9, milestones=[6, 21]),
}
GAMMA = 0.1


def checkpoints(steps):
    return list(CHECKPOINTS) + [steps]


def initial_and_gradients(steps, seed=SEED):
    """(initial parameters, grads): float32 arrays; grads[s][i] is tensor i's gradient in step s + 1, or None."""
    rs = np.random.RandomState(seed)
    params = [(0.1 * rs.standard_normal(s)).astype(np.float32) for s in SHAPES]
    grads = []
    for step in range(1, steps + 1):
        row = [rs.standard_normal(s).astype(np.float32) for s in SHAPES]      # drawn for every tensor: the stream does not
        if step == NO_GRAD[1]:                                               # depend on the rule below
            row[NO_GRAD[0]] = None
        grads.append(row)
    return params, grads
