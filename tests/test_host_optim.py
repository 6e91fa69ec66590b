"""optim.SGD / optim.getOptimizer / tmf_sgd_step without a GPU: the C-ABI binding and its argument checks (all of them host
code that runs before any device call), the drop-in surface of getOptimizer against what the reference's getOptimizer made
(tests/golden/optim_*.npz, tests/golden/make_golden_optim.py), the constructor's refusals and the register / scratch
budget of csrc/sgd.hip."""
import copy
import ctypes as C
import json
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _optim_inputs as OI

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def _arrays(n, numel=8, grads=True):
    """ctypes argument arrays over host memory (never dereferenced: the calls below are refused, or have nothing to do)"""
    store = (C.c_float * (n * numel))()
    base = C.addressof(store)
    ptrs = (C.c_void_p * n)(*[base + 4 * numel * i for i in range(n)])
    gptrs = (C.c_void_p * n)(*[(base + 4 * numel * i) if grads else None for i in range(n)])
    return store, ptrs, gptrs, (C.c_long * n)(*([numel] * n)), (C.c_int * n)(*([1] * n))


def test_sgd_step_is_bound_and_exported():
    from transmf_ad_amd import _lib
    assert "tmf_sgd_step" in _lib.PROTOTYPES
    assert hasattr(C.CDLL(_lib.LIB_PATH), "tmf_sgd_step")
    assert _lib.load().tmf_sgd_step.argtypes == _lib.PROTOTYPES["tmf_sgd_step"][1]


def test_sgd_step_argument_validation_without_gpu():
    from transmf_ad_amd import _lib
    store, p, g, numel, fresh = _arrays(3)
    buf = C.addressof(store)                    # 16-byte aligned or not, the refusals below come first
    with pytest.raises(_lib.TmfError, match="'params' is NULL"):
        _lib.call("tmf_sgd_step", 3, None, g, numel, None, None, 0.1, 0.0, 0.0, None)
    with pytest.raises(_lib.TmfError, match="'grads' is NULL"):
        _lib.call("tmf_sgd_step", 3, p, None, numel, None, None, 0.1, 0.0, 0.0, None)
    with pytest.raises(_lib.TmfError, match="'numel' is NULL"):
        _lib.call("tmf_sgd_step", 3, p, g, None, None, None, 0.1, 0.0, 0.0, None)
    for n in (0, _lib.ADAM_MAX_TENSORS + 1):
        with pytest.raises(_lib.TmfError, match=f"{n} tensors"):
            _lib.call("tmf_sgd_step", n, p, g, numel, None, None, 0.1, 0.0, 0.0, None)
    for lr, mom, wd, what in ((-0.1, 0.0, 0.0, "lr=-0.1"), (0.1, -0.5, 0.0, "momentum=-0.5"), (0.1, 0.0, -1e-3, "weight_decay=-0.001")):
        with pytest.raises(_lib.TmfError, match=what):
            _lib.call("tmf_sgd_step", 3, p, g, numel, buf, fresh, lr, mom, wd, None)
    with pytest.raises(_lib.TmfError, match="momentum=0.9 needs momentum_buf"):
        _lib.call("tmf_sgd_step", 3, p, g, numel, None, fresh, 0.1, 0.9, 0.0, None)
    with pytest.raises(_lib.TmfError, match="momentum=0.9 needs momentum_buf"):
        _lib.call("tmf_sgd_step", 3, p, g, numel, buf, None, 0.1, 0.9, 0.0, None)
    with pytest.raises(_lib.TmfError, match="not 16-byte aligned"):
        _lib.call("tmf_sgd_step", 3, p, g, numel, (buf & ~15) + 4, fresh, 0.1, 0.9, 0.0, None)
    big = (C.c_long * 3)(8, 1 << 31, 8)
    with pytest.raises(_lib.TmfError, match="tensor 1 has 2147483648 elements"):
        _lib.call("tmf_sgd_step", 3, p, g, big, None, None, 0.1, 0.0, 0.0, None)
    big = (C.c_long * 3)((1 << 31) - 8, (1 << 31) - 8, 8)
    with pytest.raises(_lib.TmfError, match="2\\^31 elements of optimizer state"):
        _lib.call("tmf_sgd_step", 3, p, g, big, None, None, 0.1, 0.0, 0.0, None)
    pn = (C.c_void_p * 3)(p[0], None, p[2])
    with pytest.raises(_lib.TmfError, match="parameter 1 is NULL"):
        _lib.call("tmf_sgd_step", 3, pn, g, numel, None, None, 0.1, 0.0, 0.0, None)


def test_sgd_step_without_any_gradient_is_a_no_op_without_gpu():
    """n tensors that all have a NULL gradient: nothing to launch, no device call, rc 0 — with and without momentum."""
    from transmf_ad_amd import _lib
    store, p, g, numel, fresh = _arrays(_lib.ADAM_MAX_TENSORS, grads=False)
    before = bytes(store)
    _lib.call("tmf_sgd_step", _lib.ADAM_MAX_TENSORS, p, g, numel, None, None, 0.1, 0.0, 1e-3, None)
    aligned = (C.addressof(store) + 15) & ~15
    _lib.call("tmf_sgd_step", _lib.ADAM_MAX_TENSORS, p, g, numel, aligned, fresh, 0.1, 0.9, 0.0, None)
    assert bytes(store) == before and list(fresh) == [1] * _lib.ADAM_MAX_TENSORS
    # the layout rule of the momentum buffer is the one of Adam's moments
    assert _lib.query("tmf_adam_state_elems", 4, (C.c_long * 4)(1, 5, 8, 2049)) == 4 + 8 + 8 + 2052


def _cpu_params():
    p0, _ = OI.initial_and_gradients(1)
    return [torch.nn.Parameter(torch.from_numpy(a)) for a in p0]


@pytest.mark.parametrize("name", ["optim_ref_sgd", "optim_ref_adam"])
def test_get_optimizer_builds_what_the_reference_builds(name):
    from transmf_ad_amd import optim
    z, meta = fixture(name)
    case = meta["case"]
    assert case == OI.CASES[name] and meta["seed"] == OI.SEED and [tuple(s) for s in meta["shapes"]] == OI.SHAPES
    params = _cpu_params()
    opt = SimpleNamespace(optimizer=case["optimizer"], lr=case["lr"], weight_decay=case["weight_decay"])
    got = optim.getOptimizer((p for p in params), opt)                 # a generator, as net.parameters() is
    assert isinstance(got, tuple) and len(got) == 2
    optimizer, scheduler = got
    assert type(optimizer) is {"SGD": optim.SGD, "Adam": optim.Adam}[case["optimizer"]]
    assert type(optimizer).__name__ == meta["optimizer_class"]
    assert isinstance(optimizer, torch.optim.Optimizer)
    assert [id(p) for p in optimizer.param_groups[0]["params"]] == [id(p) for p in params]
    keys = ("lr", "momentum", "weight_decay") if case["optimizer"] == "SGD" else ("lr", "betas", "eps", "weight_decay")
    for k in keys:
        want = meta["defaults"][k]
        have = optimizer.defaults[k]
        assert (list(have) if isinstance(have, tuple) else have) == want, k
    for k in set(optimizer.defaults) & set(meta["defaults"]):          # every key both have, the named ones included
        have = optimizer.defaults[k]
        assert (list(have) if isinstance(have, tuple) else have) == meta["defaults"][k], k
    assert type(scheduler) is torch.optim.lr_scheduler.MultiStepLR
    assert sorted(scheduler.milestones) == meta["milestones"] == case["milestones"] and scheduler.gamma == meta["gamma"]
    lrs = []
    for _ in range(case["steps"]):
        lrs.append(optimizer.param_groups[0]["lr"])
        scheduler.step()               # (torch warns that no optimizer.step() came first; the lr sequence is unaffected)
    assert lrs == list(z["lr"])        # exactly: the same scheduler arithmetic on the same numbers


def test_get_optimizer_returns_none_for_an_unknown_name():
    from transmf_ad_amd import optim
    for name in ("AdamW", "sgd", "", None):
        assert optim.getOptimizer(iter(_cpu_params()), SimpleNamespace(optimizer=name, lr=1e-3, weight_decay=0.0)) is None


def test_mnet_fixture_matches_its_inputs_file():
    z, meta = fixture("optim_mnet_sgd")
    assert meta["case"] == OI.CASES["optim_mnet_sgd"] and meta["defaults"]["momentum"] == 0.9
    assert meta["milestones"] == [6, 21] and meta["checkpoints"] == OI.checkpoints(30)
    assert z["ref_err"].shape == (4, len(OI.SHAPES)) and z["lr"].shape == (30,)
    assert z["lr"][5] == 1e-3 and z["lr"][6] < 1e-3 and z["lr"][21] < z["lr"][20]


def test_sgd_constructor_is_torchs_and_refuses_what_is_not_built():
    from transmf_ad_amd import optim
    o = optim.SGD(_cpu_params(), 0.05, 0.8, 0, 1e-3, False)             # torch's positional order
    assert o.defaults == dict(lr=0.05, momentum=0.8, dampening=0, weight_decay=1e-3, nesterov=False)
    o = optim.SGD(_cpu_params())
    assert (o.defaults["lr"], o.defaults["momentum"], o.defaults["weight_decay"]) == (1e-3, 0, 0)
    assert o.state_dict()["state"] == {}                                 # nothing is created before the first step
    for kw in (dict(dampening=0.1), dict(momentum=0.9, nesterov=True), dict(maximize=True), dict(foreach=True),
               dict(fused=True), dict(differentiable=True)):
        with pytest.raises(ValueError, match="torch.optim.SGD"):
            optim.SGD(_cpu_params(), lr=0.1, **kw)
    for kw in (dict(lr=-1.0), dict(momentum=-0.1), dict(weight_decay=-1e-3)):
        with pytest.raises(ValueError):
            optim.SGD(_cpu_params(), **kw)


def test_sgd_has_no_cpu_path_and_copies_without_a_device():
    from transmf_ad_amd import _lib, optim
    for kw in (dict(), dict(momentum=0.9)):
        params = _cpu_params()
        o = optim.SGD(params, lr=0.1, **kw)
        for p in params:
            p.grad = torch.ones_like(p)
        before = [p.detach().clone() for p in params]
        with pytest.raises(_lib.TmfError, match="on one HIP device"):
            o.step()
        assert all(torch.equal(a, b) for a, b in zip(before, params))   # refused, not computed some other way
        assert len(o.state) == 0
        for o2 in (copy.deepcopy(o), pickle.loads(pickle.dumps(o))):    # an optimizer that has not stepped copies on the host
            assert type(o2) is optim.SGD and len(o2.state) == 0
            assert {k: o2.defaults[k] for k in o.defaults} == o.defaults    # (torch's __setstate__ may add keys of its own)
    # a state dict of torch's own, taken before any step, loads as well
    o = optim.SGD(_cpu_params(), lr=0.1, momentum=0.9)
    o.load_state_dict(torch.optim.SGD(_cpu_params(), lr=0.2, momentum=0.5).state_dict())
    assert o.param_groups[0]["lr"] == 0.2 and o.param_groups[0]["momentum"] == 0.5


@pytest.fixture(scope="module")
def sgd_kernels():
    from tools import resources as R
    obj = os.path.join(R.CSRC, "sgd.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built (python -m transmf_ad_amd.build)")
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    return R.kernels_of(obj)


def test_sgd_kernels_have_no_scratch(sgd_kernels):
    ks = [k for k in sgd_kernels if "sgd_step_kernel" in k["name"]]
    assert len(ks) == 2                                   # with | without momentum
    for k in sgd_kernels:
        assert k.get("scratch", 0) == 0, k
        assert k["vgpr"] <= 64, k                         # an element-wise kernel: nothing may limit its occupancy
