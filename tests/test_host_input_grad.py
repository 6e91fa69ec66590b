"""Host side of the input-gradient work (no GPU): the new entry points and their argument errors, the builders of
tests/_dgrad_inputs.py (exactness budget, ties, exclusions, recorded distances), and transmf_ad_amd.saliency on a CPU stub."""
import ctypes

import pytest
import torch
import torch.nn as nn

import _dgrad_inputs as di


# ---- the library's new symbols -----------------------------------------------------------------------------------------------
def test_new_symbols_are_bound_and_refuse_bad_arguments():
    """NULL pointers -> TMF_E_NULL, a short workspace -> TMF_E_WORKSPACE, a bad shape -> TMF_E_SHAPE; bf16 precision with dvol ->
    TMF_E_ARG.  No launch happens, so the pointers only have to be non-NULL."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    E_NULL, E_SHAPE, E_WORKSPACE, E_ARG = -1, -2, -4, -5
    p = 4096
    geo = (2, 6, 8, 10, 12)
    need = lib.tmf_c1_bwd_dgrad_workspace_bytes(*geo)
    assert need > 0 and lib.tmf_c1_bwd_dgrad_workspace_bytes(0, 6, 8, 10, 12) == 0
    ok = [p] * 10
    for i in range(10):
        args = list(ok)
        args[i] = None
        assert lib.tmf_c1_bwd_dgrad(*args, need, *geo, 0.01, None) == E_NULL, i
    assert lib.tmf_c1_bwd_dgrad(*ok, need - 1, *geo, 0.01, None) == E_WORKSPACE
    assert lib.tmf_c1_bwd_dgrad(*ok, need, 2, 0, 8, 10, 12, 0.01, None) == E_SHAPE
    # the one-pass backward that also hands out coef: coef is required, z_sel and arg go together
    fargs = [p] * 7 + [None, None] + [p] * 6
    bad = list(fargs)
    bad[13] = None
    assert lib.tmf_c1_bwd_fused_coef(*bad, 1 << 20, *geo, 0.01, 1, None) == E_NULL
    bad = list(fargs)
    bad[7] = p
    assert lib.tmf_c1_bwd_fused_coef(*bad, 1 << 20, *geo, 0.01, 1, None) == E_NULL
    # one call: bf16 precision has no input gradient
    desc = _lib.SnetDesc(B=1, D=16, H=16, W=16, dim=32, precision=1, storage_bf16=0, flags=0)
    g = _lib.SnetGrads()
    assert lib.tmf_snet_train_bwd_input(ctypes.byref(desc), p, p, 1 << 30, p, ctypes.byref(g), p, 1 << 30, None, p) == E_ARG
    desc.precision = 0
    assert lib.tmf_snet_train_bwd_input(ctypes.byref(desc), None, p, 1 << 30, p, ctypes.byref(g), p, 1 << 30, None, p) == E_NULL
    assert lib.tmf_snet_train_bwd(ctypes.byref(desc), None, p, 1 << 30, p, ctypes.byref(g), p, 1 << 30, None) == E_NULL


# ---- the builders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("shape", di.SHAPES + [di.EMPTY_POOL_SHAPE], ids=str)
def test_exact_family_budget_ties_and_restatement(shape, train):
    """Every dx element's sum of |terms| (as written, and factored through a, M, N) stays below 2^24 units of 1/16, the prepared
    coefficients are fp32 numbers, many windows tie, one channel has scale 0 - and the fp32 restatement equals fp64 exactly."""
    inp = di.exact_inputs(shape, train)                     # (asserts the budget itself)
    direct, factored = di.exact_budget(inp)
    assert direct < di.EXACT_LIMIT and factored < di.EXACT_LIMIT
    assert di.tie_share(inp) > 0.25
    assert int((inp["scale"] == 0).sum()) >= 1
    assert bool((inp["coef"] != 0).any()) == train
    r64, r32 = di.dx_ref(inp, di.EXACT_SLOPE), di.dx_ref(inp, di.EXACT_SLOPE, torch.float32)
    assert torch.equal(r32.double(), r64)
    assert torch.equal((r64 / di.EXACT_UNIT).round() * di.EXACT_UNIT, r64)


def test_factored_batchnorm_part_equals_the_formula():
    """dx = routed part - the a / M stencil (masked at the faces) and, in the interior, - (sum a + N stencil): the form the kernel
    evaluates, restated on the host in fp64 on an exact-family case."""
    shape = di.SHAPES[2]
    inp = di.exact_inputs(shape, True)
    B, D, H, W, C = shape
    a, M, N = di.bn_factors(inp)
    ref = di.dx_ref(inp, di.EXACT_SLOPE)
    nobn = dict(inp, coef=torch.zeros(2, C))
    routed = di.dx_ref(nobn, di.EXACT_SLOPE)
    x = torch.nn.functional.pad(inp["x"].double(), (2, 2, 2, 2, 2, 2))
    bn = torch.zeros_like(ref)
    for t in range(27):
        kd, kh, kw = t // 9, (t // 3) % 3, t % 3
        s = torch.full((B, D, H, W), float(a[t]), dtype=torch.float64)          # value at v, for every v of the volume
        for u in range(27):
            ud, uh, uw = u // 9 - 1, (u // 3) % 3 - 1, u % 3 - 1
            s += M[t, u] * x[:, 2 + ud:2 + ud + D, 2 + uh:2 + uh + H, 2 + uw:2 + uw + W]
        sp = torch.nn.functional.pad(s, (1, 1, 1, 1, 1, 1))                     # 0 outside the volume
        bn += sp[:, 2 - kd:2 - kd + D, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]    # v = u - t + 1
    assert torch.equal(routed - bn, ref)
    inner = a.sum() + sum(N[i, j, k] * x[:, i:i + D, j:j + H, k:k + W] for i in range(5) for j in range(5) for k in range(5))
    assert torch.equal((routed - inner)[:, 1:-1, 1:-1, 1:-1], ref[:, 1:-1, 1:-1, 1:-1])


@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("shape", di.SHAPES, ids=str)
def test_conditioning_family_exclusions_and_distances(shape, train):
    inp, excluded = di.cond_inputs(shape, train)
    assert excluded <= di.COND_MAX_EXCLUDED
    assert bool((inp["scale"] > 0).any()) and bool((inp["scale"] < 0).any())
    assert bool((inp["coef"] != 0).any()) == train
    now, rec = di.cond_restatement_distance(shape, train), di.COND_DISTANCE[(shape, train)]
    assert rec / 2 <= now <= rec * 2, f"{shape} train={train}: recorded {rec:.3e}, measured {now:.3e}"


# ---- saliency on a CPU stub --------------------------------------------------------------------------------------------------
class _Stub(nn.Module):
    """Two volumes -> (features, logits (B, 3)); raises on request."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(3)
        self.a = nn.Conv3d(1, 2, 3, padding=1)
        self.b = nn.Conv3d(1, 2, 3, padding=1)
        self.fc = nn.Linear(4, 3)
        self.fail = False

    def forward(self, u, v):
        if self.fail:
            raise RuntimeError("stub failure")
        f = torch.cat([torch.tanh(self.a(u)).mean((2, 3, 4)), torch.tanh(self.b(v)).mean((2, 3, 4))], 1)
        return f, self.fc(f)


def _vols():
    g = torch.Generator().manual_seed(5)
    return torch.randn(3, 1, 4, 5, 6, generator=g), torch.randn(3, 1, 4, 5, 6, generator=g)


def _plain_grads(model, vols, target, output=1):
    leaves = [v.clone().requires_grad_(True) for v in vols]
    logits = model(*leaves)[output]
    if target is None:
        target = logits.detach().argmax(1)
    return torch.autograd.grad(logits.gather(1, target.view(-1, 1)).sum(), leaves)


def test_saliency_is_exported():
    import transmf_ad_amd
    from transmf_ad_amd import saliency
    assert transmf_ad_amd.input_gradients is saliency.input_gradients
    assert transmf_ad_amd.integrated_gradients is saliency.integrated_gradients


@pytest.mark.parametrize("target", (None, 2, [0, 2, 1]))
def test_input_gradients_match_autograd(target):
    from transmf_ad_amd import input_gradients
    m, (u, v) = _Stub(), _vols()
    want = _plain_grads(m, (u, v), None if target is None else torch.as_tensor([target] * 3 if isinstance(target, int) else target))
    got = input_gradients(m, u, v, target=target, output=1)
    assert len(got) == 2 and all(torch.equal(g, w) and g.shape == x.shape for g, w, x in zip(got, want, (u, v)))
    assert not u.requires_grad and u.grad is None and all(not g.requires_grad for g in got)
    assert all(p.requires_grad and p.grad is None for p in m.parameters())
    # freeze=False: the same numbers, parameters untouched as well
    got2 = input_gradients(m, u, v, target=target, output=1, freeze=False)
    assert all(torch.equal(g, w) for g, w in zip(got2, want)) and all(p.grad is None for p in m.parameters())
    # output selection: output 0 is (B, 4) here, another tensor, another gradient
    g0 = input_gradients(m, u, v, target=1, output=0)
    w0 = _plain_grads(m, (u, v), torch.tensor([1, 1, 1]), output=0)
    assert all(torch.equal(g, w) for g, w in zip(g0, w0)) and not torch.equal(g0[0], got[0])


def test_saliency_leaves_inputs_that_carry_a_graph_alone():
    from transmf_ad_amd import input_gradients
    m, (u, v) = _Stub(), _vols()
    leaf = u.clone().requires_grad_(True)
    scaled = leaf * 2.0                                          # a non-leaf input
    got = input_gradients(m, scaled, v, target=0, output=1)
    want = _plain_grads(m, (scaled.detach(), v), torch.tensor([0, 0, 0]))
    assert torch.equal(got[0], want[0]) and leaf.grad is None and scaled.grad_fn is not None


def test_requires_grad_is_restored_after_an_exception():
    from transmf_ad_amd import input_gradients, integrated_gradients
    m, (u, v) = _Stub(), _vols()
    m.fc.bias.requires_grad_(False)                             # the caller's own frozen parameter stays frozen
    m.fail = True
    for fn in (input_gradients, integrated_gradients):
        with pytest.raises(RuntimeError, match="stub failure"):
            fn(m, u, v, output=1)
        assert [p.requires_grad for p in m.parameters()] == [True, True, True, True, True, False]


@pytest.mark.parametrize("steps", (1, 4))
def test_integrated_gradients_is_its_definition(steps):
    from transmf_ad_amd import input_gradients, integrated_gradients
    m, (u, v) = _Stub(), _vols()
    base = (0.5 * torch.ones_like(u), torch.zeros_like(v))
    target = m(u, v)[1].argmax(1)
    acc = [torch.zeros_like(u), torch.zeros_like(v)]
    for k in range(steps):
        al = (k + 0.5) / steps
        g = input_gradients(m, base[0] + al * (u - base[0]), base[1] + al * (v - base[1]), target=target, output=1)
        for a, gi in zip(acc, g):
            a += gi
    want = [(x - b) * (a / steps) for x, b, a in zip((u, v), base, acc)]
    got = integrated_gradients(m, u, v, baselines=base, steps=steps, output=1)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # default baseline: zeros; completeness holds roughly (midpoint rule) for a smooth stub
    got0 = integrated_gradients(m, u, v, steps=32, output=1)
    f1 = m(u, v)[1].gather(1, target.view(-1, 1)).sum()
    f0 = m(torch.zeros_like(u), torch.zeros_like(v))[1].gather(1, target.view(-1, 1)).sum()
    assert abs(float(sum(g.sum() for g in got0)) - float((f1 - f0).detach())) < 1e-3 * max(1.0, abs(float((f1 - f0).detach())))
    assert all(p.requires_grad and p.grad is None for p in m.parameters())


def test_bad_arguments_raise_value_error():
    from transmf_ad_amd import input_gradients, integrated_gradients
    m, (u, v) = _Stub(), _vols()
    for bad in (torch.tensor([0, 1]), torch.zeros(3, 1, dtype=torch.long), torch.tensor([0, 1, 3]), torch.tensor([0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            input_gradients(m, u, v, target=bad, output=1)
    for steps in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            integrated_gradients(m, u, v, steps=steps, output=1)
    with pytest.raises(ValueError):
        integrated_gradients(m, u, v, baselines=(torch.zeros_like(u),), output=1)
    with pytest.raises(ValueError):
        input_gradients(m)
    for output in (2, -3, 1.0):                                 # the stub returns two outputs
        with pytest.raises(ValueError):
            input_gradients(m, u, v, output=output)


# ---- the kernel's budget ---------------------------------------------------------------------------------------------------------
def test_dgrad_kernels_fit_two_workgroups_per_cu_without_scratch():
    """csrc/conv1_dgrad.hip states its budget: <= 256 registers, zero scratch, LDS for two workgroups per CU (read from the built
    code object, as tests/test_kernel_resources.py does)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from tools import resources as R
    assert os.path.exists(os.path.join(R.CSRC, "conv1_dgrad.o")), "conv1_dgrad.o is not built (python -m transmf_ad_amd.build)"
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    ks = [k for k in R.all_kernels()["conv1_dgrad.o"] if "c1_dgrad" in k["name"]]
    assert len(ks) == 3                                     # prepare, c1_split on, c1_split off
    for k in ks:
        assert k["vgpr"] <= 256 and k.get("scratch", 0) == 0 and k["lds"] <= 80 * 1024, k
