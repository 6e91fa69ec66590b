"""The fusion block at the reference's other `--dim` settings (options/option.py:36): dim 64 and 256, in both head
geometries of its drivers (4 heads of dim / 4: kfold_train_adversarial.py:78-79; 8 heads of dim / 8:
train_adversarial.py:30-31), mlp = 4 dim.  Kernel level (csrc/token_gemm.hip's 64- and 256-column tiles and its
LayerNorm prologue / LayerNorm-backward epilogue at K = 64 and 256), module level (Transformer on the token GEMMs against
the fp64 formula), the one-call fusion entry against the per-Transformer path, and golden train steps from the
reference.  No torch nn.Linear anywhere on these paths."""
import ctypes
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _golden import Golden
from test_gpu_kernels import _gelu64, _rand, _relerr, _transformer64_live
from test_gpu_model import DEV, TOL, _golden_train_step, build, step

pytestmark = pytest.mark.gpu

GEOMETRIES = [(64, 4), (64, 8), (256, 4), (256, 8)]
MID = {(64, 4): "ad_d64_mid", (64, 8): "ad_d64_h8_mid", (256, 4): "ad_d256_mid", (256, 8): "ad_d256_h8_mid"}
GOLDEN = list(MID.values()) + ["ad_d64_full_b2", "ad_d256_full_b2"]


@pytest.fixture
def linear_calls(monkeypatch):
    """Counts torch.nn.functional.linear calls on device tensors (every nn.Linear forward goes through it; the fp64
    oracle the golden checks evaluate on the host is not counted)."""
    n = [0]
    real = F.linear

    def counted(x, *a, **k):
        n[0] += int(x.is_cuda)
        return real(x, *a, **k)
    monkeypatch.setattr(torch.nn.functional, "linear", counted)
    return n


def _ops():
    from transmf_ad_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# kernel level
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1731, 50])
@pytest.mark.parametrize("nout", [64, 256, 1024])
@pytest.mark.parametrize("K", [64, 256])
def test_tok_linear_fwd_layernorm_prologue(K, nout, R):
    ops = _ops()
    x = _rand(R, K, seed=201) * 2 + 0.5
    w = _rand(nout, K, seed=202, scale=K ** -0.5)
    b = _rand(nout, seed=203, scale=0.1)
    g, be = 1 + _rand(K, seed=204, scale=0.1), _rand(K, seed=205, scale=0.1)
    xd, wd = x.double(), w.double()
    ln = F.layer_norm(xd, (K,), g.double(), be.double(), 1e-5)
    y, (mean, rstd, a), _ = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), ln=(g.to(DEV), be.to(DEV), 1e-5), keep_ln_out=True)
    torch.cuda.synchronize()
    assert _relerr(a.cpu(), ln) < 2e-5 and _relerr(y.cpu(), ln @ wd.t()) < 2e-5
    assert _relerr(mean.cpu(), xd.mean(1)) < 2e-5
    assert _relerr(rstd.cpu(), (xd.var(1, unbiased=False) + 1e-5).rsqrt()) < 2e-5
    y, _, pre = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), bias=b.to(DEV), ln=(g.to(DEV), be.to(DEV), 1e-5), gelu=True)
    torch.cuda.synchronize()
    h = ln @ wd.t() + b.double()
    assert _relerr(pre.cpu(), h) < 2e-5 and _relerr(y.cpu(), _gelu64(h)) < 2e-5


@pytest.mark.parametrize("R", [1731, 50])
@pytest.mark.parametrize("K,nout", [(256, 64), (64, 64), (1024, 64), (16, 192)])
def test_tok_linear_fwd_64_column_tiles(K, nout, R):
    """Output widths that are multiples of 64 but not of 128, without the LayerNorm prologue: + bias + residual, GELU."""
    ops = _ops()
    x, w = _rand(R, K, seed=211), _rand(nout, K, seed=212, scale=K ** -0.5)
    b, res = _rand(nout, seed=213, scale=0.1), _rand(R, nout, seed=214)
    xd, wd = x.double(), w.double()
    y, _, _ = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), bias=b.to(DEV), residual=res.to(DEV))
    torch.cuda.synchronize()
    assert _relerr(y.cpu(), xd @ wd.t() + b.double() + res.double()) < 2e-5
    y, _, pre = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), bias=b.to(DEV), gelu=True)
    torch.cuda.synchronize()
    h = xd @ wd.t() + b.double()
    assert _relerr(pre.cpu(), h) < 2e-5 and _relerr(y.cpu(), _gelu64(h)) < 2e-5


@pytest.mark.parametrize("R", [1731, 50])
@pytest.mark.parametrize("nmul", [1, 4])
@pytest.mark.parametrize("K", [64, 256])
def test_tok_linear_bwd_input_epilogues(K, nmul, R):
    """dx = E(dy . w) with w [Nout][K]: the LayerNorm-backward epilogue (a K-wide tile) with two residual gradients, the
    dgamma | dbeta partials at {0..K-1 | K..2K-1} and the bias column sums of dy; the GELU-gradient and plain epilogues."""
    ops = _ops()
    from transmf_ad_amd import _lib as lib
    nout = nmul * K
    nblk = lib.query("tmf_tok_row_blocks", R)
    dy = _rand(R, nout, seed=221)
    w = _rand(nout, K, seed=222, scale=nout ** -0.5)
    add1, add2 = _rand(R, K, seed=223), _rand(R, K, seed=224)
    x = _rand(R, K, seed=225) * 2 - 0.3
    g = 1 + _rand(K, seed=226, scale=0.1)
    xd = x.double().requires_grad_(True)
    gd = g.double().requires_grad_(True)
    bd = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xd, (K,), gd, bd, 1e-5).backward(dy.double() @ w.double())
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()
    o_bias, o_ln, stride = 8, 8 + nout, 8 + nout + 2 * K + 8        # regions inside a wider row, nothing else written
    part = torch.full((nblk, stride), 1e30, device=DEV)
    dx = ops.tok_linear_bwd_input(dy.to(DEV), w.to(DEV), ln=(x.to(DEV), mean.float().to(DEV), rstd.float().to(DEV), g.to(DEV)),
                                  add1=add1.to(DEV), add2=add2.to(DEV), ln_partial=(part, o_ln),
                                  bias_partial=(part, o_bias), partial_stride=stride)
    torch.cuda.synchronize()
    assert _relerr(dx.cpu(), xd.grad + add1.double() + add2.double()) < 2e-5
    sums = part.sum(0).cpu()
    assert _relerr(sums[o_ln:o_ln + K], gd.grad) < 2e-5 and _relerr(sums[o_ln + K:o_ln + 2 * K], bd.grad) < 2e-5
    assert _relerr(sums[o_bias:o_bias + nout], dy.double().sum(0)) < 2e-5
    assert bool((part[:, :o_bias] == 1e30).all()) and bool((part[:, o_ln + 2 * K:] == 1e30).all())
    # GELU' epilogue, with the bias column sums of dy:  dy [R][nout] . w [nout][K] * gelu'(h)
    h = _rand(R, K, seed=227)
    hd = h.double().requires_grad_(True)
    _gelu64(hd).backward(dy.double() @ w.double())
    part = torch.zeros((nblk, nout), device=DEV)
    dx = ops.tok_linear_bwd_input(dy.to(DEV), w.to(DEV), gelu_pre=h.to(DEV), bias_partial=(part, 0), partial_stride=nout)
    torch.cuda.synchronize()
    assert _relerr(dx.cpu(), hd.grad) < 2e-5
    assert _relerr(part.sum(0).cpu(), dy.double().sum(0)) < 2e-5
    # plain epilogue + one residual gradient
    dx = ops.tok_linear_bwd_input(dy.to(DEV), w.to(DEV), add1=add1.to(DEV))
    torch.cuda.synchronize()
    assert _relerr(dx.cpu(), dy.double() @ w.double() + add1.double()) < 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_transformer_on_token_gemms_matches_fp64_formula(dim, heads, linear_calls):
    """Transformer(dim, 1, heads, dim / heads, 4 dim) with a context on the fused-launch path (ops.TransformerLayer):
    output and the gradients of x, the context and every parameter against the fp64 formula, no nn.Linear call."""
    ops = _ops()
    from transmf_ad_amd import networks
    torch.manual_seed(7)
    tr = networks.Transformer(dim, 1, heads, dim // heads, 4 * dim, 0.).to(DEV)
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    x0, c0, go = _rand(3, 50, dim, seed=231), _rand(3, 70, dim, seed=232), _rand(3, 50, dim, seed=233)
    tr64 = copy.deepcopy(tr).cpu().double()
    x64, c64 = x0.double().requires_grad_(True), c0.double().requires_grad_(True)
    y64 = _transformer64_live(tr64, x64, c64, x64)
    y64.backward(go.double())
    ref = [y64.detach(), x64.grad, c64.grad] + [p.grad for p in tr64.parameters()]
    x = x0.to(DEV).requires_grad_(True)
    c = c0.to(DEV).requires_grad_(True)
    assert tr._fused(x)
    y = tr(x, context=c, residual=x)
    assert type(y.grad_fn).__name__.startswith("LayerNorm"), y.grad_fn
    y.backward(go.to(DEV))
    torch.cuda.synchronize()
    got = [y.detach().cpu(), x.grad.cpu(), c.grad.cpu()] + [p.grad.cpu() for p in tr.parameters()]
    assert linear_calls[0] == 0
    for i, (a, r) in enumerate(zip(got, ref)):
        assert _relerr(a, r) < 2e-5, (i, _relerr(a, r))


def _graph_nodes(t):
    seen, todo, names = set(), [t.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(nf for nf, _ in fn.next_functions)
    return names


@pytest.mark.parametrize("name", list(MID.values()))
def test_one_call_fusion_matches_per_transformer_path(name, linear_calls):
    """tmf_fusion_train_fwd / _bwd (one library call per pass) against the per-Transformer path, which at these dims now
    also runs on the token GEMMs: the same launch sequence forward (bitwise equal outputs and loss); gradients to fp32
    round-off (1e-5 of each tensor's max)."""
    ops = _ops()
    g = Golden(name)
    res = []
    try:
        for one_call in (True, False):
            ops.FUSION_ONE_CALL = one_call
            net = build(g)
            outs, loss = step(net, g, train=True)
            assert ("FusionTrainBackward" in _graph_nodes(outs["logits"])) == one_call
            res.append((outs, loss, {k: p.grad.clone() for k, p in net.named_parameters()}))
    finally:
        ops.FUSION_ONE_CALL = True
    assert linear_calls[0] == 0
    (o1, l1, g1), (o2, l2, g2) = res
    assert torch.equal(l1, l2)
    for k in o1:
        assert torch.equal(o1[k], o2[k]), k
    for k in g1:
        err = (g1[k] - g2[k]).abs().max().item() / max(g2[k].abs().max().item(), 1e-30)
        assert err <= 1e-5, (k, err)


# ---------------------------------------------------------------------------------------------------------------------
# golden train steps from the reference (tests/golden/make_golden_dims.py)
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", GOLDEN)
def test_train_step_matches_reference_golden_at_dim(name, linear_calls):
    """The project's golden gates (test_gpu_model._golden_train_step: logits, cls / encoder probes, gradient probes, BN
    buffers) at dim 64 / 256, the whole model_ad train step without one nn.Linear call."""
    _golden_train_step(name)
    assert linear_calls[0] == 0


@pytest.mark.parametrize("name", GOLDEN)
def test_fusion_takes_one_call_and_eval_matches_golden_at_dim(name, linear_calls):
    from transmf_ad_amd import _lib
    g = Golden(name)
    net = build(g)
    mri, pet, _y = (torch.from_numpy(a).to(DEV) for a in g.inputs())
    net.train()
    seen = {}
    hook = net.fuse_transformer.register_forward_hook(lambda _m, _i, o: seen.__setitem__("cls", o))
    lo, _dm, _dp = net(mri, pet)
    hook.remove()
    assert "FusionTrainBackward" in _graph_nodes(lo)
    cls = seen["cls"]
    assert type(cls.grad_fn).__name__.startswith("FusionTrain"), cls.grad_fn
    assert _lib.query("tmf_fusion_uses_fused", ctypes.byref(cls.grad_fn.desc)) == 0      # one launch per op
    torch.cuda.synchronize()
    outs, _ = step(build(g), g, train=False)          # val_step: no_grad, per-Transformer path on the token GEMMs
    for k, v in outs.items():
        assert np.abs(v.double().cpu().numpy() - g[f"f32/eval/{k}"]).max() <= TOL, k
    assert linear_calls[0] == 0
