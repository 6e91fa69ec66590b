"""Dropout in the fusion block (options/option.py:39 --dropout) at every dim the token GEMMs take (64, 128, 256;
options/option.py:36): the keep-masks of networks.py:153 (to_out), :131 (after GELU) and :133 (after the second Linear)
applied by the one-launch-per-op path of the one-call entry (csrc/fusion_path.hip) and by ops.TransformerLayer —
token_gemm.hip's masked epilogues, token_ops.hip's masked LayerNorm backward.  No torch nn.Linear on these paths."""
import copy
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from _golden import Golden
from test_gpu_dims import _graph_nodes, linear_calls  # noqa: F401  (fixture)
from test_gpu_kernels import _FixedMask, _fusion64, _gelu64, _rand, _relerr
from test_gpu_model import DEV, _golden_train_step, build

pytestmark = pytest.mark.gpu

GEOMETRIES = [(64, 4), (64, 8), (256, 4), (256, 8)]
DROP_GOLDEN = ["ad_d64_mid_drop", "ad_d256_h8_mid_drop"]


def _ops():
    from transmf_ad_amd import ops
    return ops


def _keep(rs, rows, n, p=0.3):
    return torch.from_numpy((rs.rand(rows, n) >= p).astype(np.float32) / np.float32(1.0 - p))


def _fix_masks(tr, rs, rows):
    """_FixedMask (a fixed scaled keep-mask) at the three Dropout sites of every layer of the Transformer `tr`."""
    for attn_pre, ff_pre in tr.layers:
        at, ff = attn_pre.fn, ff_pre.fn
        dim, mlp = at.to_out[0].out_features, ff.net[0].out_features
        at.to_out[1] = _FixedMask(_keep(rs, rows, dim))
        ff.net[2] = _FixedMask(_keep(rs, rows, mlp))
        ff.net[4] = _FixedMask(_keep(rs, rows, dim))
    tr._drops = None


def _fusion_with_masks(dim, heads, depth, B, N):
    from transmf_ad_amd import networks
    torch.manual_seed(7)
    fz = networks.CrossTransformer_MOD_AVG(dim, depth, heads, dim // heads, 4 * dim, 0.).to(DEV).train()
    with torch.no_grad():
        for p in fz.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    rs = np.random.RandomState(3)
    for pair in fz.layers:
        for tr in pair:
            _fix_masks(tr, rs, B * N)
    return fz


def _inputs(B, N, dim):
    return _rand(B, N, dim, seed=301), _rand(B, N, dim, seed=302), _rand(B, 4 * dim, seed=303)


def _names(fz):
    return ["cls", "d mri", "d pet"] + [k for k, _ in fz.named_parameters()]


def _run(fz, m0, p0, go):
    """cls, both token gradients and every parameter gradient of one pass on the device; the node that made cls."""
    from transmf_ad_amd import _lib
    fz.zero_grad()
    m, p = m0.to(DEV).requires_grad_(True), p0.to(DEV).requires_grad_(True)
    c = fz(m, p)
    fn = c.grad_fn
    fused = _lib.query("tmf_fusion_uses_fused", ctypes.byref(fn.desc)) if hasattr(fn, "desc") else None
    c.backward(go.to(DEV))
    torch.cuda.synchronize()
    return type(fn).__name__, fused, [c.detach().cpu(), m.grad.cpu(), p.grad.cpu()] + [q.grad.cpu() for q in fz.parameters()]


def _ref64(fz, m0, p0, go):
    fz64 = copy.deepcopy(fz).cpu().double().train()
    m64, p64 = m0.double().requires_grad_(True), p0.double().requires_grad_(True)
    c64 = _fusion64(fz64, m64, p64)
    c64.backward(go.double())
    return [c64.detach(), m64.grad, p64.grad] + [p.grad for p in fz64.parameters()]


def _max_rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


# ---------------------------------------------------------------------------------------------------------------------
# the one-call entry, one launch per op
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,N,depth", [(2, 5, 2), (2, 27, 1), (2, 150, 3), (1, 216, 2)])
@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_fusion_block_with_masks_matches_fp64_formula(dim, heads, B, N, depth, linear_calls):
    """CrossTransformer_MOD_AVG with fixed keep-masks at all three Dropout sites of every instance, on the one-call entry's
    one-launch-per-op path, against the fp64 formula that applies them (_fusion64): cls, both token gradients and every
    parameter gradient.  Ragged token counts (partial 16-row tiles), depth 1-3."""
    fz = _fusion_with_masks(dim, heads, depth, B, N)
    m0, p0, go = _inputs(B, N, dim)
    ref = _ref64(fz, m0, p0, go)
    node, fused, got = _run(fz, m0, p0, go)
    assert node.startswith("FusionTrain"), node
    assert fused == 0
    assert linear_calls[0] == 0
    for name, a, r in zip(_names(fz), got, ref):
        assert torch.isfinite(a).all(), name
        assert _relerr(a, r) < 3e-5, (name, _relerr(a, r))


@pytest.mark.parametrize("heads", [4, 8], ids=["4x32", "8x16"])
def test_dim128_per_op_masks_match_fused_kernels(heads, linear_calls):
    """At dim 128 the same masks through one launch per op (ops.FUSION_FUSED_KERNELS = False) and through the fused
    per-instance kernels: every tensor within 1e-5 of its max."""
    ops = _ops()
    B, N, depth = 2, 150, 2
    fz = _fusion_with_masks(128, heads, depth, B, N)
    m0, p0, go = _inputs(B, N, 128)
    res = {}
    try:
        for fused in (True, False):
            ops.FUSION_FUSED_KERNELS = fused
            node, used, res[fused] = _run(fz, m0, p0, go)
            assert node.startswith("FusionTrain"), node
            assert used == int(fused)
    finally:
        ops.FUSION_FUSED_KERNELS = True
    assert linear_calls[0] == 0
    for name, a, b in zip(_names(fz), res[True], res[False]):
        assert torch.isfinite(b).all(), name
        assert _max_rel(b, a) <= 1e-5, (name, _max_rel(b, a))


def test_dim128_masks_beyond_the_fused_kernels_match_fp64_formula(linear_calls):
    """N > 512 (volumes above 128^3): the fused kernels refuse the shape, the one-call entry takes it with its masks."""
    ops = _ops()
    B, N, depth = 1, 600, 1
    assert not ops.fusion_fused_supported(N, 128, 4, 32, 512)
    fz = _fusion_with_masks(128, 4, depth, B, N)
    m0, p0, go = _inputs(B, N, 128)
    ref = _ref64(fz, m0, p0, go)
    node, fused, got = _run(fz, m0, p0, go)
    assert node.startswith("FusionTrain"), node
    assert fused == 0
    assert linear_calls[0] == 0
    for name, a, r in zip(_names(fz), got, ref):
        assert _relerr(a, r) < 3e-5, (name, _relerr(a, r))


@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_one_call_masks_match_per_transformer_path(dim, heads, linear_calls):
    """The same fixed masks through the one-call entry and through one ops.TransformerLayer per Transformer: the same
    forward launches (bitwise-equal cls), gradients to fp32 round-off (1e-5 of each tensor's max)."""
    ops = _ops()
    B, N, depth = 2, 27, 3
    fz = _fusion_with_masks(dim, heads, depth, B, N)
    m0, p0, go = _inputs(B, N, dim)
    res = []
    try:
        for one_call in (True, False):
            ops.FUSION_ONE_CALL = one_call
            node, _used, out = _run(fz, m0, p0, go)
            assert node.startswith("FusionTrain") == one_call, node
            res.append(out)
    finally:
        ops.FUSION_ONE_CALL = True
    assert linear_calls[0] == 0
    assert torch.equal(res[0][0], res[1][0])
    for name, a, b in zip(_names(fz), res[0], res[1]):
        assert _max_rel(a, b) <= 1e-5, (name, _max_rel(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# one Transformer with a context (ops.TransformerLayer)
# ---------------------------------------------------------------------------------------------------------------------

def _transformer64_masked(tr, x, ctx, residual):
    """fp64 Transformer.forward with a context (networks.py:114-175, 215-230) and the Dropout sites (:131, :133, :153)
    applied through the modules that sit there."""
    for attn_pre, ff_pre in tr.layers:
        at, ff = attn_pre.fn, ff_pre.fn
        xn = F.layer_norm(x, (x.shape[-1],), attn_pre.norm.weight, attn_pre.norm.bias, attn_pre.norm.eps)
        q = xn @ at.to_q.weight.t()
        k, v = (ctx @ at.to_kv.weight.t()).chunk(2, dim=-1)
        B, N, inner = q.shape
        h = at.heads
        sp = lambda t: t.reshape(B, t.shape[1], h, inner // h).transpose(1, 2)
        dots = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * at.scale
        out = torch.einsum("bhij,bhjd->bhid", dots.softmax(dim=-1), sp(v)).transpose(1, 2).reshape(B, N, inner)
        x = at.to_out[1](out @ at.to_out[0].weight.t() + at.to_out[0].bias) + x
        xn = F.layer_norm(x, (x.shape[-1],), ff_pre.norm.weight, ff_pre.norm.bias, ff_pre.norm.eps)
        hdn = ff.net[2](_gelu64(xn @ ff.net[0].weight.t() + ff.net[0].bias))
        x = ff.net[4](hdn @ ff.net[3].weight.t() + ff.net[3].bias) + x
    y = F.layer_norm(x, (x.shape[-1],), tr.norm.weight, tr.norm.bias, tr.norm.eps)
    return y if residual is None else y + residual


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("dim,heads", [(64, 4), (128, 4), (256, 8)])
def test_transformer_with_masks_on_token_gemms_matches_fp64_formula(dim, heads, depth, linear_calls):
    """Transformer(dim, depth, heads, dim / heads, 4 dim) with a context and fixed keep-masks takes ops.TransformerLayer:
    output and the gradients of x, the context and every parameter against the fp64 formula, no nn.Linear call."""
    from transmf_ad_amd import networks
    torch.manual_seed(11)
    tr = networks.Transformer(dim, depth, heads, dim // heads, 4 * dim, 0.).to(DEV).train()
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    B, N, M = 3, 50, 70
    _fix_masks(tr, np.random.RandomState(5), B * N)
    x0, c0, go = _rand(B, N, dim, seed=311), _rand(B, M, dim, seed=312), _rand(B, N, dim, seed=313)
    tr64 = copy.deepcopy(tr).cpu().double().train()
    x64, c64 = x0.double().requires_grad_(True), c0.double().requires_grad_(True)
    y64 = _transformer64_masked(tr64, x64, c64, x64)
    y64.backward(go.double())
    ref = [y64.detach(), x64.grad, c64.grad] + [p.grad for p in tr64.parameters()]
    x, c = x0.to(DEV).requires_grad_(True), c0.to(DEV).requires_grad_(True)
    assert tr._fused(x)
    y = tr(x, context=c, residual=x)
    assert "TransformerLayerBackward" in _graph_nodes(y)
    y.backward(go.to(DEV))
    torch.cuda.synchronize()
    got = [y.detach().cpu(), x.grad.cpu(), c.grad.cpu()] + [p.grad.cpu() for p in tr.parameters()]
    assert linear_calls[0] == 0
    assert len(got) == len(ref)
    for i, (a, r) in enumerate(zip(got, ref)):
        assert _relerr(a, r) < 2e-5, (i, _relerr(a, r))


def test_hooked_dropout_keeps_the_module_path(linear_calls):
    """A forward hook on one Dropout module sends its Transformer back to the module path, where the hook fires."""
    from transmf_ad_amd import networks
    torch.manual_seed(13)
    tr = networks.Transformer(64, 1, 4, 16, 256, 0.1).to(DEV).train()
    x, c = _rand(2, 27, 64, seed=321).to(DEV), _rand(2, 27, 64, seed=322).to(DEV)
    assert tr._fused(x)
    seen = []
    h = tr.layers[0][1].fn.net[2].register_forward_hook(lambda _m, _i, o: seen.append(tuple(o.shape)))
    try:
        assert not tr._fused(x)
        tr(x, context=c).sum().backward()
        torch.cuda.synchronize()
    finally:
        h.remove()
    assert seen == [(2, 27, 256)]
    assert linear_calls[0] > 0
    assert tr._fused(x)


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------

def _golden_train_step_ill_conditioned(name, head_tol):
    """test_gpu_model._golden_train_step for a fixture whose train-mode BatchNorm1d head (batch of two) is ill-conditioned:
    the reference's OWN fp32 run is `head_tol`-class away from its fp64 run on the logits, so those (and the head evaluated
    on our cls, and fc_cls.5's statistics) get head_tol.  What is well-posed keeps the standard bounds: cls and the encoder
    outputs against the reference's fp64 probes (5e-5 of scale), D's logits (2e-4), the gradient probes (5e-2 of max), the
    other BatchNorm buffers (1e-4)."""
    import test_gpu_model as M
    from _golden import gprobe, probe, zero_grad_keys
    from oracle import tmf_oracle as O
    g = Golden(name)
    net = build(g)
    seen = {}
    hooks = [net.fuse_transformer.register_forward_hook(lambda _m, _i, o: seen.__setitem__("cls", o))]
    for c in ("mri_cnn", "pet_cnn"):
        hooks.append(getattr(net, c).register_forward_hook(lambda _m, _i, o, c=c: seen.__setitem__(f"{c}.conv4.3", o.contiguous())))
    outs, loss = M.step(net, g, train=True)
    for h in hooks:
        h.remove()
    for k, t in seen.items():
        ref = g[f"f64/probe/{k}"]
        assert np.abs(probe(t) - ref).max() <= 5e-5 * max(1.0, np.abs(ref).max()), (k, probe(t) - ref)
    S = O.to_state(g.arrays(), g.spec, dtype=torch.float64, requires_grad=False)
    k1, k2 = (torch.from_numpy(m) for m in g.masks())
    ref_head = O.fc_cls_forward(S, seen["cls"].detach().double().cpu(), True, (k1, k2))
    assert (outs["logits"].detach().double().cpu() - ref_head).abs().max().item() <= head_tol
    for k, v in outs.items():
        tol = head_tol if k == "logits" else M.TOL
        assert np.abs(v.detach().double().cpu().numpy() - g[f"f64/train/{k}"]).max() <= tol, k
    assert abs(loss.item() - float(g["f64/train/loss"])) <= head_tol
    zk = zero_grad_keys(g.spec, g.model)
    for k, p in net.named_parameters():
        ref = g[f"f64/grad/{k}"]
        got = gprobe(p.grad if p.grad is not None else torch.zeros_like(p))
        if k in zk:
            assert got[2] <= 1e-3 * max(g[f"f64/grad/{k[:-4]}weight"][2], 1e-12) + 1e-6, k
            continue
        assert np.abs(got[3:] - ref[3:]).max() / max(ref[2], 1e-30) <= 5e-2, k
    for k, b in net.named_buffers():
        ref = g[f"f32/buf/{k}"]
        btol = head_tol if k.startswith("fc_cls.5.") else 1e-4
        assert np.abs(b.detach().double().cpu().numpy() - ref).max() <= btol * max(1.0, np.abs(ref).max()), k


# the reference's own fp32 run of ad_d256_h8_mid_drop sits 8.2e-3 from its fp64 run on the logits (2.5e-3 on the loss): its
# two blob samples reach fc_cls's batch-of-two BatchNorm1d with nearly equal features (test_gpu_model.LOGIT_TOL, ad_full_b2)
HEAD_TOL = {"ad_d256_h8_mid_drop": 1e-2}


@pytest.mark.parametrize("name", DROP_GOLDEN)
def test_train_step_with_dropout_matches_reference_golden_at_dim(name, linear_calls):
    """The golden gates of test_gpu_model._golden_train_step on fixtures whose fusion block runs with dropout 0.3 at dim 64
    (4 heads of 16) and dim 256 (8 heads of 32), the whole train step on the library: no nn.Linear call, the fusion block
    one library call per pass."""
    if name in HEAD_TOL:
        _golden_train_step_ill_conditioned(name, HEAD_TOL[name])
    else:
        _golden_train_step(name)
    assert linear_calls[0] == 0
    g = Golden(name)
    net = build(g).train()
    mri, pet, _y = (torch.from_numpy(a).to(DEV) for a in g.inputs())
    lo, _dm, _dp = net(mri, pet)
    assert "FusionTrainBackward" in _graph_nodes(lo)
    assert linear_calls[0] == 0


@pytest.mark.parametrize("dim", [64, 256])
def test_real_dropout_train_step_on_the_library(dim, linear_calls):
    """model_ad(dim, dropout=0.1), B = 2, 48^3: the masks come from ops.dropout_keep_masks (torch's generator): the same
    seed gives a bitwise-equal step, another seed other logits; eval under no_grad equals a dropout-0 model."""
    import transmf_ad_amd as T
    torch.manual_seed(0)
    kw = dict(dim=dim, depth=3, heads=4, dim_head=dim // 4, mlp_dim=4 * dim)
    net = T.model_ad(dropout=0.1, **kw).to(DEV)
    mri, pet = torch.rand(2, 1, 48, 48, 48, device=DEV), torch.rand(2, 1, 48, 48, 48, device=DEV)
    y = torch.tensor([0, 1], device=DEV)
    ones, zeros = torch.ones_like(y), torch.zeros_like(y)
    crit = nn.CrossEntropyLoss()
    state0 = copy.deepcopy(net.state_dict())

    def run(seed):
        net.load_state_dict(state0)          # (BatchNorm running statistics: every run starts from the same buffers)
        net.zero_grad(set_to_none=True)
        net.train()
        torch.manual_seed(seed)
        lo, dm, dp = net(mri, pet)
        loss = crit(lo, y) + (crit(dm, ones) + crit(dp, zeros)) / 2
        nodes = _graph_nodes(lo)
        loss.backward()
        torch.cuda.synchronize()
        return lo.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in net.named_parameters()}, nodes

    a, b, c = run(1), run(1), run(2)
    assert "FusionTrainBackward" in a[3]
    assert linear_calls[0] == 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    assert not torch.equal(a[0], c[0])
    net0 = T.model_ad(dropout=0., **kw).to(DEV)
    net0.load_state_dict(net.state_dict())
    net.eval()
    net0.eval()
    with torch.no_grad():
        e1, e0 = net(mri, pet), net0(mri, pet)
    for u, v in zip(e1, e0):
        assert torch.equal(u, v)
    assert linear_calls[0] == 0
