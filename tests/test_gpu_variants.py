"""The reference's remaining model classes on MI355X (models/mymodel.py:40-141) and networks.CrossTransformer
(networks.py:233-252): the two-part-context attention entries (tmf_xattn_fwd_cat / _bwd_cat) against fp64, the
CrossTransformer on the token GEMMs against the fp64 formula and against a concatenated context, and golden train / eval
steps from the reference (tests/golden/make_golden_variants.py)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
from torch import nn

from _golden import GOLDEN_DIR, gprobe, probe
from test_gpu_dims import linear_calls  # noqa: F401  (fixture)
from test_gpu_kernels import _rand, _relerr, _transformer64_live
from test_gpu_model import DEV, GATE, TOL, FixedMaskDropout, ScaledMask

pytestmark = pytest.mark.gpu

RES = ["res_mid", "res_mid_drop", "res_d64_mid", "res_d256_h8_mid", "res_full_b2"]
GOLDEN = RES + ["tr_mid", "cnnp_mid"]


# ---------------------------------------------------------------------------------------------------------------------
# kernel level: keys / values from two buffers
# ---------------------------------------------------------------------------------------------------------------------

def _cat_attention(q, kv1, kv2, heads, scale, dout):
    """tmf_xattn_fwd_cat / _bwd_cat on device tensors -> out, lse, dq, dkv1, dkv2."""
    from transmf_ad_amd import _lib, ops
    B, N, inner = q.shape
    M1, M2 = kv1.shape[1], kv2.shape[1]
    dh = inner // heads
    out = torch.empty_like(q)
    lse = torch.empty((B, heads, N), device=DEV)
    s = ops._stream()
    p = lambda t, off=0: t.data_ptr() + 4 * off
    _lib.call("tmf_xattn_fwd_cat", p(q), p(kv1), p(kv1, inner), p(kv2), p(kv2, inner), p(out), p(lse), B, heads, N, M1, M2, dh,
              inner, 2 * inner, scale, s)
    dq, dkv1, dkv2 = torch.empty_like(q), torch.empty_like(kv1), torch.empty_like(kv2)
    _lib.call("tmf_xattn_bwd_cat", p(q), p(kv1), p(kv1, inner), p(kv2), p(kv2, inner), p(out), p(lse), p(dout), p(dq),
              p(dkv1), p(dkv1, inner), p(dkv2), p(dkv2, inner), B, heads, N, M1, M2, dh, inner, 2 * inner, 2 * inner, scale, s)
    torch.cuda.synchronize()
    return out, lse, dq, dkv1, dkv2


@pytest.mark.parametrize("B,heads,N,M1,M2,dh", [
    (2, 4, 216, 216, 216, 32),      # 96^3 tokens: 432 keys
    (1, 4, 512, 512, 512, 32),      # 128^3 tokens: 1 024 keys cross the 512-row resident limit
    (2, 2, 100, 37, 61, 16),        # ragged parts, a key tile straddling the split
    (1, 2, 70, 300, 250, 64),       # dh 64: 256-row super-blocks, the split inside the second one
    (3, 8, 27, 27, 27, 8),
])
def test_cat_attention_matches_fp64(B, heads, N, M1, M2, dh):
    """out, lse, dq, dk, dv of attention over [kv1 ; kv2] against fp64 autograd through torch.cat, and bitwise equal to the
    one-buffer entry on the concatenated tensor (the same staging, the same arithmetic)."""
    from transmf_ad_amd import ops
    inner = heads * dh
    scale = dh ** -0.5
    q, kv1, kv2 = _rand(B, N, inner, seed=61), _rand(B, M1, 2 * inner, seed=62), _rand(B, M2, 2 * inner, seed=63)
    go = _rand(B, N, inner, seed=64)
    qd, k1d, k2d = (t.double().requires_grad_(True) for t in (q, kv1, kv2))
    kv = torch.cat([k1d, k2d], dim=1)
    sp = lambda t, n: t.reshape(B, n, heads, dh).transpose(1, 2)
    s64 = torch.einsum("bhid,bhjd->bhij", sp(qd, N), sp(kv[..., :inner], M1 + M2)) * scale
    ref = torch.einsum("bhij,bhjd->bhid", s64.softmax(-1), sp(kv[..., inner:], M1 + M2)).transpose(1, 2).reshape(B, N, inner)
    ref.backward(go.double())
    lse_ref = torch.logsumexp(s64.detach(), dim=-1) / np.log(2.0)
    out, lse, dq, dkv1, dkv2 = _cat_attention(q.to(DEV), kv1.to(DEV), kv2.to(DEV), heads, scale, go.to(DEV))
    assert _relerr(out, ref.detach()) < 5e-6
    assert (lse.double().cpu() - lse_ref).abs().max().item() < 1e-5 * max(1.0, lse_ref.abs().max().item())
    assert _relerr(dq, qd.grad) < 2e-5
    assert _relerr(dkv1, k1d.grad) < 2e-5 and _relerr(dkv2, k2d.grad) < 2e-5
    one = ops.cross_attention(q.to(DEV), torch.cat([kv1, kv2], 1).to(DEV).contiguous(), heads, scale)
    torch.cuda.synchronize()
    assert torch.equal(one, out)


# ---------------------------------------------------------------------------------------------------------------------
# module level: CrossTransformer on the token GEMMs
# ---------------------------------------------------------------------------------------------------------------------

def _cross64(ct, m, p):
    """CrossTransformer.forward (networks.py:248-252) in fp64 on an fp64 CPU copy."""
    for mri_enc, pet_enc in ct.layers:
        m = _transformer64_live(mri_enc, m, torch.cat([m, p], 1), m)
        p = _transformer64_live(pet_enc, p, torch.cat([m, p], 1), p)
    return m, p


def _cross_module(dim, heads, depth, seed=7):
    from transmf_ad_amd import networks
    torch.manual_seed(seed)
    ct = networks.CrossTransformer(dim, depth, heads, dim // heads, 4 * dim, 0.).to(DEV).train()
    with torch.no_grad():
        for q in ct.parameters():
            q.add_(torch.randn_like(q) * 0.05)
    return ct


def _run_cross(ct, m0, p0, gm, gp):
    ct.zero_grad()
    m, p = m0.to(DEV).requires_grad_(True), p0.to(DEV).requires_grad_(True)
    mo, po = ct(m, p)
    (mo * gm.to(DEV)).sum().add((po * gp.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    return [mo.detach().cpu(), po.detach().cpu(), m.grad.cpu(), p.grad.cpu()] + [q.grad.cpu() for q in ct.parameters()]


@pytest.mark.parametrize("dim,heads,B,N,depth", [(64, 4, 2, 27, 2), (128, 4, 2, 216, 3), (128, 8, 1, 50, 1),
                                                 (256, 8, 2, 27, 2)])
def test_cross_transformer_matches_fp64_formula(dim, heads, B, N, depth, linear_calls):
    """Both output token tensors, both input gradients and every parameter gradient against the fp64 formula, with no
    nn.Linear and no concatenated context: every instance's to_kv runs once per stream and the attention reads both."""
    ct = _cross_module(dim, heads, depth)
    m0, p0, gm, gp = (_rand(B, N, dim, seed=s) for s in (71, 72, 73, 74))
    ct64 = copy.deepcopy(ct).cpu().double()
    m64, p64 = m0.double().requires_grad_(True), p0.double().requires_grad_(True)
    mo, po = _cross64(ct64, m64, p64)
    ((mo * gm.double()).sum() + (po * gp.double()).sum()).backward()
    ref = [mo.detach(), po.detach(), m64.grad, p64.grad] + [q.grad for q in ct64.parameters()]
    real_cat = torch.cat
    cats = [0]

    def counted(ts, *a, **k):
        cats[0] += int(any(t.is_cuda and t.dim() == 3 for t in ts))
        return real_cat(ts, *a, **k)
    torch.cat = counted
    try:
        got = _run_cross(ct, m0, p0, gm, gp)
    finally:
        torch.cat = real_cat
    assert linear_calls[0] == 0 and cats[0] == 0
    names = ["mri", "pet", "d mri", "d pet"] + [k for k, _ in ct.named_parameters()]
    for name, a, r in zip(names, got, ref):
        assert torch.isfinite(a).all(), name
        assert _relerr(a, r) < 3e-5, (name, _relerr(a, r))


def test_two_part_context_matches_a_concatenated_one(linear_calls):
    """One Transformer with context [c1 ; c2] handed over as two tensors and as their torch.cat: bitwise-equal output and
    input gradients of x; the context and to_kv gradients to fp32 round-off (to_kv's weight gradient is two sums)."""
    from transmf_ad_amd import networks
    torch.manual_seed(3)
    tr = networks.Transformer(128, 1, 4, 32, 512, 0.).to(DEV)
    x0, c10, c20, go = _rand(2, 216, 128, seed=81), _rand(2, 216, 128, seed=82), _rand(2, 216, 128, seed=83), \
        _rand(2, 216, 128, seed=84)
    res = []
    for two in (True, False):
        tr.zero_grad()
        x, c1, c2 = (t.to(DEV).requires_grad_(True) for t in (x0, c10, c20))
        y = tr(x, context=c1, context2=c2) if two else tr(x, context=torch.cat([c1, c2], 1))
        y.backward(go.to(DEV))
        torch.cuda.synchronize()
        res.append([y.detach(), x.grad, c1.grad, c2.grad] + [q.grad.clone() for q in tr.parameters()])
    assert linear_calls[0] == 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2:], res[1][2:]):
        assert (a - b).abs().max().item() <= 1e-5 * b.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# golden train / eval steps from the reference
# ---------------------------------------------------------------------------------------------------------------------

class _VGolden:
    """A make_golden_variants.py fixture: the state_dict spec comes from its meta (the oracle does not know these models)."""

    def __init__(self, name):
        self.z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
        self.meta = m = json.loads(bytes(self.z["meta"]).decode())
        self.model, self.kw, self.batch, self.size = m["model"], m["kwargs"], m["batch"], tuple(m["size"])
        self.spec = {k: (kind, tuple(s)) for (k, s), kind in zip(m["keys"], m["kinds"])}

    def __getitem__(self, k):
        return self.z[k]

    def arrays(self):
        from oracle import params as P
        return P.init_arrays(self.spec, seed=self.meta["param_seed"])

    def inputs(self):
        from oracle import params as P
        return P.make_inputs(self.batch, self.size, seed=self.meta["input_seed"], kind=self.meta["input_kind"])


def _build(g, inject_masks=True):
    import transmf_ad_amd as T
    from oracle import params as P
    if g.model == "model_CNN":
        net = T.model_CNN(g.kw["dim"])
    else:
        net = getattr(T, g.model)(dropout=g.meta["fusion_dropout"], **g.kw)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g.arrays().items()}, strict=True)
    net = net.to(DEV)
    if inject_masks:
        for i, km in zip(g.meta["head_dropout"], P.make_masks(g.batch, seed=g.meta["mask_seed"])):
            net.fc_cls[i] = FixedMaskDropout(torch.from_numpy(km).float().to(DEV))
        p = g.meta["fusion_dropout"]
        if p > 0:
            tokens = (g.size[0] // 16) * (g.size[1] // 16) * (g.size[2] // 16)
            fm = P.make_fusion_masks(g.batch * tokens, 2 * g.kw["depth"], p, g.kw["dim"], g.kw["mlp_dim"],
                                     seed=g.meta["fusion_mask_seed"])
            inst = 0
            for pair in net.fuse_transformer.layers:
                for tr in pair:
                    at, ff = tr.layers[0][0].fn, tr.layers[0][1].fn
                    mo, mg, mf = (ScaledMask(torch.from_numpy(k.astype(np.float32) / np.float32(1.0 - p)).to(DEV))
                                  for k in fm[inst])
                    at.to_out[1], ff.net[2], ff.net[4] = mo, mg, mf
                    tr._drops = None
                    inst += 1
    return net


def _step(net, g, train=True):
    mri, pet, y = (torch.from_numpy(a).to(DEV) for a in g.inputs())
    net.train(train)
    with torch.enable_grad() if train else torch.no_grad():
        lo = net(mri, pet)
        loss = nn.CrossEntropyLoss()(lo, y)
        if train:
            loss.backward()
    torch.cuda.synchronize()
    return lo, loss


def _zero_grad_keys(g):
    z = {k for k, (_kind, s) in g.spec.items() if k.endswith(".bias") and len(g.spec[k[:-4] + "weight"][1]) == 5}
    if g.model == "model_transformer":          # constant shifts ahead of fc_cls's train-mode BatchNorm1d layers
        z |= {"fc_cls.0.bias", "fc_cls.4.bias", f"fuse_transformer.layers.{g.kw['depth'] - 1}.1.norm.bias"}
    return z


@pytest.mark.parametrize("name", GOLDEN)
def test_train_step_matches_reference_golden(name):
    """Logits and loss (TOL where no train-mode BatchNorm1d precedes the logits, GATE behind model_transformer's), the
    encoder outputs, every Transformer instance's output and the fusion block's output against the reference's fp64
    probes, gradient probes and buffers."""
    g = _VGolden(name)
    net = _build(g)
    seen, hooks = {}, []
    for c in ("mri_cnn", "pet_cnn"):
        hooks.append(getattr(net, c).register_forward_hook(lambda _m, _i, o, c=c: seen.__setitem__(f"{c}.conv4.3", o.contiguous())))
    if hasattr(net, "fuse_transformer"):
        for l, pair in enumerate(net.fuse_transformer.layers):
            for s in (0, 1):
                hooks.append(pair[s].register_forward_hook(
                    lambda _m, _i, o, k=f"fuse_transformer.layers.{l}.{s}": seen.__setitem__(k, o)))
        hooks.append(net.fuse_transformer.register_forward_hook(lambda _m, _i, o: seen.__setitem__("fused", o)))
    lo, loss = _step(net, g)
    for h in hooks:
        h.remove()
    for k, t in seen.items():
        ref = g[f"f64/probe/{k}"]
        got = probe(t) if torch.is_tensor(t) else np.concatenate([probe(u) for u in t])
        assert np.abs(got - ref).max() <= 5e-5 * max(1.0, np.abs(ref).max()), k
    tol = GATE if g.model == "model_transformer" else TOL
    got = lo.detach().double().cpu().numpy()
    assert np.abs(got - g["f32/train/logits"]).max() <= tol
    assert np.abs(got - g["f64/train/logits"]).max() <= tol
    assert abs(loss.item() - float(g["f64/train/loss"])) <= tol
    zk = _zero_grad_keys(g)
    for k, p in net.named_parameters():
        ref = g[f"f64/grad/{k}"]
        gp = gprobe(p.grad if p.grad is not None else torch.zeros_like(p))
        if k in zk:
            assert gp[2] <= 1e-3 * max(g[f"f64/grad/{k[:-4]}weight"][2], 1e-12) + 1e-6, k
            continue
        assert np.abs(gp[3:] - ref[3:]).max() / max(ref[2], 1e-30) <= 5e-2, k
    for k, b in net.named_buffers():
        ref = g[f"f32/buf/{k}"]
        btol = GATE if k.startswith("fc_cls.5.") else 1e-4
        assert np.abs(b.detach().double().cpu().numpy() - ref).max() <= btol * max(1.0, np.abs(ref).max()), k


@pytest.mark.parametrize("name", GOLDEN)
def test_eval_matches_reference_golden(name):
    g = _VGolden(name)
    lo, _ = _step(_build(g), g, train=False)
    assert np.abs(lo.double().cpu().numpy() - g["f32/eval/logits"]).max() <= TOL


@pytest.mark.parametrize("name", ["res_d64_mid", "res_mid", "res_d256_h8_mid"])
def test_cross_transformer_of_the_model_makes_no_linear_call(name, linear_calls):
    """At dim 64, 128 and 256 the model's fusion block runs on the token GEMMs: no nn.Linear, no concatenated context."""
    g = _VGolden(name)
    net = _build(g)
    lo, _ = _step(net, g)
    assert linear_calls[0] == 3                   # fc_cls's three Linears: the model's heads run on stock torch ops
    names, todo, done = set(), [lo.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in done:
            continue
        done.add(fn)
        names.add(type(fn).__name__)
        todo.extend(nf for nf, _ in fn.next_functions)
    assert "TransformerLayerBackward" in names


def test_model_cnn_takes_the_one_launch_heads():
    g = _VGolden("cnnp_mid")
    net = _build(g)
    mri, pet, _y = (torch.from_numpy(a).to(DEV) for a in g.inputs())
    lo = net.train()(mri, pet)
    assert type(lo.grad_fn).__name__.startswith("HeadsCNN"), lo.grad_fn


@pytest.mark.parametrize("name", ["res_mid", "tr_mid", "cnnp_mid"])
def test_two_identical_steps_are_bit_identical(name):
    g = _VGolden(name)
    res = []
    for _ in range(2):
        net = _build(g)
        lo, loss = _step(net, g)
        res.append([lo.detach(), loss.detach()] + [p.grad.detach().clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*res))


def test_live_dropout_is_reproducible_under_manual_seed():
    """model_transformer_res(dropout=0.1) with its real nn.Dropout modules (fusion block and fc_cls): the same seed gives the
    same step bit for bit, another seed another one."""
    g = _VGolden("res_mid")
    import transmf_ad_amd as T
    net = T.model_transformer_res(dropout=0.1, **g.kw).to(DEV)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(DEV) for k, v in g.arrays().items()}, strict=True)
    mri, pet, _y = (torch.from_numpy(a).to(DEV) for a in g.inputs())
    outs = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        net.train()
        lo = net(mri, pet)
        lo.sum().backward()
        outs.append((lo.detach().clone(), net.fuse_transformer.layers[0][0].layers[0][0].fn.to_q.weight.grad.clone()))
        net.zero_grad(set_to_none=True)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])
    assert all(torch.isfinite(t).all() for o in outs for t in o)
