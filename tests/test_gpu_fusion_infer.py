"""The forward-only one-call fusion entry (tmf_fusion_infer_fwd, csrc/fusion_path.hip; the forward-only instances of
xf_fwd_kernel, csrc/xformer_fused.hip) and its route in CrossTransformer_MOD_AVG under torch.no_grad() — val_step
(kfold_train_adversarial.py:144-161) and the test run after training (:229-250).

Reference of every numeric check: tmf_fusion_train_fwd on the same descriptor, tokens, parameters and masks (held to fp64
by test_gpu_kernels.py / test_gpu_dims.py).  The forward-only form is the same arithmetic in the same order with stores
removed, so cls must be BIT-identical: torch.equal, no tolerance."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_criterion import count_launches
from test_gpu_dims import linear_calls  # noqa: F401  (fixture)
from test_gpu_dropout_dims import _keep
from test_gpu_kernels import _fusion64, _rand, _relerr
from test_gpu_model import DEV

pytestmark = pytest.mark.gpu

E_NULL, E_SHAPE, E_WORKSPACE = -1, -2, -4            # include/tmf_hip.h
MIB = 1 << 20


def _lib():
    from transmf_ad_amd import _lib
    return _lib


def _desc(B, N, depth, dim=128, heads=4, flags=0):
    return _lib().FusionDesc(B=B, N=N, dim=dim, heads=heads, dim_head=dim // heads, mlp=4 * dim, depth=depth, flags=flags)


def _params(d, seed=11):
    """Per Transformer instance the 14 tensors of _lib.XFORMER_PTRS order, on the device."""
    dim, inner, mlp = d.dim, d.heads * d.dim_head, d.mlp
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    out = []
    for _ in range(2 * d.depth):
        out.append([1 + rn(dim, scale=0.1), rn(dim, scale=0.1), rn(inner, dim, scale=dim ** -0.5),
                    rn(2 * inner, dim, scale=dim ** -0.5), rn(dim, inner, scale=inner ** -0.5), rn(dim, scale=0.1),
                    1 + rn(dim, scale=0.1), rn(dim, scale=0.1), rn(mlp, dim, scale=dim ** -0.5), rn(mlp, scale=0.1),
                    rn(dim, mlp, scale=mlp ** -0.5), rn(dim, scale=0.1), 1 + rn(dim, scale=0.1), rn(dim, scale=0.1)])
    return [[t.to(DEV).contiguous() for t in inst] for inst in out]


def _masks(d, seed=3):
    rs = np.random.RandomState(seed)
    R = d.B * d.N
    return [[_keep(rs, R, w).to(DEV).contiguous() for w in (d.dim, d.mlp, d.dim)] for _ in range(2 * d.depth)]


def _table(d, params, masks=None):
    L = _lib()
    inst = (L.XformerParams * max(2 * d.depth, 1))()
    for i, ts in enumerate(params):
        for name, t in zip(L.XFORMER_PTRS, ts):
            setattr(inst[i], name, t.data_ptr())
        inst[i].eps1 = inst[i].eps2 = inst[i].epsf = 1e-5
        if masks is not None:
            inst[i].mask_o, inst[i].mask_g, inst[i].mask_f = (m.data_ptr() for m in masks[i])
    return inst


def _tokens(d, seed=201):
    return _rand(d.B, d.N, d.dim, seed=seed).to(DEV), _rand(d.B, d.N, d.dim, seed=seed + 1).to(DEV)


def _train_cls(d, mri, pet, inst):
    L = _lib()
    n = L.query("tmf_fusion_saved_bytes", ctypes.byref(d))
    saved = torch.empty(n, device=DEV, dtype=torch.uint8)
    cls = torch.full((d.B, 4 * d.dim), float("nan"), device=DEV)
    L.call("tmf_fusion_train_fwd", ctypes.byref(d), mri.data_ptr(), pet.data_ptr(), inst, saved.data_ptr(), n, cls.data_ptr(), None)
    torch.cuda.synchronize()
    return cls


def _infer_cls(d, mri, pet, inst, ws=None):
    L = _lib()
    n = L.query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d))
    assert n > 0
    if ws is None:
        ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    assert ws.numel() == n and ws.data_ptr() % 16 == 0
    cls = torch.full((d.B, 4 * d.dim), float("nan"), device=DEV)
    L.call("tmf_fusion_infer_fwd", ctypes.byref(d), mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n, cls.data_ptr(), None)
    torch.cuda.synchronize()
    return cls


def _both(d, masks=False):
    params = _params(d)
    mk = _masks(d) if masks else None
    inst = _table(d, params, mk)
    mri, pet = _tokens(d)
    m0, p0 = mri.clone(), pet.clone()
    ref = _train_cls(d, mri, pet, inst)
    got = _infer_cls(d, mri, pet, inst)
    assert torch.isfinite(ref).all()
    assert torch.equal(mri, m0) and torch.equal(pet, p0)
    return ref, got, (params, mk, inst, mri, pet)


# ---------------------------------------------------------------------------------------------------------------------
# entry level (ctypes), bit-identical to tmf_fusion_train_fwd
# ---------------------------------------------------------------------------------------------------------------------

FUSED_CASES = [          # B, N, depth: what it reaches
    (1, 1, 1),           # one tile with one valid row
    (2, 16, 1),          # one full tile, guarded MT 8
    (3, 17, 2),          # ragged second tile
    (9, 150, 1),         # exact MT 10, second batch group of xf_who
    (2, 200, 1),         # guarded MT 16
    (2, 216, 3),         # exact MT 14, the reference's own geometry
    (1, 300, 1),         # guarded MT 32
    (1, 512, 1),         # exact MT 32
]


@pytest.mark.parametrize("B,N,depth", FUSED_CASES)
def test_fused_geometry_is_bit_identical_to_the_train_entry(B, N, depth):
    d = _desc(B, N, depth)
    assert _lib().query("tmf_fusion_uses_fused", ctypes.byref(d)) == 1
    ref, got, _ = _both(d)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("B,N,depth", [(3, 17, 2), (2, 216, 1)])
def test_fused_geometry_eight_heads_of_16(B, N, depth):
    d = _desc(B, N, depth, heads=8)
    assert _lib().query("tmf_fusion_uses_fused", ctypes.byref(d)) == 1
    ref, got, _ = _both(d)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


def test_depth_zero_is_pooling_only():
    d = _desc(2, 17, 0)
    mri, pet = _tokens(d)
    ref = _train_cls(d, mri, pet, None)
    got = _infer_cls(d, mri, pet, None)
    assert torch.equal(got, ref)
    want = torch.cat([mri.double().mean(1), pet.double().mean(1), mri.double().amax(1), pet.double().amax(1)], dim=1)
    assert _relerr(got, want.cpu()) < 17 * 2.0 ** -24          # a mean of N = 17 fp32 values: N roundings of half an ulp


@pytest.mark.parametrize("dim,heads,per_op", [(64, 4, False), (64, 8, False), (256, 4, False), (256, 8, False), (128, 4, True)],
                         ids=["d64-4x16", "d64-8x8", "d256-4x64", "d256-8x32", "d128-per-op"])
def test_one_launch_per_op_is_bit_identical_to_the_train_entry(dim, heads, per_op):
    d = _desc(3, 50, 2, dim=dim, heads=heads, flags=_lib().FUSION_PER_OP if per_op else 0)
    assert _lib().query("tmf_fusion_uses_fused", ctypes.byref(d)) == 0
    ref, got, _ = _both(d)
    assert torch.equal(got, ref), (got - ref).abs().max().item()


@pytest.mark.parametrize("B,N,depth,dim", [(3, 17, 2, 128), (3, 50, 1, 64)], ids=["fused", "d64"])
def test_keep_masks_are_applied(B, N, depth, dim):
    """Fixed keep-masks (built as tests/test_gpu_dropout_dims.py builds them): equal to tmf_fusion_train_fwd with the same
    masks bit for bit, and different from the mask-free result."""
    d = _desc(B, N, depth, dim=dim)
    ref, got, (params, _mk, _inst, mri, pet) = _both(d, masks=True)
    assert torch.equal(got, ref), (got - ref).abs().max().item()
    plain = _infer_cls(d, mri, pet, _table(d, params))
    assert torch.isfinite(plain).all() and not torch.equal(plain, got)


@pytest.mark.parametrize("B,N,depth,dim", [(3, 17, 2, 128), (3, 50, 2, 256)], ids=["fused", "d256"])
def test_workspace_is_scratch(B, N, depth, dim):
    """Nothing in the workspace is read before it is written (0xFF bytes = NaN everywhere), nothing outside its
    tmf_fusion_infer_workspace_bytes is touched (1 MiB of sentinels on either side), the tokens are not written."""
    d = _desc(B, N, depth, dim=dim)
    ref, clean, (_params_, _mk, inst, mri, pet) = _both(d)
    assert torch.equal(clean, ref)
    n = _lib().query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d))
    big = torch.full((n + 2 * MIB,), 0x5A, device=DEV, dtype=torch.uint8)
    ws = big[MIB:MIB + n]
    ws.fill_(0xFF)
    m0, p0 = mri.clone(), pet.clone()
    first = _infer_cls(d, mri, pet, inst, ws)
    second = _infer_cls(d, mri, pet, inst, ws)
    assert torch.equal(first, clean) and torch.equal(second, clean)
    assert bool((big[:MIB] == 0x5A).all()) and bool((big[MIB + n:] == 0x5A).all())
    assert torch.equal(mri, m0) and torch.equal(pet, p0)


def test_error_paths_return_before_any_launch():
    L = _lib()
    lib = L.load()
    d = _desc(3, 17, 2)
    params = _params(d)
    inst = _table(d, params)
    mri, pet = _tokens(d)
    n = L.query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d))
    ws = torch.empty(n, device=DEV, dtype=torch.uint8)
    cls = torch.full((d.B, 4 * d.dim), 7.0, device=DEV)

    def call(desc, m, p, ins, w, nbytes, c):
        return lib.tmf_fusion_infer_fwd(ctypes.byref(desc), m, p, ins, w, nbytes, c, None)
    assert call(d, mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n - 1, cls.data_ptr()) == E_WORKSPACE
    assert call(d, mri.data_ptr(), pet.data_ptr(), inst, None, n, cls.data_ptr()) == E_NULL
    assert call(d, mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n, None) == E_NULL
    assert call(d, mri.data_ptr(), pet.data_ptr(), None, ws.data_ptr(), n, cls.data_ptr()) == E_NULL
    d96 = _desc(3, 17, 2, dim=96)
    assert call(d96, mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n, cls.data_ptr()) == E_SHAPE
    # a misaligned token pointer: the code tmf_fusion_train_fwd returns for it
    ns = L.query("tmf_fusion_saved_bytes", ctypes.byref(d))
    saved = torch.empty(ns, device=DEV, dtype=torch.uint8)
    want = lib.tmf_fusion_train_fwd(ctypes.byref(d), mri.data_ptr() + 4, pet.data_ptr(), inst, saved.data_ptr(), ns,
                                    cls.data_ptr(), None)
    assert want < 0
    assert call(d, mri.data_ptr() + 4, pet.data_ptr(), inst, ws.data_ptr(), n, cls.data_ptr()) == want
    assert call(d, mri.data_ptr(), pet.data_ptr() + 4, inst, ws.data_ptr(), n, cls.data_ptr()) == want
    torch.cuda.synchronize()
    assert bool((cls == 7.0).all())                  # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# module level
# ---------------------------------------------------------------------------------------------------------------------

def _record_calls(monkeypatch):
    L = _lib()
    names, real = [], L.call

    def recorded(name, *a):
        names.append(name)
        return real(name, *a)
    monkeypatch.setattr(L, "call", recorded)
    return names


def _model(dim, dropout=0.):
    import transmf_ad_amd as T
    torch.manual_seed(0)
    net = T.model_ad(dim=dim, depth=3, heads=4, dim_head=dim // 4, mlp_dim=4 * dim, dropout=dropout).to(DEV)
    with torch.no_grad():
        for p in net.fuse_transformer.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    return net


def _model_tokens(net):
    """The tokens model_ad hands its fusion block for B = 2, 32^3 volumes (eval, no_grad)."""
    g = torch.Generator().manual_seed(5)
    mri, pet = (torch.rand(2, 1, 32, 32, 32, generator=g).to(DEV) for _ in range(2))
    seen = []
    h = net.fuse_transformer.register_forward_pre_hook(lambda _m, args: seen.append(args))
    was = net.training
    net.eval()
    with torch.no_grad():
        net(mri, pet)
    h.remove()
    net.train(was)
    (mt, pt), = seen
    return mt.contiguous(), pt.contiguous()


def test_eval_fusion_block_is_one_call_of_2_depth_plus_3_kernels(monkeypatch):
    from transmf_ad_amd import ops
    depth = 3
    net = _model(128).eval()
    mt, pt = _model_tokens(net)
    fz = net.fuse_transformer
    out = {}

    def run():
        with torch.no_grad():
            out["cls"] = fz(mt, pt)
    names = count_launches(run)
    print("no_grad fusion block:", len(names), "kernels")
    assert len(names) == 2 * depth + 3, names         # weight pack, first K / V, one per instance, pool
    new = out["cls"].clone()
    assert not new.requires_grad and new.grad_fn is None
    # FusionTrain's cls on the same tokens, bit for bit; with grad enabled the call still goes to tmf_fusion_train_fwd
    calls = _record_calls(monkeypatch)
    ref = fz(mt, pt)
    assert type(ref.grad_fn).__name__.startswith("FusionTrain"), ref.grad_fn
    assert "tmf_fusion_train_fwd" in calls and "tmf_fusion_infer_fwd" not in calls
    assert torch.equal(new, ref.detach())
    del calls[:]
    run()
    assert calls == ["tmf_fusion_infer_fwd"]
    # against a CPU fp64 copy of the module: _relerr < 3e-5, the bound test_gpu_kernels.py:995
    # (test_fused_fusion_kernels_match_fp64_formula) holds this forward to
    fz64 = copy.deepcopy(fz).cpu().double()
    c64 = _fusion64(fz64, mt.double().cpu(), pt.double().cpu())
    assert _relerr(new, c64) < 3e-5, _relerr(new, c64)
    # the switch off: the old launch sequence (per instance seven launches and the separate "+ tokens" add, then the pool)
    monkeypatch.setattr(ops, "FUSION_INFER_ONE_CALL", False)
    del calls[:]
    old_names = count_launches(run)
    print("switch off:", len(old_names), "kernels")
    assert "tmf_fusion_infer_fwd" not in calls
    assert len(old_names) == 2 * depth * (7 + 1) + 1, old_names
    assert _relerr(out["cls"], c64) < 3e-5


def test_hook_on_an_inner_transformer_keeps_the_module_path(monkeypatch):
    net = _model(128).eval()
    mt, pt = _model_tokens(net)
    fz = net.fuse_transformer
    calls = _record_calls(monkeypatch)
    with torch.no_grad():
        want = fz(mt, pt)
    assert calls == ["tmf_fusion_infer_fwd"]
    fired = []
    h = fz.layers[1][0].register_forward_hook(lambda _m, _i, o: fired.append(tuple(o.shape)))
    try:
        del calls[:]
        with torch.no_grad():
            got = fz(mt, pt)
        torch.cuda.synchronize()
    finally:
        h.remove()
    assert fired == [tuple(mt.shape)]
    assert "tmf_fusion_infer_fwd" not in calls and len(calls) > 1
    assert _relerr(got, want.cpu()) < 3e-5             # the module walk sums in another order: test_gpu_kernels.py:995's bound


def test_dim_64_eval_block_is_one_library_call(monkeypatch, linear_calls):  # noqa: F811
    net = _model(64).eval()
    mt, pt = _model_tokens(net)
    fz = net.fuse_transformer
    ref = fz(mt, pt)                                   # grad enabled: FusionTrain
    assert type(ref.grad_fn).__name__.startswith("FusionTrain"), ref.grad_fn
    calls = _record_calls(monkeypatch)
    n0 = linear_calls[0]
    with torch.no_grad():
        got = fz(mt, pt)
    torch.cuda.synchronize()
    assert calls == ["tmf_fusion_infer_fwd"]
    assert linear_calls[0] == n0 == 0
    assert torch.equal(got, ref.detach())


def test_train_mode_module_under_no_grad_draws_its_masks():
    """dropout 0.1, train(), no_grad at dim 128: the masks come from torch's generator — the same seed gives equal
    outputs, another seed other outputs."""
    net = _model(128, dropout=0.1)
    mt, pt = _model_tokens(net)
    fz = net.fuse_transformer.train()

    def run(seed):
        torch.manual_seed(seed)
        with torch.no_grad():
            return fz(mt, pt).clone()
    a, b, c = run(1), run(1), run(2)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all()
    assert torch.equal(a, b) and not torch.equal(a, c)
    fz.eval()
    with torch.no_grad():
        e = fz(mt, pt)
    assert not torch.equal(a, e)
