"""The attention maps on the device: tmf_xattn_probs on its own (csrc/attention.hip, through _lib.call with raw pointers)
against the fp64 maps of tests/_attn_map_inputs.py at every boundary shape of tests/_attn_inputs.py; tmf_fusion_attn_maps
(csrc/fusion_path.hip) on random tokens against tmf_fusion_infer_fwd and the fp64 formula; attention_maps(model, ...) against
the maps the reference itself builds (tests/golden/attn_maps_*.npz).

probs are judged per query row and head, recv per (batch, head) row:
    |kernel - fp64| <= MARGIN x floor_distance(ATTN_MAP_DISTANCE[case][quantity, class]) x max |fp64| of the row,
and the sums that are 1 exactly (a probs row, a recv row over the keys) by the same tolerance (sum_ratios says why).
Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs must be
unchanged, every output element written and finite, and the inputs are surrounded by NaN."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import _attn_inputs as ai
import _attn_map_inputs as mi
from _golden import GOLDEN_DIR, Golden
from test_gpu_bn_reduce import Arena, _call, _st
from test_gpu_fusion_infer import _desc, _infer_cls, _params, _table, _tokens
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs and fp64 maps of one case (shared by the tests; never modified)."""
    inp = ai.attn_inputs(case)
    return inp, mi.map_ref(inp)


RUNS = ("_p", "_r", "_b", "_again")          # probs only, recv only, both, both again


def _run(case, cat, source):
    """tmf_xattn_probs of one case on one arena, four times: probs alone, recv alone, both, both again.  `cat`: on the two
    context parts, else on the whole context in one buffer; source "kernel": lse from tmf_xattn_fwd / _fwd_cat on the same
    arena, "fp64": the fp64 lse rounded to fp32.  -> {"probs" + run: (B, heads, N, M), "recv" + run: (B, heads, M)}."""
    B, heads, N, M1, M2, dh = case
    M, inner = M1 + M2, heads * dh
    inp, ref = _case(case)
    cols = ai.layout_columns(case)
    parts = [(0, M1), (M1, M)] if cat else [(0, M)]
    k, v = ai.to_mem(inp["k"]), ai.to_mem(inp["v"])
    ins = dict(ai.place([(ai.to_mem(inp["q"]), cols["q"])], N, B))
    for i, (a, b) in enumerate(parts):
        for buf, t in ai.place([(k[:, a:b], cols["k"]), (v[:, a:b], cols["v"])], b - a, B).items():
            ins[f"{buf}{i}"] = t
    outs = {}
    if source == "fp64":
        ins["lse"] = ref["lse"].float().contiguous()
    else:
        outs.update(out=((B, N, inner), F32), lse=((B, heads, N), F32))
    for tag in RUNS:
        if tag != "_r":
            outs["probs" + tag] = ((B, heads, N, M), F32)
        if tag != "_p":
            outs["recv" + tag] = ((B, heads, M), F32)
    q_stride, kv_stride = cols["q"][1], cols["k"][1]
    arena = Arena(ins, outs, tail=64 * max(q_stride, kv_stride) * 4)

    def at(name, part=None):
        buf, _width, col = cols[name]
        return arena.ptr(buf if part is None else f"{buf}{part}") + 4 * col

    scale = inp["scale"]
    if source == "kernel":
        kv_args = [at(n, i) for i in range(len(parts)) for n in ("k", "v")]
        _call("tmf_xattn_fwd_cat" if cat else "tmf_xattn_fwd", at("q"), *kv_args, arena.ptr("out"), arena.ptr("lse"),
              B, heads, N, *([M1, M2] if cat else [M]), dh, q_stride, kv_stride, scale, _st())
    k_args = [at("k", 0), at("k", 1) if cat else None]
    for tag in RUNS:
        _call("tmf_xattn_probs", at("q"), *k_args, arena.ptr("lse"), None if tag == "_r" else arena.ptr("probs" + tag),
              None if tag == "_p" else arena.ptr("recv" + tag), B, heads, N, *([M1, M2] if cat else [M, 0]), dh, q_stride,
              kv_stride, scale, _st())
    return arena.fetch(may_nan=tuple(outs))          # every element written; finiteness is judged below


@pytest.mark.parametrize("source", ("kernel", "fp64"))
@pytest.mark.parametrize("case", ai.ATTN_CASES, ids=ai.case_id)
def test_probs_kernel_against_fp64(case, source):
    """Every output finite and within its per-row tolerance, the sums over the keys 1; probs alone, recv alone, both and a
    second call of both bit-identical; a two-part case also on the concatenated context in one buffer, bit-identical."""
    M2 = case[4]
    res = _run(case, M2 > 0, source)
    for n in ("probs", "recv"):
        a, b = ("_p" if n == "probs" else "_r"), "_b"
        assert torch.isfinite(res[n + b]).all(), f"{n} is not finite"
        assert torch.equal(res[n + a], res[n + b]), f"{n}: alone and together differ"
        assert torch.equal(res[n + b], res[n + "_again"]), f"{n}: two calls differ"
    if M2 > 0:
        one = _run(case, False, source)
        for n in ("probs_b", "recv_b"):
            assert torch.equal(res[n], one[n]), f"{n}: two parts differ from the one-buffer call on the concatenated context"
    got = dict(probs=res["probs_b"], recv=res["recv_b"])
    bad = []
    for what, ratios in (("value", mi.map_ratios(got, _case(case)[1], case)), ("sum", mi.sum_ratios(got, case))):
        for (name, cls), ratio in ratios.items():
            print(f"{ai.case_id(case)} {ai.attn_layout(case)} {source} {name} {cls} {what}: err / tol {ratio:.3f}")
            if not ratio <= 1.0:
                bad.append((name, cls, what, f"{ratio:.3g}"))
    assert not bad, f"{case} {source}: {bad} beyond their tolerance"


def test_probs_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    t = torch.full((64, 64), 7.0, device=DEV)
    p = t.data_ptr()
    args = (2, 2, 8, 8, 0, 16, 32, 64, 0.25, None)
    assert lib.tmf_xattn_probs(p, p, None, p, None, None, *args) < 0           # neither output
    assert lib.tmf_xattn_probs(p, p, None, p, p, p, 2, 2, 8, 8, 4, 16, 32, 64, 0.25, None) < 0    # M2 > 0 without k2
    assert lib.tmf_xattn_probs(p, p, None, p, p, p, 2, 2, 8, 8, 0, 12, 32, 64, 0.25, None) < 0    # dh
    assert lib.tmf_xattn_probs(p + 4, p, None, p, p, p, *args) < 0             # alignment of q
    assert lib.tmf_xattn_probs(p, p, None, p, p, p, 2, 2, 8, 8, 0, 16, 30, 64, 0.25, None) < 0    # q_stride
    torch.cuda.synchronize()
    assert bool((t == 7.0).all())


def test_ops_xattn_probs_two_part_context():
    """ops.xattn_probs on the to_q / to_kv layout with a second context part, lse from tmf_xattn_fwd_cat."""
    from transmf_ad_amd import _lib, ops
    case = (2, 2, 50, 33, 30, 16)
    B, heads, N, M1, M2, dh = case
    inner = heads * dh
    inp, ref = _case(case)
    q = ai.to_mem(inp["q"]).contiguous().to(DEV)
    kv = torch.cat([ai.to_mem(inp["k"]), ai.to_mem(inp["v"])], 2)
    kv1, kv2 = kv[:, :M1].contiguous().to(DEV), kv[:, M1:].contiguous().to(DEV)
    out, lse = torch.empty((B, N, inner), device=DEV), torch.empty((B, heads, N), device=DEV)
    _lib.call("tmf_xattn_fwd_cat", q.data_ptr(), kv1.data_ptr(), kv1.data_ptr() + 4 * inner, kv2.data_ptr(),
              kv2.data_ptr() + 4 * inner, out.data_ptr(), lse.data_ptr(), B, heads, N, M1, M2, dh, inner, 2 * inner,
              inp["scale"], _st())
    probs, recv = ops.xattn_probs(q, kv1, lse, heads, inp["scale"], kv2=kv2)
    none, recv2 = ops.xattn_probs(q, kv1, lse, heads, inp["scale"], kv2=kv2, want_probs=False)
    assert none is None and torch.equal(recv, recv2)
    ratios = mi.map_ratios(dict(probs=probs.cpu(), recv=recv.cpu()), ref, case)
    assert max(ratios.values()) <= 1.0, ratios


# ---------------------------------------------------------------------------------------------------------------------
# tmf_fusion_attn_maps on random tokens
# ---------------------------------------------------------------------------------------------------------------------

def _host_fusion(d, params, dtype):
    """CrossTransformer_MOD_AVG on the CPU in `dtype` holding the entry test's parameters (its own forward is never run)."""
    import transmf_ad_amd as T
    ft = T.CrossTransformer_MOD_AVG(d.dim, d.depth, d.heads, d.dim_head, d.mlp, 0.)
    with torch.no_grad():
        for dst, src in zip(ft._one_call_args()[1], [t for inst in params for t in inst]):
            dst.copy_(src.cpu())
    return ft.to(dtype).eval()


def _rows(t):
    """(instances, B, heads, rows, M) whether t is probs (depth, 2, B, heads, N, N) or recv (depth, 2, B, heads, N)."""
    t = t.reshape(-1, *t.shape[2:])
    return t if t.dim() == 5 else t.unsqueeze(3)


def _row_err(got, ref):
    """Per instance: the worst row's max |got - ref| over max |ref| of the row."""
    got, ref = _rows(got), _rows(ref)
    return [float(mi.row_error(got[i], ref[i]).max()) for i in range(ref.shape[0])]


@pytest.mark.parametrize("N", (27, 40))
@pytest.mark.parametrize("dim,heads", [(64, 4), (128, 4), (128, 8), (256, 4)], ids=["d64", "d128", "d128-h8", "d256"])
def test_fusion_attn_maps_entry(dim, heads, N):
    """cls bit-identical to tmf_fusion_infer_fwd with TMF_FUSION_PER_OP (whatever the descriptor's own flags say), with and
    without probs; recv the same bits either way; probs and recv against attention_maps_torch in fp64 on the CPU, within
    MARGIN distances of the same formula in fp32 on the CPU (per instance, the worst row); the workspace is scratch."""
    import transmf_ad_amd as T
    from transmf_ad_amd import _lib
    B, depth = 2, 2
    d = _desc(B, N, depth, dim=dim, heads=heads)
    d_op = _desc(B, N, depth, dim=dim, heads=heads, flags=_lib.FUSION_PER_OP)
    params = _params(d)
    inst = _table(d, params)
    mri, pet = _tokens(d)
    m0, p0 = mri.clone(), pet.clone()
    want_cls = _infer_cls(d_op, mri, pet, inst)
    n = _lib.query("tmf_fusion_attn_maps_workspace_bytes", ctypes.byref(d))
    assert n == _lib.query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d_op)) > 0
    res = {}
    for tag, want_probs in (("both", True), ("recv", False)):
        ws = torch.full((n,), 0xFF, device=DEV, dtype=torch.uint8)
        cls = torch.full((B, 4 * dim), float("nan"), device=DEV)
        recv = torch.full((2 * depth, B, heads, N), float("nan"), device=DEV)
        probs = torch.full((2 * depth, B, heads, N, N), float("nan"), device=DEV) if want_probs else None
        _lib.call("tmf_fusion_attn_maps", ctypes.byref(d), mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n, cls.data_ptr(),
                  None if probs is None else probs.data_ptr(), recv.data_ptr(), None)
        torch.cuda.synchronize()
        res[tag] = (cls, recv, probs)
        assert torch.equal(cls, want_cls), (cls - want_cls).abs().max().item()
    assert torch.equal(res["both"][1], res["recv"][1])
    assert torch.equal(mri, m0) and torch.equal(pet, p0)
    assert _lib.load().tmf_fusion_attn_maps(ctypes.byref(d), mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), n,
                                            cls.data_ptr(), None, None, None) < 0          # recv is required
    _cls, recv, probs = res["both"]
    assert torch.isfinite(recv).all() and torch.isfinite(probs).all()
    ref = T.attention_maps_torch(_host_fusion(d, params, torch.float64), mri.double().cpu(), pet.double().cpu(), probs=True)
    f32 = T.attention_maps_torch(_host_fusion(d, params, torch.float32), mri.cpu(), pet.cpu(), probs=True)
    shape = (depth, 2, B, heads, N)
    bad = []
    for name, got, r64, r32 in (("probs", probs.cpu().view(*shape, N), ref.probs, f32.probs),
                                ("recv", recv.cpu().view(shape), ref.received, f32.received)):
        for i, (err, dist) in enumerate(zip(_row_err(got, r64), _row_err(r32, r64))):
            tol = mi.MARGIN * mi.floor_distance(dist)
            print(f"dim {dim} heads {heads} N {N} {name} instance {i}: err {err:.3e}, fp32 formula {dist:.3e}, err / tol {err / tol:.3f}")
            if not err <= tol:
                bad.append((name, i, f"{err / tol:.3g}"))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# attention_maps(model, ...) against the reference's own maps
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("ad_mid", "ad_mid_h8", "ad_d64_mid", "ad_d256_mid"))
def test_attention_maps_of_the_model_against_the_reference(name, monkeypatch):
    """logits are the model's own eval forward; the maps come from ONE tmf_fusion_attn_maps call; probs and received within
    MARGIN x floor_distance(the reference's stored fp32 <-> fp64 distance of the tensor) x max |reference| of the tensor;
    volume() has the input's shape; a model in train mode raises."""
    import transmf_ad_amd as T
    from transmf_ad_amd import _lib
    z = np.load(os.path.join(GOLDEN_DIR, f"attn_maps_{name}.npz"))
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = g.inputs()
    mri, pet = torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)
    with torch.no_grad():
        want_logits = net(mri, pet)[0].clone()
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda fn, *a: (names.append(fn), real(fn, *a))[1])
    maps = T.attention_maps(net, mri, pet, probs=True)
    monkeypatch.undo()
    assert names.count("tmf_fusion_attn_maps") == 1
    assert torch.equal(maps.logits, want_logits)
    depth, B, heads = g.kw["depth"], g.batch, g.kw["heads"]
    N = z["recv"].shape[-1]
    assert maps.grid == tuple(s // 16 for s in g.size) and tuple(maps.received.shape) == (depth, 2, B, heads, N)
    assert tuple(maps.volume().shape) == (B,) + tuple(g.size)
    bad = []
    for got, key in ((maps.probs, "probs"), (maps.received, "recv")):
        want = torch.from_numpy(z[key]).double()
        assert got.shape == want.shape
        for l in range(depth):
            for s in (0, 1):
                err = float((got[l, s].double().cpu() - want[l, s]).abs().max()) / float(want[l, s].abs().max())
                tol = mi.MARGIN * mi.floor_distance(z["dist_" + key][l, s])
                print(f"{name} {key}[{l}, {s}]: err {err:.3e} tol {tol:.3e} err / tol {err / tol:.3f}")
                if not err <= tol:
                    bad.append((key, l, s, f"{err / tol:.3g}"))
    only = T.attention_maps(net, mri, pet)
    assert only.probs is None and torch.equal(only.received, maps.received)
    with pytest.raises(ValueError, match="eval"):
        T.attention_maps(net.train(), mri, pet)
    assert not bad, bad
