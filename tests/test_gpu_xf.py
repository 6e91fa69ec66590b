"""The one-call fusion entries at dim 128 called on their own (tmf_fusion_train_fwd / _train_bwd / _infer_fwd through _lib.call
with raw pointers, nothing of ops.py in between) against the fp64 reference of tests/_xf_inputs.py: csrc/xformer_fused.hip at
4 heads of 32 and at 8 heads of 16, and one launch per op (TMF_FUSION_PER_OP) on the same inputs, reference and tolerances -
if both paths fail alike, suspect the reference; if one fails, the failure names the kernel family.

The cases are the shapes that reach each boundary of the fused kernels (XF_CASES says which); the layer-0 instances have flat,
peaked, low (every logit near -100) and high (every logit near +100) query rows in one tensor.

cls is judged per batch row, the mean half and the max half apart; the token gradients per token row and class, the Gaussian
columns and the reserved columns apart; every weight gradient per weight row; `small` and `lnf` per segment:
    |kernel - fp64| <= margin x floor_distance(XF_DISTANCE[case, heads][quantity, class]) x scale of the row
(xf_row_errors and xf_tolerance of tests/_xf_inputs.py have the scales and say where a scale is the sum of the terms' magnitudes;
the module docstring there says what the mean half of cls cannot see).  No kernel had to change: the first runs failed alike on
the fused kernels and on one launch per op, in the sums that are zero only because every row of dS sums to zero, and what
was wrong were the yardstick's scales and its backward, which was handed the forward's own P (_Arith, xf_row_errors).
Every buffer lives in the Arena of tests/test_gpu_bn_reduce.py: `saved`, the backward's scratch and the forward-only workspace
are slots of exactly the size their query names, every byte outside the outputs and workspaces (the inputs included) must be
unchanged, every output element written and finite."""
import ctypes
import functools

import pytest
import torch

import _xf_inputs as xi
from test_gpu_bn_reduce import Arena, _st

pytestmark = pytest.mark.gpu
F32, U8 = torch.float32, torch.uint8
MODES = {"4x32": ((4, 32), False), "8x16": ((8, 16), False), "per-op": ((4, 32), True)}
GRADS = ("small", "lnf") + xi.WEIGHTS                 # the fields of tmf_xformer_grads


@functools.lru_cache(maxsize=None)
def _case(case, heads):
    """Inputs and fp64 reference of one case (shared by the modes; never modified)."""
    inp = xi.xf_inputs(case, heads)
    ref = xi.xf_ref(inp, heads)
    del ref["fwd"]
    return inp, ref


def _grad_shapes(heads):
    inner = heads[0] * heads[1]
    return dict(small=(6 * xi.DIM + xi.MLP,), lnf=(2 * xi.DIM,), dwq=(inner, xi.DIM), dwkv=(2 * inner, xi.DIM), dwo=(xi.DIM, inner),
                dw1=(xi.MLP, xi.DIM), dw2=(xi.DIM, xi.MLP))


def _run(case, heads, per_op):
    """The three entries of one case on one arena: the training forward twice (each into a `saved` of its own), the
    forward-only entry, the backward twice on the FIRST forward's saved (the second time on a scratch the first left dirty).
    -> {name: host tensor}, the second call's results under name + "_again", the forward-only cls under "cls_infer"."""
    from transmf_ad_amd import _lib as L
    B, N, depth, _masks = case
    h, dh = heads
    inp, _ref = _case(case, heads)
    d = L.FusionDesc(B=B, N=N, dim=xi.DIM, heads=h, dim_head=dh, mlp=xi.MLP, depth=depth, flags=L.FUSION_PER_OP if per_op else 0)
    assert L.query("tmf_fusion_uses_fused", ctypes.byref(d)) == (0 if per_op else 1)
    n_saved = L.query("tmf_fusion_saved_bytes", ctypes.byref(d))
    n_scratch = L.query("tmf_fusion_bwd_scratch_bytes", ctypes.byref(d))
    n_ws = L.query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d))
    assert min(n_saved, n_scratch, n_ws) > 0
    n_inst = 2 * depth
    ins = dict(mri=inp["mri"], pet=inp["pet"], dcls=inp["dcls"])
    for k, p in enumerate(inp["params"]):
        ins.update({f"p{k}.{name}": p[name] for name in xi.PARAM_NAMES})
        if inp["masks"] is not None:
            ins.update({f"m{k}.{j}": m for j, m in enumerate(inp["masks"][k])})
    outs = {"cls": ((B, 4 * xi.DIM), F32), "cls_again": ((B, 4 * xi.DIM), F32), "cls_infer": ((B, 4 * xi.DIM), F32)}
    for tag in ("", "_again"):
        outs["dmri_tok" + tag] = outs["dpet_tok" + tag] = ((B, N, xi.DIM), F32)
        for k in range(n_inst):
            outs.update({f"i{k}.{name}{tag}": (shape, F32) for name, shape in _grad_shapes(heads).items()})
    workspaces = {"saved": n_saved, "saved_again": n_saved, "scratch": n_scratch, "ws": n_ws}
    outs.update({name: ((n,), U8) for name, n in workspaces.items()})
    arena = Arena(ins, outs)
    p = arena.ptr
    inst = (L.XformerParams * n_inst)()
    for k in range(n_inst):
        for name in xi.PARAM_NAMES:
            setattr(inst[k], name, p(f"p{k}.{name}"))
        inst[k].eps1 = inst[k].eps2 = inst[k].epsf = xi.EPS
        if inp["masks"] is not None:
            inst[k].mask_o, inst[k].mask_g, inst[k].mask_f = (p(f"m{k}.{j}") for j in range(3))
    for tag in ("", "_again"):
        L.call("tmf_fusion_train_fwd", ctypes.byref(d), p("mri"), p("pet"), inst, p("saved" + tag), n_saved, p("cls" + tag), _st())
    L.call("tmf_fusion_infer_fwd", ctypes.byref(d), p("mri"), p("pet"), inst, p("ws"), n_ws, p("cls_infer"), _st())
    for tag in ("", "_again"):
        grads = (L.XformerGrads * n_inst)()
        for k in range(n_inst):
            for name in GRADS:
                setattr(grads[k], name, p(f"i{k}.{name}{tag}"))
        L.call("tmf_fusion_train_bwd", ctypes.byref(d), p("mri"), p("pet"), inst, p("saved"), n_saved, p("dcls"), grads,
               p("dmri_tok" + tag), p("dpet_tok" + tag), p("scratch"), n_scratch, _st())
    # finiteness is judged below, per row and class; here: every output element written, every other byte unchanged
    return arena.fetch(may_nan=tuple(n for n in outs if n not in workspaces), workspace=tuple(workspaces))


def _offenders(got, ref, case, heads):
    """[(quantity, class, rows beyond their tolerance or not finite)] - token rows as (batch element, token)."""
    cls = xi.xf_class(case[1])
    bad = []
    for key, rel in xi.xf_row_errors(got, ref).items():
        hit = (~(rel <= xi.xf_tolerance(case, heads, key))).nonzero().tolist()
        if hit and key[0].startswith(("dmri_tok", "dpet_tok")):
            rows = (cls == xi.XF_CLASSES.index(key[1])).nonzero().flatten().tolist()
            hit = [(b, rows[i]) for b, i in hit]
        if hit:
            bad.append((key[0], key[1], f"{len(hit)} rows, the first {hit[:6]}", f"worst err {float(rel.max()):.3g}"))
    return bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", xi.XF_CASES, ids=xi.case_id)
def test_fusion_entries_against_fp64(case, mode):
    """tmf_fusion_uses_fused is 1 for the two fused modes and 0 for one launch per op; the forward called twice gives a
    bit-identical cls, the forward-only entry the same bits again; the backward called twice on the first forward's `saved`
    gives bit-identical gradients; nothing outside the outputs and the three workspaces is written; then every output is finite
    and within its per-row tolerance (the worst err / tol per quantity and class is printed)."""
    heads, per_op = MODES[mode]
    back = _run(case, heads, per_op)
    _inp, ref = _case(case, heads)
    got = {n: back[n] for n in back if n in ref}
    assert torch.equal(back["cls"].view(torch.int32), back["cls_again"].view(torch.int32)), "cls: two forward calls differ"
    assert torch.equal(back["cls"].view(torch.int32), back["cls_infer"].view(torch.int32)), "cls: the forward-only entry differs"
    for n in got:
        if n != "cls":
            assert torch.equal(back[n].view(torch.int32), back[n + "_again"].view(torch.int32)), f"{n}: two backward calls differ"
    for key, ratio in xi.xf_ratios(got, ref, case, heads).items():
        print(f"{xi.case_id(case)} {mode} {key[0]} {key[1]}: err / tol {ratio:.3f}")
    bad = _offenders(got, ref, case, heads)
    assert not bad, f"{case} {mode}: beyond their tolerance or not finite: {bad}"
