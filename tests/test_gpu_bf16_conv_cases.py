"""The rows of tests/_bf16_conv_cases.py on the MI355X, each under its options and only after the library has confirmed the
row's kernel and plan.

Weight gradients: integer operands on which every product and every sum is exact in any order, so dw must EQUAL the fp64
reference in both layouts, whatever a workgroup's walk looks like: a brick dropped, taken twice or fetched from the wrong place
changes an integer.  x, dz, dw and the workspace live in one arena between NaN bands, and the workspace starts as NaN: a halo
chunk fetched from outside a tensor, or a slab element nobody wrote, surfaces as NaN in dw.  One many-brick row per kernel
also runs general operands (in-kernel rounding, fp32 accumulation against fp64).

Forward and data gradient: every instantiation on integer operands thinned until the statistics are exact too.

Each case prints the plan it ran ("BF16CASE ...")."""
import pytest
import torch

import _bf16_conv_cases as K
from _conv_util import _lib, _ops
from test_gpu_bn_reduce import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN_BYTE = 0xFF


def _st():
    return torch.cuda.current_stream().cuda_stream


def _plan(shape, io):
    import ctypes
    ns, tps = ctypes.c_int(-1), ctypes.c_int(-1)
    n = _lib().query("tmf_conv3d_wgrad_bf16_plan", *shape, io, ctypes.addressof(ns), ctypes.addressof(tps))
    return n, ns.value, tps.value


@pytest.fixture
def wrow(request):
    """The row under its wgrad_tr (1 again afterwards); the library must select the row's kernel and plan there."""
    r = request.param
    lib = _lib()
    lib.call("tmf_set_option", b"wgrad_tr", r[0])
    try:
        assert lib.query("tmf_conv3d_wgrad_bf16_kernel_name", *r[2], r[1]).decode() == r[3]
        assert _plan(r[2], r[1]) == (K.ntiles(r[2]), r[4], r[5]) and K.order_of(r[3], r[4]) == r[6]
        yield r
    finally:
        lib.call("tmf_set_option", b"wgrad_tr", 1)


@pytest.fixture
def frow(request):
    """The row under its bf16_v2 and bf16_dma (1 and 1 again afterwards)."""
    r = request.param
    lib = _lib()
    lib.call("tmf_set_option", b"bf16_v2", r[0])
    lib.call("tmf_set_option", b"bf16_dma", r[1])
    try:
        assert lib.query("tmf_conv3d_fwd_bf16_kernel_name", *r[3], r[2]).decode() == r[4]
        yield r
    finally:
        lib.call("tmf_set_option", b"bf16_v2", 1)
        lib.call("tmf_set_option", b"bf16_dma", 1)


def _wgrad_both_layouts(row, x, dz):
    """tmf_conv3d_wgrad_bf16_t in the tap-major and in the reference layout on host tensors x, dz (fp32; sent as the row's
    tensor type) inside one guarded arena, the workspace NaN before each call.  -> (tap-major dw, reference-layout dw)."""
    lib = _lib()
    _tr, io, shape, _kernel, _nsplit, _tps, _order = row
    B, D, H, W, cin, cout = shape
    dt = torch.bfloat16 if io else torch.float32
    nbytes = lib.query("tmf_conv3d_wgrad_bf16_workspace_bytes", *shape)
    a = Arena(dict(x=x.to(dt), dz=dz.to(dt)),
              dict(dw0=((27, cin, cout), torch.float32), dw1=((cout, cin, 3, 3, 3), torch.float32), ws=((nbytes // 4,), torch.float32)))
    off, n = a.slots["ws"][:2]
    for layout, name in ((0, "dw0"), (1, "dw1")):
        a.dev[off:off + n].fill_(NAN_BYTE)
        lib.call("tmf_conv3d_wgrad_bf16_t", a.ptr("x"), a.ptr("dz"), a.ptr(name), a.ptr("ws"), nbytes, B, D, H, W, cin, cout,
                 io, layout, _st())
    res = a.fetch(workspace=("ws",))                 # guards and inputs unchanged, dw0 and dw1 free of NaN
    return res["dw0"], res["dw1"]


@pytest.mark.parametrize("wrow", K.WGRAD_ROWS, ids=K.wgrad_row_id, indirect=True)
def test_weight_gradient_is_exact_over_many_bricks(wrow):
    c = K.wgrad_case(wrow[2])
    lo, hi = K.bricks_per_workgroup(wrow)
    print("BF16CASE {} {} nsplit {} tiles_per_split {} {} step {} bricks per workgroup {}..{}{}".format(
        K.wgrad_row_id(wrow), wrow[3], wrow[4], wrow[5], wrow[6], K.step_of(wrow), lo, hi,
        " (a walk crosses samples)" if K.crosses_sample(wrow) else ""))
    dw0, dw1 = _wgrad_both_layouts(wrow, c["x"], c["dz"])
    assert torch.equal(dw0, c["dw"]), "tap-major: {} entries differ, largest difference {}".format(
        int((dw0 != c["dw"]).sum()), float((dw0 - c["dw"]).abs().max()))
    assert torch.equal(dw1, c["dw_ref"]), "reference layout: {} entries differ".format(int((dw1 != c["dw_ref"]).sum()))


@pytest.mark.parametrize("wrow", K.WGRAD_GENERAL_ROWS, ids=K.wgrad_row_id, indirect=True)
def test_weight_gradient_of_general_operands_over_many_bricks(wrow):
    """Standard-normal operands: within fp32-accumulation accuracy (5e-6 of the largest entry, the gate of
    test_conv3d_wgrad_bf16_mfma, set there for up to 27 648 voxels) of fp64 on the bf16-rounded operands.  The kernels that
    take fp32 tensors round in the kernel: bit-identical to the same call on pre-rounded operands.  (The kernels that take
    bf16 tensors are handed the rounded operands as they are.)"""
    c = K.wgrad_general_case(wrow[2])
    xb, dzb = c["x"].bfloat16().float(), c["dz"].bfloat16().float()
    dw0, dw1 = _wgrad_both_layouts(wrow, xb, dzb)
    err = float((dw0.double() - c["dw"]).abs().max() / c["dw"].abs().max())
    print("BF16CASE {} general operands: error {:.3e} of the largest entry".format(K.wgrad_row_id(wrow), err))
    assert err < 5e-6
    assert torch.equal(K.reference_layout(dw0), dw1)
    if wrow[1] == 0:
        raw0, raw1 = _wgrad_both_layouts(wrow, c["x"], c["dz"])
        assert torch.equal(raw0, dw0) and torch.equal(raw1, dw1)


def _forward(shape, io, xin, wpacked, want_stats):
    """tmf_conv3d_fwd_bf16_t into a NaN-filled z (and NaN-filled statistic rows) -> (z, stat_partial or None)."""
    lib = _lib()
    B, D, H, W, cin, cout = shape
    z = torch.full((B, D, H, W, cout), float("nan"), device=DEV, dtype=torch.bfloat16 if io & 2 else torch.float32)
    part = None
    if want_stats:
        part = torch.full((lib.query("tmf_conv3d_bf16_stat_blocks", B, D, H, W), 2, cout), float("nan"), device=DEV)
    lib.call("tmf_conv3d_fwd_bf16_t", xin.data_ptr(), wpacked.data_ptr(), z.data_ptr(), part.data_ptr() if want_stats else None,
             B, D, H, W, cin, cout, io, _st())
    torch.cuda.synchronize()
    return z.cpu(), (part.cpu() if want_stats else None)


@pytest.mark.parametrize("frow", K.FWD_ROWS, ids=K.fwd_row_id, indirect=True)
def test_forward_statistics_and_data_gradient_are_exact(frow):
    ops, lib = _ops(), _lib()
    _v2, _dma, io, shape, name = frow
    B, D, H, W, cin, cout = shape
    c = K.fwd_case(shape)
    idt, odt = (torch.bfloat16 if io & 1 else torch.float32), (torch.bfloat16 if io & 2 else torch.float32)
    w = c["w"].to(DEV)
    z, part = _forward(shape, io, c["x"].to(idt).to(DEV), ops.pack_weight_bf16(w), True)
    print("BF16CASE {} {} max |z| {:.0f}".format(K.fwd_row_id(frow), name, float(c["z"].abs().max())))
    assert torch.equal(z, c["z"].to(odt)), "{} voxels differ".format(int((z != c["z"].to(odt)).sum()))
    s = part.double().sum(0)
    assert torch.equal(s[0], c["s1"]) and torch.equal(s[1], c["s2"])
    if cout % 8 == 0:
        swapped = (B, D, H, W, cout, cin)
        dname = lib.query("tmf_conv3d_fwd_bf16_kernel_name", *swapped, io).decode()
        assert dname in K.expected_fwd_names() and K.fwd_brick(dname) == K.fwd_brick(name)
        dx, _ = _forward(swapped, io, c["dz"].to(idt).to(DEV), ops.pack_weight_dgrad_bf16(w), False)
        assert torch.equal(dx, c["dx"].to(odt)), "data gradient ({}): {} voxels differ".format(dname, int((dx != c["dx"].to(odt)).sum()))
