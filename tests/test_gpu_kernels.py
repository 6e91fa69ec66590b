"""Kernel-level parity (MI355X): every entry point of libtmf_hip.so, called through the
C ABI wrappers in transmf_ad_amd.ops, against the CPU oracle's ops (stock torch fp32/fp64 on
the host) on the same seeded inputs.  Tolerances are fp32-roundoff class and stated per test.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _conv_util import _ncdhw, _ndhwc, _ops, _rand, _relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(params=[(0, 1), (2, 1), (2, 0)], ids=["small-brick", "8x8x8-brick", "8x8x8-brick-register-staged"])
def bf16_kernel_choice(request):
    """Run a test with the bf16 forward kernel forced to the 4x8x8-brick variant (0) and to the 8x8x8-brick, 2 x NT
    register-tile variant (2; with bf16 tensors in its LDS-DMA form, and with that switched off); the default (1) picks by
    brick count."""
    from transmf_ad_amd import _lib
    _lib.call("tmf_set_option", b"bf16_v2", request.param[0])
    _lib.call("tmf_set_option", b"bf16_dma", request.param[1])
    yield request.param[0]
    _lib.call("tmf_set_option", b"bf16_v2", 1)
    _lib.call("tmf_set_option", b"bf16_dma", 1)


CONV_SHAPES = [
    # B, D, H, W, cin, cout, k
    (2, 8, 8, 8, 8, 8, 3),
    (1, 5, 7, 9, 16, 32, 3),          # ragged: bricks overhang on every axis
    (2, 16, 16, 16, 32, 64, 3),       # L64 config, full bricks
    (1, 17, 16, 19, 32, 32, 3),       # L32 config, ragged
    (1, 12, 12, 12, 128, 256, 3),     # S128 config, 4 cin chunks, 2 cout blocks
    (1, 12, 12, 12, 256, 128, 1),     # 1x1x1
    (2, 24, 24, 24, 64, 128, 3),      # L64, 2 cin chunks, 2 cout blocks
    (1, 6, 5, 4, 6, 10, 3),           # channel counts not multiples of 4 (scalar path)
    (1, 4, 4, 4, 40, 72, 3),          # cin > 32 with a partial last chunk; partial cout tile
    (2, 3, 2, 2, 16, 16, 1),
    (1, 9, 10, 11, 1, 32, 3),         # first layer (cin = 1)
    (2, 8, 8, 8, 1, 8, 3),
    (1, 33, 7, 5, 1, 40, 3),
]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3d_fwd_and_stats(shape):
    ops = _ops()
    B, D, H, W, cin, cout, k = shape
    x = _rand(B, cin, D, H, W, seed=1)
    w = _rand(cout, cin, k, k, k, seed=2, scale=(cin * k ** 3) ** -0.5)
    ref = F.conv3d(x.double(), w.double(), padding=k // 2)
    xg = _ndhwc(x).to(DEV)
    z, part, nblk = ops.conv3d_raw(xg, ops.pack_weight(w.to(DEV)), cin, cout, k, True)
    torch.cuda.synchronize()
    got = _ncdhw(z.cpu())
    assert _relerr(got, ref) < 1e-5          # fp32 accumulation over K = 27*cin terms (K up to 3456)
    s = part.double().sum(0).cpu()
    r = ref.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    assert (s[0] - r.sum(1)).abs().max() <= 1e-4 * max(1.0, r.abs().sum(1).max().item())
    assert (s[1] - (r * r).sum(1)).abs().max() <= 1e-5 * (r * r).sum(1).max().item()


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv3d_wgrad_and_dgrad(shape):
    ops = _ops()
    B, D, H, W, cin, cout, k = shape
    x = _rand(B, cin, D, H, W, seed=3).double().requires_grad_(True)
    w = _rand(cout, cin, k, k, k, seed=4, scale=(cin * k ** 3) ** -0.5).double().requires_grad_(True)
    dz = _rand(B, cout, D, H, W, seed=5)
    F.conv3d(x, w, padding=k // 2).backward(dz.double())
    xg, dzg = _ndhwc(x.detach().float()).to(DEV), _ndhwc(dz).to(DEV)
    dw = ops.unpack_wgrad(ops.conv3d_wgrad(xg, dzg, cin, cout, k), cout, cin, k)
    assert _relerr(dw, w.grad) < 5e-6
    # TMF_DW_REFERENCE: the final reduction stores the nn.Conv3d layout itself — bit-identical values
    assert torch.equal(ops.conv3d_wgrad(xg, dzg, cin, cout, k, reference_layout=True), dw)
    if cin > 1:
        dx, _, _ = ops.conv3d_raw(dzg, ops.pack_weight_dgrad(w.detach().float().to(DEV)), cout, cin, k, False)
        assert _relerr(_ncdhw(dx.cpu()), x.grad) < 1e-5


RT_SHAPES = [
    # volumes the 6 x 6 x 12 bricks of the register-tiled forward kernel tile exactly: B, D, H, W, cin, cout
    (1, 6, 6, 12, 16, 16),            # one brick, one 16-channel tile (RtCfg<1>)
    (2, 12, 6, 24, 32, 48),           # 48 output channels: 16-channel workgroups
    (1, 12, 12, 12, 128, 256),        # the model's 12^3 layer: 8 chunks
    (8, 24, 24, 24, 64, 64),          # 256 bricks x 2: RtCfg<2>, the model's 24^3 layer
    (2, 18, 12, 36, 16, 32),
]


@pytest.mark.parametrize("shape", RT_SHAPES)
def test_register_tiled_conv_matches_fp64_and_the_ring_kernel(shape):
    """The register-tiled forward / data-gradient kernel (conv3d_fwd_rt_kernel: 6x6x12 bricks, 7 x NT tiles of
    v_mfma_f32_16x16x4_f32 per wave) against fp64 — z, the BatchNorm statistic partials, the data gradient through the same
    kernel — and against the ring kernel on the same inputs (tmf_set_option("conv_rt", 0)): same sums up to fp32 order."""
    ops = _ops()
    from transmf_ad_amd import _lib
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=11)
    w = _rand(cout, cin, 3, 3, 3, seed=12, scale=(cin * 27) ** -0.5)
    ref = F.conv3d(x.double(), w.double(), padding=1)
    xg, wp = _ndhwc(x).to(DEV), ops.pack_weight(w.to(DEV))
    try:
        _lib.call("tmf_set_option", b"conv_rt", 1)
        assert _lib.query("tmf_conv3d_fwd_kernel_name", B, D, H, W, cin, cout, 3).decode().startswith("RtCfg")
        z, part, nblk = ops.conv3d_raw(xg, wp, cin, cout, 3, True)
        assert nblk == B * (D // 6) * (H // 6) * (W // 12)
        _lib.call("tmf_set_option", b"conv_rt", 0)
        assert not _lib.query("tmf_conv3d_fwd_kernel_name", B, D, H, W, cin, cout, 3).decode().startswith("RtCfg")
        z0, part0, _ = ops.conv3d_raw(xg, wp, cin, cout, 3, True)
        _lib.call("tmf_set_option", b"conv_rt", 2)
        torch.cuda.synchronize()
        assert _relerr(_ncdhw(z.cpu()), ref) < 1e-5
        assert (z - z0).abs().max().item() <= 2e-5 * ref.abs().max().item()
        s = part.double().sum(0).cpu()
        r = ref.permute(1, 0, 2, 3, 4).reshape(cout, -1)
        assert (s[0] - r.sum(1)).abs().max() <= 1e-4 * max(1.0, r.abs().sum(1).max().item())
        assert (s[1] - (r * r).sum(1)).abs().max() <= 1e-5 * (r * r).sum(1).max().item()
        # the statistic partials are those of the z the kernel stored
        zc = z.double().reshape(-1, cout)
        assert (part.double().sum(0)[0] - zc.sum(0)).abs().max().item() <= 1e-4 * max(1.0, zc.abs().sum(0).max().item())
        # data gradient through the same kernel; and run to run bitwise
        dz = _rand(B, cout, D, H, W, seed=13)
        xr = x.double().requires_grad_(True)
        F.conv3d(xr, w.double(), padding=1).backward(dz.double())
        wd = ops.pack_weight_dgrad(w.to(DEV))
        dx, _, _ = ops.conv3d_raw(_ndhwc(dz).to(DEV), wd, cout, cin, 3, False)
        assert _relerr(_ncdhw(dx.cpu()), xr.grad) < 1e-5
        z2, part2, _ = ops.conv3d_raw(xg, wp, cin, cout, 3, True)
        assert torch.equal(z2, z) and torch.equal(part2, part)
    finally:
        _lib.call("tmf_set_option", b"conv_rt", 0)


def test_mfma_layout_is_transpose_sensitive():
    """A = I-like probe with an asymmetric weight: catches swapped rows/columns of the MFMA fragments."""
    ops = _ops()
    cin, cout = 32, 64
    x = torch.zeros(1, cin, 8, 8, 8)
    x[0, :, 3, 4, 5] = torch.arange(cin, dtype=torch.float32) + 1
    w = torch.zeros(cout, cin, 3, 3, 3)
    for co in range(cout):
        for ci in range(cin):
            w[co, ci, 1, 1, 1] = (co * 37 + ci * 11) % 23 - 7.0
    w[:, :, 0, 1, 2] = 0.5
    ref = F.conv3d(x, w, padding=1)
    z, _, _ = ops.conv3d_raw(_ndhwc(x).to(DEV), ops.pack_weight(w.to(DEV)), cin, cout, 3, False)
    assert torch.equal(_ncdhw(z.cpu()), ref)      # small integers: exact


BLOCK_CASES = [
    # B, D, H, W, cin, cout, k, pool
    (2, 8, 8, 8, 8, 16, 3, "max"),
    (3, 7, 9, 5, 8, 8, 3, "max"),         # odd sizes: floor-mode pooling drops the last plane
    (2, 6, 6, 6, 16, 32, 3, None),
    (2, 4, 6, 5, 32, 16, 1, "avg"),
    (2, 10, 9, 8, 1, 8, 3, "max"),        # first layer (fused recompute path: conv output never stored)
    (1, 13, 17, 11, 1, 32, 3, "max"),     # first layer, every brick ragged, odd pooling edges
    (2, 8, 16, 24, 1, 40, 3, "max"),      # first layer, two channel tiles
    (1, 12, 24, 24, 1, 32, 3, "max"),     # first layer with an interior brick (mask-free buffer loads) next to face bricks
    (1, 6, 6, 6, 1, 8, 3, None),          # first layer without pool -> generic (stored-z) path
    (1, 5, 4, 3, 6, 10, 3, "max"),        # scalar channel path
    (2, 16, 16, 16, 32, 64, 3, "max"),
    (8, 22, 27, 22, 64, 64, 3, "max"),    # the reference's third level at batch 8: plan_fwd takes the 4x4x8 half brick
    (8, 11, 13, 11, 128, 256, 3, None),   # ... and its fourth: 64-channel instance of the 4x4x4-brick kernel (fwd and dgrad)
]


def _block_ref(x, w, b, g, be, rm, rv, train, pool, dtype):
    x = x.to(dtype).requires_grad_(True)
    P = [t.to(dtype).requires_grad_(True) for t in (w, b, g, be)]
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    z = F.conv3d(x, P[0], P[1], padding=w.shape[2] // 2)
    y = F.leaky_relu(F.batch_norm(z, rm, rv, P[2], P[3], train, 0.1, 1e-5), 0.01)
    if pool == "max":
        y = F.max_pool3d(y, 2, 2)
    elif pool == "avg":
        y = F.avg_pool3d(y, 2, 2)
    return x, P, rm, rv, y


@pytest.mark.parametrize("case", BLOCK_CASES)
@pytest.mark.parametrize("train", [True, False])
def test_conv_bn_act_pool_block(case, train):
    """One full sNet block, forward + backward, train and eval mode, vs fp64 torch on the host."""
    ops = _ops()
    B, D, H, W, cin, cout, k, pool = case
    x = _rand(B, cin, D, H, W, seed=11)
    w = _rand(cout, cin, k, k, k, seed=12, scale=(cin * k ** 3) ** -0.5)
    b = _rand(cout, seed=13, scale=0.1)
    g = 1 + _rand(cout, seed=14, scale=0.1)
    be = _rand(cout, seed=15, scale=0.1)
    rm = _rand(cout, seed=16, scale=0.1)
    rv = 1 + _rand(cout, seed=17, scale=0.1).abs()
    xr, P, rm_ref, rv_ref, yr = _block_ref(x, w, b, g, be, rm, rv, train, pool, torch.float64)
    go = _rand(*yr.shape, seed=18)
    if pool is None:
        # LeakyReLU' jumps at zero: an fp32 pre-activation a few 1e-6 from 0 can land on the other side than the fp64
        # reference's, and ONE such element moves the weight gradient by ~1 % of its maximum (seen with the Winograd
        # form's other rounding at 128 -> 256 channels).  No upstream gradient where the reference itself is ambiguous.
        go = go * (yr.detach().abs() > 1e-6).float()
    if yr.numel():
        yr.backward(go.double())

    xg = _ndhwc(x).to(DEV).requires_grad_(cin > 1)
    Pg = [t.clone().to(DEV).requires_grad_(True) for t in (w, b, g, be)]
    rmg, rvg = rm.clone().to(DEV), rv.clone().to(DEV)
    yg = ops.conv_bn_act_pool(xg, Pg[0], Pg[1], Pg[2], Pg[3], rmg, rvg, train, pool=pool)
    assert tuple(yg.shape) == tuple(_ndhwc(yr).shape)
    if yr.numel() == 0:
        return
    assert _relerr(_ncdhw(yg.detach().cpu()), yr.detach()) < 2e-5
    yg.backward(_ndhwc(go).to(DEV))
    torch.cuda.synchronize()
    if train:
        assert _relerr(rmg, rm_ref) < 1e-5 and _relerr(rvg, rv_ref) < 1e-5
    assert _relerr(Pg[0].grad, P[0].grad) < 5e-4, "dweight"
    assert _relerr(Pg[2].grad, P[2].grad) < 5e-4, "dgamma"
    assert _relerr(Pg[3].grad, P[3].grad) < 5e-4, "dbeta"
    if train:   # exactly zero in exact arithmetic
        assert Pg[1].grad.abs().max().item() == 0.0
        assert P[1].grad.abs().max().item() < 1e-9
    else:
        assert _relerr(Pg[1].grad, P[1].grad) < 5e-4, "dbias"
    if cin > 1:
        assert _relerr(_ncdhw(xg.grad.cpu()), xr.grad) < 5e-4, "dx"


@pytest.mark.parametrize("shape", [(2, 16, 16, 16, 32), (1, 10, 13, 9, 24), (2, 32, 32, 32, 32)])
def test_first_block_in_bf16_mode(shape):
    """Fused Conv3d(1->C) block with both products on the bf16 matrix cores.  Inputs and weights that ARE bf16
    numbers make the convolution exact, so the forward (statistics, activation, pooling) is held to fp32 accuracy
    against fp64; the weight gradient additionally rounds dz to bf16 (<= 2^-9 relative per element)."""
    ops = _ops()
    B, D, H, W, C = shape
    x = _rand(B, 1, D, H, W, seed=131).abs().bfloat16().float()
    w = _rand(C, 1, 3, 3, 3, seed=132, scale=27 ** -0.5).bfloat16().float()
    b, g, be = _rand(C, seed=133, scale=0.1), 1 + _rand(C, seed=134, scale=0.1), _rand(C, seed=135, scale=0.1)
    rm, rv = _rand(C, seed=136, scale=0.1), 1 + _rand(C, seed=137, scale=0.1).abs()
    xr, P, rm_ref, rv_ref, yr = _block_ref(x, w, b, g, be, rm, rv, True, "max", torch.float64)
    go = _rand(*yr.shape, seed=138)
    yr.backward(go.double())
    ops.set_conv_precision("bf16")
    try:
        Pg = [t.clone().to(DEV).requires_grad_(True) for t in (w, b, g, be)]
        rmg, rvg = rm.clone().to(DEV), rv.clone().to(DEV)
        yg = ops.conv_bn_act_pool(_ndhwc(x).to(DEV), Pg[0], Pg[1], Pg[2], Pg[3], rmg, rvg, True, pool="max")
        yg.backward(_ndhwc(go).to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision("fp32")
    assert _relerr(_ncdhw(yg.detach().cpu()), yr.detach()) < 2e-5
    assert _relerr(rmg, rm_ref) < 1e-5 and _relerr(rvg, rv_ref) < 1e-5
    assert _relerr(Pg[2].grad, P[2].grad) < 5e-4 and _relerr(Pg[3].grad, P[3].grad) < 5e-4      # fp32 reductions
    assert _relerr(Pg[0].grad, P[0].grad) < 1e-2                                                # dz rounded to bf16
    assert Pg[1].grad.abs().max().item() == 0.0


EVAL_EXTRA = [
    (1, 24, 24, 24, 64, 128, 3, "max"),    # two output-channel groups, cross-wave h pairs
    (1, 18, 20, 22, 32, 32, 3, "max"),     # ragged 4x8x8 bricks, odd pooled edge in no dimension, partial bricks
    (1, 17, 19, 21, 32, 64, 3, "max"),     # odd sizes: floor-mode pooling drops the last plane / row / column
    (1, 12, 12, 12, 128, 256, 3, None),    # 4x4x4 bricks x 128 channels (conv4.0)
    (2, 12, 12, 12, 256, 128, 1, "avg"),   # 1x1x1 + average pool (conv4.3)
    (1, 12, 10, 14, 128, 128, 3, "max"),   # 4x4x4 bricks with pooling (h pairs inside one lane)
    (1, 16, 16, 16, 32, 32, 3, None),
]


def _winograd_takes(case):
    """At conv_wino >= 2 the block's fused eval form is tmf_conv3d_fwd_wino_affine, not the direct kernel's epilogue."""
    B, D, H, W, cin, cout, k, pool = case
    return k == 3 and cin % 8 == 0 and cout % 32 == 0 and pool != "avg"


# Every case at the default conv_wino 3 (ids case0, case1, ... as before); the cases Winograd takes there once more at
# conv_wino 0, on tmf_conv3d_fwd_affine — but for the two batch-8 ones, whose brick geometries tests/test_gpu_conv_variants.py
# runs at a fraction of the size.  (The other cases run the same kernels under either setting.)
EVAL_CASES = [pytest.param(c, 3, id="case{}".format(i)) for i, c in enumerate(BLOCK_CASES + EVAL_EXTRA)] + [
    pytest.param(c, 0, id="case{}-direct".format(i)) for i, c in enumerate(BLOCK_CASES + EVAL_EXTRA) if _winograd_takes(c) and c[0] != 8]


@pytest.fixture
def conv_wino(request):
    from transmf_ad_amd import _lib
    _lib.call("tmf_set_option", b"conv_wino", request.param)
    yield request.param
    _lib.call("tmf_set_option", b"conv_wino", 3)


@pytest.mark.parametrize("case,conv_wino", EVAL_CASES, indirect=["conv_wino"])
def test_eval_block_single_pass(case, conv_wino):
    """Inference form (no_grad, eval): conv + folded BN + LeakyReLU + pool in one kernel, against fp64 on the host
    and against the two-pass path on the same data."""
    ops = _ops()
    B, D, H, W, cin, cout, k, pool = case
    assert ops.conv_wino_mode() == conv_wino
    if conv_wino == 0:
        assert ops.wino_ok(cin, cout)             # a case the default setting sends to the Winograd kernel
    if cin == 1 or cin % 4 or cout % 4:
        pytest.skip("single-pass eval kernel needs cin > 1 and channel counts that are multiples of 4")
    x = _rand(B, cin, D, H, W, seed=141)
    w = _rand(cout, cin, k, k, k, seed=142, scale=(cin * k ** 3) ** -0.5)
    b, g, be = _rand(cout, seed=143, scale=0.1), 1 + _rand(cout, seed=144, scale=0.1), _rand(cout, seed=145, scale=0.1)
    rm, rv = _rand(cout, seed=146, scale=0.1), 1 + _rand(cout, seed=147, scale=0.1).abs()
    _, _, _, _, yr = _block_ref(x, w, b, g, be, rm, rv, False, pool, torch.float64)
    args = [t.to(DEV) for t in (w, b, g, be, rm, rv)]
    with torch.no_grad():
        y1 = ops.conv_bn_act_pool(_ndhwc(x).to(DEV), *args, False, pool=pool)
        ops.FUSE_EVAL_BLOCKS = False
        try:
            y2 = ops.conv_bn_act_pool(_ndhwc(x).to(DEV), *args, False, pool=pool)
        finally:
            ops.FUSE_EVAL_BLOCKS = True
    torch.cuda.synchronize()
    assert tuple(y1.shape) == tuple(_ndhwc(yr).shape)
    if yr.numel() == 0:
        return
    assert _relerr(_ncdhw(y1.cpu()), yr.detach()) < 2e-5
    assert _relerr(y1, y2.cpu()) < 5e-6       # (with conv_rt on, the two-pass path runs another fp32 summation order, K up to 3456)


def test_two_blocks_with_bf16_activation_storage(bf16_kernel_choice):
    """Two chained blocks (32->32 no pool, 32->64 max pool) with bf16 tensors between and inside them, forward and
    backward, against fp64 on the host: bf16-operand accuracy (one extra 2^-9 rounding per stored tensor)."""
    ops = _ops()
    B, S = 2, 16
    x = _rand(B, 32, S, S, S, seed=171)
    w1 = _rand(32, 32, 3, 3, 3, seed=172, scale=(32 * 27) ** -0.5)
    w2 = _rand(64, 32, 3, 3, 3, seed=173, scale=(32 * 27) ** -0.5)
    P1 = [_rand(32, seed=174, scale=0.1), 1 + _rand(32, seed=175, scale=0.1), _rand(32, seed=176, scale=0.1)]
    P2 = [_rand(64, seed=177, scale=0.1), 1 + _rand(64, seed=178, scale=0.1), _rand(64, seed=179, scale=0.1)]
    rm1, rv1, rm2, rv2 = torch.zeros(32), torch.ones(32), torch.zeros(64), torch.ones(64)
    xr, Q1, _, _, y1 = _block_ref(x, w1, *P1, rm1, rv1, True, None, torch.float64)
    w2d = w2.double().requires_grad_(True)
    g2, b2 = P2[1].double().requires_grad_(True), P2[2].double().requires_grad_(True)
    y2 = F.max_pool3d(F.leaky_relu(F.batch_norm(F.conv3d(y1, w2d, P2[0].double(), padding=1), rm2.double(), rv2.double(),
                                                 g2, b2, True, 0.1, 1e-5), 0.01), 2, 2)
    go = _rand(*y2.shape, seed=180)
    y2.backward(go.double())
    ops.set_conv_precision("bf16")
    ops.set_activation_storage("bf16")
    try:
        xg = _ndhwc(x).to(DEV).bfloat16().requires_grad_(True)
        A1 = [t.clone().to(DEV).requires_grad_(True) for t in (w1, *P1)]
        A2 = [t.clone().to(DEV).requires_grad_(True) for t in (w2, *P2)]
        h = ops.conv_bn_act_pool(xg, A1[0], A1[1], A1[2], A1[3], rm1.to(DEV), rv1.to(DEV), True, pool=None, out_bf16=True)
        assert h.dtype == torch.bfloat16
        yg = ops.conv_bn_act_pool(h, A2[0], A2[1], A2[2], A2[3], rm2.to(DEV), rv2.to(DEV), True, pool="max", out_bf16=False)
        assert yg.dtype == torch.float32
        yg.backward(_ndhwc(go).to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_activation_storage("fp32")
        ops.set_conv_precision("fp32")
    assert _relerr(_ncdhw(yg.detach().cpu()), y2.detach()) < 3e-2

    def l2(got, ref):
        return ((got.double().cpu() - ref).norm() / ref.norm()).item()
    assert xg.grad.dtype == torch.bfloat16
    # bf16 noise (4e-3 of z) flips max-pool / LeakyReLU decisions on random data: gradients are compared in L2
    assert l2(A2[0].grad, w2d.grad) < 2e-1 and l2(A1[0].grad, Q1[0].grad) < 2e-1
    assert l2(A2[2].grad, g2.grad) < 2e-1 and l2(_ncdhw(xg.grad.float().cpu()), xr.grad) < 2e-1


def test_maxpool_first_argmax_on_ties():
    """Ties inside a pooling window route the gradient to the FIRST maximum in (d,h,w) order (torch)."""
    ops = _ops()
    B, D, H, W, C = 1, 4, 4, 4, 8
    z = torch.zeros(B, D, H, W, C)
    z[0, 0, 1, 0] = 1.0
    z[0, 1, 0, 1] = 1.0        # same window (0,0,0), later in scan order
    scale, shift = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    zg = z.to(DEV)
    dout = torch.ones(B, 2, 2, 2, C, device=DEV)
    from transmf_ad_amd import _lib
    dz = torch.empty_like(zg)
    coef = torch.zeros(2, C, device=DEV)
    mean, invstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    _lib.call("tmf_bn_act_pool_bwd_apply", zg.data_ptr(), dout.data_ptr(), scale.data_ptr(),
              shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), dz.data_ptr(),
              B, D, H, W, C, _lib.POOL_MAX2, 0.01, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    zr = z.permute(0, 4, 1, 2, 3).clone().requires_grad_(True)
    F.max_pool3d(F.leaky_relu(zr, 0.01), 2, 2).sum().backward()
    assert torch.equal(_ncdhw(dz.cpu()), zr.grad)


ATTN_CASES = [
    # B, heads, N, M, dh
    (2, 4, 8, 8, 8),
    (1, 4, 27, 27, 32),
    (2, 4, 216, 216, 32),
    (1, 2, 100, 37, 16),        # N != M, ragged tiles
    (1, 2, 130, 200, 64),
    (1, 1, 40, 600, 32),        # keys exceed one LDS super-block (online softmax across blocks)
    (1, 1, 600, 40, 32),        # queries exceed one super-block in the dK/dV kernel
    (1, 4, 512, 512, 32),       # 128^3 token count
]


def _attn_ref(q, kv, heads, scale):
    B, N, inner = q.shape
    M = kv.shape[1]
    dh = inner // heads
    k, v = kv[..., :inner], kv[..., inner:]
    qh = q.reshape(B, N, heads, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, M, heads, dh).permute(0, 2, 1, 3)
    vh = v.reshape(B, M, heads, dh).permute(0, 2, 1, 3)
    att = torch.softmax(qh @ kh.transpose(-1, -2) * scale, dim=-1)
    return (att @ vh).permute(0, 2, 1, 3).reshape(B, N, inner)


@pytest.mark.parametrize("case", ATTN_CASES)
def test_cross_attention(case):
    ops = _ops()
    B, heads, N, M, dh = case
    inner = heads * dh
    q = _rand(B, N, inner, seed=21)
    kv = _rand(B, M, 2 * inner, seed=22)
    go = _rand(B, N, inner, seed=23)
    scale = dh ** -0.5
    qr, kvr = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    ref = _attn_ref(qr, kvr, heads, scale)
    ref.backward(go.double())
    qg, kvg = q.to(DEV).requires_grad_(True), kv.to(DEV).requires_grad_(True)
    out = ops.cross_attention(qg, kvg, heads, scale)
    out.backward(go.to(DEV))
    torch.cuda.synchronize()
    assert _relerr(out.detach(), ref.detach()) < 5e-6
    assert _relerr(qg.grad, qr.grad) < 2e-5
    assert _relerr(kvg.grad, kvr.grad) < 2e-5


def test_cross_attention_spiked_key():
    """One key dominates a row at a late chunk: forces the online-softmax rescale branch."""
    ops = _ops()
    B, heads, N, M, dh = 1, 1, 64, 300, 32
    q = _rand(B, N, dh, seed=31)
    kv = _rand(B, M, 2 * dh, seed=32)
    kv[0, 260, :dh] = q[0, 5] * 6.0           # huge score for query 5 at key 260 (third chunk)
    ref = _attn_ref(q.double(), kv.double(), heads, dh ** -0.5)
    out = ops.cross_attention(q.to(DEV), kv.to(DEV), heads, dh ** -0.5)
    assert _relerr(out, ref) < 5e-6


@pytest.mark.parametrize("rows,dim", [(16, 32), (1728, 128), (5, 36), (7, 30), (33, 512)])
def test_layer_norm(rows, dim):
    ops = _ops()
    x = _rand(rows, dim, seed=41) * 2 + 0.5
    g, b = 1 + _rand(dim, seed=42, scale=0.1), _rand(dim, seed=43, scale=0.1)
    go = _rand(rows, dim, seed=44)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, g, b))
    F.layer_norm(xr, (dim,), gr, br, 1e-5).backward(go.double())
    xg, gg, bg = (t.to(DEV).requires_grad_(True) for t in (x, g, b))
    y = ops.layer_norm(xg, gg, bg, 1e-5)
    y.backward(go.to(DEV))
    assert _relerr(y.detach(), F.layer_norm(x.double(), (dim,), g.double(), b.double(), 1e-5)) < 2e-6
    assert _relerr(xg.grad, xr.grad) < 1e-5
    assert _relerr(gg.grad, gr.grad) < 1e-5
    assert _relerr(bg.grad, br.grad) < 1e-5


@pytest.mark.parametrize("B,N,dim", [(2, 8, 32), (8, 216, 128), (3, 27, 20)])
def test_token_pool(B, N, dim):
    ops = _ops()
    m, p = _rand(B, N, dim, seed=51), _rand(B, N, dim, seed=52)
    go = _rand(B, 4 * dim, seed=53)
    mr, pr = m.double().requires_grad_(True), p.double().requires_grad_(True)
    ref = torch.cat([mr.mean(1), pr.mean(1), mr.max(1).values, pr.max(1).values], dim=1)
    ref.backward(go.double())
    mg, pg = m.to(DEV).requires_grad_(True), p.to(DEV).requires_grad_(True)
    out = ops.token_pool(mg, pg)
    out.backward(go.to(DEV))
    assert _relerr(out.detach(), ref.detach()) < 1e-6
    assert _relerr(mg.grad, mr.grad) < 1e-6 and _relerr(pg.grad, pr.grad) < 1e-6


def test_argument_errors_are_reported_not_launched():
    from transmf_ad_amd import _lib
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_conv3d_fwd", None, None, None, None, 1, 4, 4, 4, 8, 8, 3, None)
    x = torch.zeros(16, device=DEV)
    with pytest.raises(_lib.TmfError, match="ksize"):
        _lib.call("tmf_conv3d_fwd", x.data_ptr(), x.data_ptr(), x.data_ptr(), None, 1, 1, 1, 1, 8, 8, 2, None)
    with pytest.raises(_lib.TmfError, match="workspace"):
        _lib.call("tmf_conv3d_wgrad", x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0,
                  1, 4, 4, 4, 8, 8, 3, 0, None)
    with pytest.raises(_lib.TmfError, match="dw_layout"):
        _lib.call("tmf_conv3d_wgrad", x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 1 << 20,
                  1, 4, 4, 4, 8, 8, 3, 7, None)
    with pytest.raises(_lib.TmfError, match="dim_head"):
        _lib.call("tmf_xattn_fwd", x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(),
                  1, 1, 4, 4, 12, 12, 24, 1.0, None)


def test_full_size_conv_properties():
    """BASELINE-size layer (conv2.3: 8 x 48^3, 32 -> 64 channels) through size-independent properties, no oracle:
    (i) exact homogeneity — scaling the input by a power of two scales every output bit-exactly;
    (ii) adjointness — <dz, conv(x, w)> == <wgrad(x, dz), w> == <dgrad(dz, w), x> (the three kernels are mutually
    consistent transposes of one bilinear map)."""
    ops = _ops()
    B, S, cin, cout = 8, 48, 32, 64
    g = torch.Generator(device=DEV).manual_seed(7)
    x = torch.randn((B, S, S, S, cin), device=DEV, generator=g)
    dz = torch.randn((B, S, S, S, cout), device=DEV, generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), device=DEV, generator=g) * (27 * cin) ** -0.5
    wp, wd = ops.pack_weight(w), ops.pack_weight_dgrad(w)
    z, part, _ = ops.conv3d_raw(x, wp, cin, cout, 3, True)
    z4, _, _ = ops.conv3d_raw(x * 4.0, wp, cin, cout, 3, False)
    assert torch.equal(z4, z * 4.0)
    assert torch.allclose(part[:, 0].double().sum(0), z.double().sum(dim=(0, 1, 2, 3)), rtol=1e-6, atol=1e-2)
    dw = ops.unpack_wgrad(ops.conv3d_wgrad(x, dz, cin, cout, 3), cout, cin, 3)
    dx, _, _ = ops.conv3d_raw(dz, wd, cout, cin, 3, False)
    a = (dz.double() * z.double()).sum().item()
    b = (dw.double() * w.double()).sum().item()
    c = (dx.double() * x.double()).sum().item()
    scale = (dz.double().abs() * z.double().abs()).sum().item()
    assert abs(a - b) <= 1e-6 * scale and abs(a - c) <= 1e-6 * scale, (a, b, c, scale)


def test_full_size_bf16_conv_properties():
    """configs[2]-size layer (conv2.3 at 128^3 input: 8 x 64^3, 32 -> 64 channels, bf16 tensors) through size-independent
    properties, no oracle: (i) the two forms of the large-brick forward kernel (register-staged, LDS-DMA) accumulate in
    the same order: bit-identical outputs and statistics; (ii) exact homogeneity under a power-of-two scale; (iii) the
    two weight-gradient kernels (register transpose, LDS transposing reads) agree to fp32 summation order; (iv)
    adjointness <dz, conv(x, w)> == <wgrad(x, dz), w> == <dgrad(dz, w), x> with bf16-exact operands."""
    ops = _ops()
    from transmf_ad_amd import _lib
    B, S, cin, cout = 8, 64, 32, 64
    g = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn((B, S, S, S, cin), device=DEV, generator=g).bfloat16()
    dz = torch.randn((B, S, S, S, cout), device=DEV, generator=g).bfloat16()
    w = (torch.randn((cout, cin, 3, 3, 3), device=DEV, generator=g) * (27 * cin) ** -0.5).bfloat16().float()
    wf, wd = ops.pack_weight_bf16(w), ops.pack_weight_dgrad_bf16(w)
    try:
        _lib.call("tmf_set_option", b"bf16_dma", 0)
        z0, p0, _ = ops.conv3d_bf16_raw(x, wf, cin, cout, True, out_bf16=False)
        _lib.call("tmf_set_option", b"bf16_dma", 1)
        z, part, _ = ops.conv3d_bf16_raw(x, wf, cin, cout, True, out_bf16=False)
        assert torch.equal(z, z0) and torch.equal(part, p0)
        z4, _, _ = ops.conv3d_bf16_raw(x * 4.0, wf, cin, cout, False, out_bf16=False)
        assert torch.equal(z4, z * 4.0)
        _lib.call("tmf_set_option", b"wgrad_tr", 0)
        dw0 = ops.conv3d_wgrad_bf16(x, dz, cin, cout)
        _lib.call("tmf_set_option", b"wgrad_tr", 1)
        dwt = ops.conv3d_wgrad_bf16(x, dz, cin, cout)
    finally:
        _lib.call("tmf_set_option", b"bf16_dma", 1)
        _lib.call("tmf_set_option", b"wgrad_tr", 1)
    assert _relerr(dwt, dw0.cpu()) < 2e-6
    dw = ops.unpack_wgrad(dwt, cout, cin, 3)
    dx, _, _ = ops.conv3d_bf16_raw(dz, wd, cout, cin, False, out_bf16=False)
    a = (dz.double() * z.double()).sum().item()
    b = (dw.double() * w.double()).sum().item()
    c = (dx.double() * x.double()).sum().item()
    scale = (dz.double().abs() * z.double().abs()).sum().item()
    assert abs(a - b) <= 1e-6 * scale and abs(a - c) <= 1e-6 * scale, (a, b, c, scale)


BF16_SHAPES = [
    # B, D, H, W, cin, cout
    (2, 8, 8, 8, 8, 16),
    (1, 5, 7, 9, 16, 32),          # ragged bricks
    (2, 16, 16, 16, 32, 64),
    (1, 12, 12, 12, 128, 256),     # 4 channel chunks, 4 output blocks
    (1, 9, 8, 11, 40, 72),         # partial last chunk, partial output tile
    (2, 24, 24, 24, 64, 32),
]


@pytest.mark.parametrize("shape", BF16_SHAPES + [(1, 17, 16, 24, 32, 32), (2, 16, 16, 16, 16, 24)])
def test_conv3d_bf16_mfma(shape, bf16_kernel_choice):
    """bf16 matrix-core convolution: with inputs and weights that ARE bf16 numbers the products are exact in fp32, so
    the kernel must match an fp64 reference to fp32-accumulation accuracy (2e-6); with general fp32 inputs the
    error is the bf16 rounding of the operands (<= 2^-8 each) — bounded at 1e-2 of max, typically 2e-3."""
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=61)
    w = _rand(cout, cin, 3, 3, 3, seed=62, scale=(cin * 27) ** -0.5)
    xb, wb = x.bfloat16().float(), w.bfloat16().float()
    ref = F.conv3d(xb.double(), wb.double(), padding=1)
    z, part, nblk = ops.conv3d_bf16_raw(_ndhwc(xb).to(DEV), ops.pack_weight_bf16(wb.to(DEV)), cin, cout, True)
    torch.cuda.synchronize()
    assert _relerr(_ncdhw(z.cpu()), ref) < 2e-6
    s = part.double().sum(0).cpu()
    r = ref.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    assert (s[0] - r.sum(1)).abs().max() <= 1e-4 * max(1.0, r.abs().sum(1).max().item())
    assert (s[1] - (r * r).sum(1)).abs().max() <= 1e-5 * (r * r).sum(1).max().item()
    # general fp32 operands: rounding happens inside the kernel (activations) / in pack_weight_bf16 (weights)
    z2, _, _ = ops.conv3d_bf16_raw(_ndhwc(x).to(DEV), ops.pack_weight_bf16(w.to(DEV)), cin, cout, False)
    assert torch.equal(z2, z)                      # in-kernel RNE == torch's .bfloat16()
    assert _relerr(_ncdhw(z2.cpu()), F.conv3d(x.double(), w.double(), padding=1)) < 1e-2
    # data gradient through the same kernel
    if cout % 8 == 0:
        dz = _rand(B, cout, D, H, W, seed=63).bfloat16().float()
        xr = xb.double().requires_grad_(True)
        F.conv3d(xr, wb.double(), padding=1).backward(dz.double())
        dx, _, _ = ops.conv3d_bf16_raw(_ndhwc(dz).to(DEV), ops.pack_weight_dgrad_bf16(wb.to(DEV)), cout, cin, False)
        assert _relerr(_ncdhw(dx.cpu()), xr.grad) < 2e-6


@pytest.mark.parametrize("shape", [(2, 16, 16, 16, 32, 64), (1, 11, 13, 9, 64, 32), (1, 9, 8, 11, 40, 72), (1, 17, 16, 24, 32, 32),
                                   (2, 8, 24, 8, 16, 24), (1, 16, 8, 8, 64, 130)])
def test_conv3d_bf16_tensor_modes_agree_bitwise(shape, bf16_kernel_choice):
    """The four tensor-type modes of tmf_conv3d_fwd_bf16_t (io bit 0: bf16 input tensor, bit 1: bf16 output tensor) run the
    same products in the same order: with an input that IS bf16-valued the fp32 outputs agree bit for bit, a bf16 output is
    the round-to-nearest-even of the fp32 one (also where bricks overhang the volume and the channel tile is partial: the
    lean buffer-store epilogue of the 8x8x8-brick kernel), and the BatchNorm statistic partials are identical."""
    ops = _ops()
    from transmf_ad_amd import _lib
    B, D, H, W, cin, cout = shape
    x = _ndhwc(_rand(B, cin, D, H, W, seed=71).bfloat16().float()).to(DEV)
    w = ops.pack_weight_bf16((_rand(cout, cin, 3, 3, 3, seed=72, scale=(cin * 27) ** -0.5)).to(DEV))
    nblk = _lib.query("tmf_conv3d_bf16_stat_blocks", B, D, H, W)
    outs = []
    for io in range(4):
        xin = x.bfloat16() if io & 1 else x
        z = torch.full((B, D, H, W, cout), float("nan"), device=DEV, dtype=torch.bfloat16 if io & 2 else torch.float32)
        part = torch.zeros((nblk, 2, cout), device=DEV)
        _lib.call("tmf_conv3d_fwd_bf16_t", xin.data_ptr(), w.data_ptr(), z.data_ptr(), part.data_ptr(),
                  B, D, H, W, cin, cout, io, torch.cuda.current_stream().cuda_stream)
        outs.append((z, part))
    torch.cuda.synchronize()
    z0, p0 = outs[0]
    assert torch.isfinite(z0).all()
    for io in range(1, 4):
        z, part = outs[io]
        if io & 2:
            assert torch.equal(z, z0.bfloat16()), io
        else:
            assert torch.equal(z, z0), io
        assert torch.equal(part, p0), io


@pytest.fixture(params=[2, 0], ids=["tr-read", "reg-transpose"])
def wgrad_kernel_choice(request):
    """Both bf16 weight-gradient kernels: the transposing-read one (cin, cout multiples of 8) and the register-transposing one."""
    from transmf_ad_amd import _lib
    _lib.call("tmf_set_option", b"wgrad_tr", request.param)
    yield request.param
    _lib.call("tmf_set_option", b"wgrad_tr", 1)


@pytest.mark.parametrize("shape", BF16_SHAPES + [(1, 20, 9, 17, 32, 64), (2, 8, 16, 8, 72, 136)])
def test_conv3d_wgrad_bf16_mfma(shape, wgrad_kernel_choice):
    """bf16 matrix-core weight gradient: operands that ARE bf16 numbers give exact products, so the result is held
    to fp32-accumulation accuracy against fp64 (fp32 tensors and bf16 tensors); general fp32 operands are rounded in the
    kernel exactly as torch's .bfloat16() does (bit-identical result), and stay within bf16-operand accuracy of the
    fp32 gradient."""
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=81)
    dz = _rand(B, cout, D, H, W, seed=82)
    xb, dzb = x.bfloat16().float(), dz.bfloat16().float()
    wr = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(xb.double(), wr, padding=1).backward(dzb.double())
    dw = ops.conv3d_wgrad_bf16(_ndhwc(xb).to(DEV), _ndhwc(dzb).to(DEV), cin, cout)
    torch.cuda.synchronize()
    got = ops.unpack_wgrad(dw, cout, cin, 3).cpu()
    assert _relerr(got, wr.grad) < 5e-6
    dw2 = ops.conv3d_wgrad_bf16(_ndhwc(x).to(DEV), _ndhwc(dz).to(DEV), cin, cout)
    assert torch.equal(dw2, dw)
    if cin % 2 == 0 and cout % 2 == 0:
        dw3 = ops.conv3d_wgrad_bf16(_ndhwc(x).to(DEV).bfloat16(), _ndhwc(dz).to(DEV).bfloat16(), cin, cout)
        assert _relerr(ops.unpack_wgrad(dw3, cout, cin, 3).cpu(), wr.grad) < 5e-6
        dw4 = ops.conv3d_wgrad_bf16(_ndhwc(x).to(DEV).bfloat16(), _ndhwc(dz).to(DEV).bfloat16(), cin, cout, reference_layout=True)
        assert _relerr(dw4.cpu(), wr.grad) < 5e-6
    wr2 = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(x.double(), wr2, padding=1).backward(dz.double())
    assert _relerr(got, wr2.grad) < 1e-2


def test_block_in_bf16_mode(bf16_kernel_choice):
    """A full sNet block with the bf16 conv precision: forward and gradients within bf16-operand accuracy of fp64."""
    ops = _ops()
    B, D, H, W, cin, cout, k, pool = 2, 16, 16, 16, 32, 64, 3, "max"
    x = _rand(B, cin, D, H, W, seed=11)
    w = _rand(cout, cin, k, k, k, seed=12, scale=(cin * k ** 3) ** -0.5)
    b, g, be = _rand(cout, seed=13, scale=0.1), 1 + _rand(cout, seed=14, scale=0.1), _rand(cout, seed=15, scale=0.1)
    rm, rv = _rand(cout, seed=16, scale=0.1), 1 + _rand(cout, seed=17, scale=0.1).abs()
    xr, P, _rm, _rv, yr = _block_ref(x, w, b, g, be, rm, rv, True, pool, torch.float64)
    go = _rand(*yr.shape, seed=18)
    yr.backward(go.double())
    ops.set_conv_precision("bf16")
    try:
        xg = _ndhwc(x).to(DEV).requires_grad_(True)
        Pg = [t.clone().to(DEV).requires_grad_(True) for t in (w, b, g, be)]
        yg = ops.conv_bn_act_pool(xg, Pg[0], Pg[1], Pg[2], Pg[3], rm.clone().to(DEV), rv.clone().to(DEV), True, pool=pool)
        yg.backward(_ndhwc(go).to(DEV))
        torch.cuda.synchronize()
    finally:
        ops.set_conv_precision("fp32")
    assert _relerr(_ncdhw(yg.detach().cpu()), yr.detach()) < 2e-2

    def l2(got, ref):       # bf16 noise (1e-3 of z) flips many max-pool / LeakyReLU decisions: compare in L2
        return ((got.double().cpu() - ref).norm() / ref.norm()).item()
    assert l2(Pg[0].grad, P[0].grad) < 1e-1 and l2(_ncdhw(xg.grad.cpu()), xr.grad) < 1e-1, (l2(Pg[0].grad, P[0].grad), l2(_ncdhw(xg.grad.cpu()), xr.grad))
    assert l2(Pg[2].grad, P[2].grad) < 1e-1 and l2(Pg[3].grad, P[3].grad) < 1e-1


@pytest.mark.parametrize("shape", BF16_SHAPES)
def test_conv3d_fp32_accurate_split(shape):
    """3-way bf16 split on the bf16 matrix cores: held to the SAME tolerance as the exact-fp32 MFMA kernel (1e-5
    of max vs fp64, general fp32 operands), and its error is compared with that kernel's on the same data."""
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=71)
    w = _rand(cout, cin, 3, 3, 3, seed=72, scale=(cin * 27) ** -0.5)
    ref = F.conv3d(x.double(), w.double(), padding=1)
    xg, wg = _ndhwc(x).to(DEV), w.to(DEV)
    w3 = ops.split3_bf16(wg.permute(2, 3, 4, 0, 1).contiguous())
    assert torch.equal(w3.float().sum(0), wg.permute(2, 3, 4, 0, 1))          # the decomposition is exact
    # tmf_pack_conv_weights_split3 (one launch for both layouts) is bitwise torch's cast / subtract / cast / subtract / cast
    p3f, p3d = ops.pack_weights_split3(wg, True)
    assert torch.equal(p3f.reshape(w3.shape), w3)
    assert torch.equal(p3d.reshape(3, 3, 3, 3, cin, cout), ops.split3_bf16(wg.flip(2, 3, 4).permute(2, 3, 4, 1, 0).contiguous()))
    z, part, _ = ops.conv3d_split_raw(xg, w3, cin, cout, True)
    z32, _, _ = ops.conv3d_raw(xg, ops.pack_weight(wg), cin, cout, 3, False)
    torch.cuda.synchronize()
    e_split, e_f32 = _relerr(_ncdhw(z.cpu()), ref), _relerr(_ncdhw(z32.cpu()), ref)
    assert e_split < 1e-5, (e_split, e_f32)
    assert e_split < 4 * e_f32 + 1e-6, (e_split, e_f32)
    s = part.double().sum(0).cpu()
    r = ref.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    assert (s[1] - (r * r).sum(1)).abs().max() <= 1e-5 * (r * r).sum(1).max().item()
    if cout % 8 == 0:
        dz = _rand(B, cout, D, H, W, seed=73)
        xr = x.double().requires_grad_(True)
        F.conv3d(xr, w.double(), padding=1).backward(dz.double())
        wd3 = ops.split3_bf16(wg.flip(2, 3, 4).permute(2, 3, 4, 1, 0).contiguous())
        dx, _, _ = ops.conv3d_split_raw(_ndhwc(dz).to(DEV), wd3, cout, cin, False)
        assert _relerr(_ncdhw(dx.cpu()), xr.grad) < 1e-5


def test_split_exact_on_integers():
    ops = _ops()
    cin, cout = 32, 64
    x = torch.zeros(1, cin, 8, 8, 8)
    x[0, :, 3, 4, 5] = torch.arange(cin, dtype=torch.float32) * 257 + 1        # needs > 8 significand bits
    w = torch.zeros(cout, cin, 3, 3, 3)
    for co in range(cout):
        for ci in range(cin):
            w[co, ci, 1, 1, 1] = (co * 37 + ci * 11) % 23 - 7.0
    w[:, :, 0, 1, 2] = 0.5
    ref = F.conv3d(x, w, padding=1)
    w3 = ops.split3_bf16(w.to(DEV).permute(2, 3, 4, 0, 1).contiguous())
    z, _, _ = ops.conv3d_split_raw(_ndhwc(x).to(DEV), w3, cin, cout, False)
    assert torch.equal(_ncdhw(z.cpu()), ref)


# ---------------------------------------------------------------------------------------------------
# fused transformer-block linears (csrc/token_gemm.hip)
# ---------------------------------------------------------------------------------------------------

def _gelu64(h):
    return 0.5 * h * (1 + torch.erf(h / 2 ** 0.5))


@pytest.mark.parametrize("R", [1728, 50])
def test_tok_linear_fwd_variants(R):
    ops = _ops()
    x = _rand(R, 128, seed=91)
    w = _rand(256, 128, seed=92, scale=128 ** -0.5)
    b = _rand(256, seed=93, scale=0.1)
    res = _rand(R, 256, seed=94)
    g, be = 1 + _rand(128, seed=95, scale=0.1), _rand(128, seed=96, scale=0.1)
    xd, wd = x.double(), w.double()
    y, _, _ = ops.tok_linear_fwd(x.to(DEV), w.to(DEV))
    assert _relerr(y.cpu(), xd @ wd.t()) < 2e-6
    y, _, _ = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), bias=b.to(DEV), residual=res.to(DEV))
    assert _relerr(y.cpu(), xd @ wd.t() + b.double() + res.double()) < 2e-6
    ln = F.layer_norm(xd, (128,), g.double(), be.double(), 1e-5)
    y, (mean, rstd, a), _ = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), ln=(g.to(DEV), be.to(DEV), 1e-5), keep_ln_out=True)
    assert _relerr(a.cpu(), ln) < 2e-6 and _relerr(y.cpu(), ln @ wd.t()) < 2e-6
    assert _relerr(mean.cpu(), xd.mean(1)) < 2e-6
    assert _relerr(rstd.cpu(), (xd.var(1, unbiased=False) + 1e-5).rsqrt()) < 2e-6
    y, _, pre = ops.tok_linear_fwd(x.to(DEV), w.to(DEV), bias=b.to(DEV), ln=(g.to(DEV), be.to(DEV), 1e-5), gelu=True)
    h = ln @ wd.t() + b.double()
    assert _relerr(pre.cpu(), h) < 2e-6 and _relerr(y.cpu(), _gelu64(h)) < 2e-6
    # K = 512 -> 128 (second FeedForward linear)
    x5, w5 = _rand(R, 512, seed=97), _rand(128, 512, seed=98, scale=512 ** -0.5)
    y, _, _ = ops.tok_linear_fwd(x5.to(DEV), w5.to(DEV), bias=b[:128].to(DEV), residual=res[:, :128].contiguous().to(DEV))
    assert _relerr(y.cpu(), x5.double() @ w5.double().t() + b[:128].double() + res[:, :128].double()) < 2e-6


@pytest.mark.parametrize("R", [1728, 50])
def test_tok_linear_bwd_input_variants(R):
    ops = _ops()
    from transmf_ad_amd import _lib as lib
    nblk = lib.query("tmf_tok_row_blocks", R)
    # plain + bias column sums:  dy [R][256] . w [256][128]
    dy = _rand(R, 256, seed=101)
    w = _rand(256, 128, seed=102, scale=0.1)
    add1, add2 = _rand(R, 128, seed=103), _rand(R, 128, seed=104)
    stride = 256 + 256
    part = torch.zeros((nblk, stride), device=DEV)
    dx = ops.tok_linear_bwd_input(dy.to(DEV), w.to(DEV), add1=add1.to(DEV), bias_partial=(part, 256), partial_stride=stride)
    assert _relerr(dx.cpu(), dy.double() @ w.double() + add1.double()) < 2e-6
    assert _relerr(part.sum(0)[256:].cpu(), dy.double().sum(0)) < 1e-5
    # GELU' epilogue:  dy [R][128] . w [128][512] * gelu'(h)
    dy2, w2, h = _rand(R, 128, seed=105), _rand(128, 512, seed=106, scale=0.1), _rand(R, 512, seed=107)
    hd = h.double().requires_grad_(True)
    _gelu64(hd).backward(dy2.double() @ w2.double())
    dx = ops.tok_linear_bwd_input(dy2.to(DEV), w2.to(DEV), gelu_pre=h.to(DEV))
    assert _relerr(dx.cpu(), hd.grad) < 2e-6
    # LayerNorm-backward epilogue + two residual gradients + parameter partials
    x = _rand(R, 128, seed=108)
    g = 1 + _rand(128, seed=109, scale=0.1)
    xd = x.double().requires_grad_(True)
    gd = g.double().requires_grad_(True)
    bd = torch.zeros(128, dtype=torch.float64, requires_grad=True)
    F.layer_norm(xd, (128,), gd, bd, 1e-5).backward(dy.double() @ w.double())
    mean = x.double().mean(1)
    rstd = (x.double().var(1, unbiased=False) + 1e-5).rsqrt()
    part = torch.zeros((nblk, stride), device=DEV)
    dx = ops.tok_linear_bwd_input(dy.to(DEV), w.to(DEV), ln=(x.to(DEV), mean.float().to(DEV), rstd.float().to(DEV), g.to(DEV)),
                                  add1=add1.to(DEV), add2=add2.to(DEV), ln_partial=(part, 0), partial_stride=stride)
    assert _relerr(dx.cpu(), xd.grad + add1.double() + add2.double()) < 5e-6
    sums = part.sum(0).cpu()
    assert _relerr(sums[:128], gd.grad) < 1e-5 and _relerr(sums[128:256], bd.grad) < 1e-5


@pytest.mark.parametrize("R", [1728, 50, 7])
def test_tok_wgrad_multi(R):
    ops = _ops()
    shapes = [(128, 512), (512, 128), (128, 128), (256, 128), (32, 64)]
    pairs = [(_rand(R + 3 * i, n, seed=150 + i), _rand(R + 3 * i, k, seed=160 + i)) for i, (n, k) in enumerate(shapes)]
    outs = ops.tok_wgrad_multi([(a.to(DEV), b.to(DEV)) for a, b in pairs])
    torch.cuda.synchronize()
    for (dy, x), got in zip(pairs, outs):
        assert _relerr(got.cpu(), dy.double().t() @ x.double()) < 5e-6


@pytest.mark.parametrize("with_context,depth", [(True, 1), (True, 2), (False, 1), (False, 2)])
def test_transformer_block_fused_and_unfused_match_fp64_formula(with_context, depth):
    """Transformer.forward on the fused-launch path (6 + 13 launches per layer) and on the op-per-launch path, each
    against an fp64 evaluation of the reference formula: output and the gradients of x, the context and every parameter.
    Without a context (self-attention) keys / values come from the LayerNorm output of the CURRENT layer — the case
    the fused path must not take with the raw tokens."""
    ops = _ops()
    from transmf_ad_amd import networks
    torch.manual_seed(5)
    tr = networks.Transformer(128, depth, 4, 32, 512, 0.).to(DEV)
    with torch.no_grad():
        for p in tr.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    x0 = _rand(3, 50, 128, seed=111)
    c0 = _rand(3, 70, 128, seed=112) if with_context else None
    go = _rand(3, 50, 128, seed=113)
    # fp64 reference with autograd on CPU copies of the parameters
    import copy
    tr64 = copy.deepcopy(tr).cpu().double()
    x64 = x0.double().requires_grad_(True)
    c64 = c0.double().requires_grad_(True) if with_context else None
    y64 = _transformer64_live(tr64, x64, c64, x64)
    y64.backward(go.double())
    ref = [y64.detach(), x64.grad] + ([c64.grad] if with_context else []) + [p.grad for p in tr64.parameters()]
    for fused in (True, False):
        ops.FUSE_TOKEN_LINEARS = fused
        try:
            tr.zero_grad()
            x = x0.to(DEV).requires_grad_(True)
            c = c0.to(DEV).requires_grad_(True) if with_context else None
            y = tr(x, context=c, residual=x)
            y.backward(go.to(DEV))
            torch.cuda.synchronize()
            got = [y.detach().cpu(), x.grad.cpu()] + ([c.grad.cpu()] if with_context else []) + \
                  [p.grad.cpu() for p in tr.parameters()]
        finally:
            ops.FUSE_TOKEN_LINEARS = True
        assert len(got) == len(ref)
        for i, (a, r) in enumerate(zip(got, ref)):
            assert _relerr(a, r) < 2e-5, (fused, i, _relerr(a, r))


def _transformer64_live(tr, x, ctx, residual):
    """fp64 evaluation of the reference formulas on an fp64 CPU copy of the module (gradients flow to its parameters):
    Transformer.forward (networks.py:226-230), PreNorm (:114-121: only x is normalised, a given context passes through
    raw; without one Attention's default(context, x) sees the NORMALISED x), Attention (:157-175), FeedForward
    (:125-137)."""
    for attn_pre, ff_pre in tr.layers:
        at, ff = attn_pre.fn, ff_pre.fn
        xn = F.layer_norm(x, (x.shape[-1],), attn_pre.norm.weight, attn_pre.norm.bias, attn_pre.norm.eps)
        c = xn if ctx is None else ctx
        q = xn @ at.to_q.weight.t()
        k, v = (c @ at.to_kv.weight.t()).chunk(2, dim=-1)
        B, N, inner = q.shape
        h = at.heads
        sp = lambda t: t.reshape(B, t.shape[1], h, inner // h).transpose(1, 2)
        dots = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * at.scale
        out = torch.einsum("bhij,bhjd->bhid", dots.softmax(dim=-1), sp(v)).transpose(1, 2).reshape(B, N, inner)
        x = out @ at.to_out[0].weight.t() + at.to_out[0].bias + x
        xn = F.layer_norm(x, (x.shape[-1],), ff_pre.norm.weight, ff_pre.norm.bias, ff_pre.norm.eps)
        hdn = _gelu64(xn @ ff.net[0].weight.t() + ff.net[0].bias)
        x = hdn @ ff.net[3].weight.t() + ff.net[3].bias + x
    y = F.layer_norm(x, (x.shape[-1],), tr.norm.weight, tr.norm.bias, tr.norm.eps)
    return y if residual is None else y + residual


class _FixedMask(torch.nn.Module):
    """Stands in for an nn.Dropout with a FIXED scaled keep-mask (what make_golden.py captures from the reference with
    forward hooks): the HIP path asks it through ``tmf_keep_mask``, the fp64 formula multiplies by ``m``."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return x * self.m.to(x.device, x.dtype).reshape(x.shape) if self.training else x

    def tmf_keep_mask(self, training):
        return self.m if training else None


def _fusion64(fz, mri, pet):
    """CrossTransformer_MOD_AVG.forward (networks.py:272-281) in fp64 on an fp64 CPU copy of the module, Dropout sites
    (networks.py:131,133,153) included through the modules that sit there."""
    def inst(tr, x, ctx):
        attn_pre, ff_pre = tr.layers[0]
        at, ff = attn_pre.fn, ff_pre.fn
        xn = F.layer_norm(x, (x.shape[-1],), attn_pre.norm.weight, attn_pre.norm.bias, attn_pre.norm.eps)
        q = xn @ at.to_q.weight.t()
        k, v = (ctx @ at.to_kv.weight.t()).chunk(2, dim=-1)
        B, N, inner = q.shape
        h = at.heads
        sp = lambda t: t.reshape(B, t.shape[1], h, inner // h).transpose(1, 2)
        dots = torch.einsum("bhid,bhjd->bhij", sp(q), sp(k)) * at.scale
        out = torch.einsum("bhij,bhjd->bhid", dots.softmax(dim=-1), sp(v)).transpose(1, 2).reshape(B, N, inner)
        x1 = at.to_out[1](out @ at.to_out[0].weight.t() + at.to_out[0].bias) + x
        xn = F.layer_norm(x1, (x.shape[-1],), ff_pre.norm.weight, ff_pre.norm.bias, ff_pre.norm.eps)
        hdn = ff.net[2](_gelu64(xn @ ff.net[0].weight.t() + ff.net[0].bias))
        x2 = ff.net[4](hdn @ ff.net[3].weight.t() + ff.net[3].bias) + x1
        return F.layer_norm(x2, (x.shape[-1],), tr.norm.weight, tr.norm.bias, tr.norm.eps)
    for mri_enc, pet_enc in fz.layers:
        mri = inst(mri_enc, mri, pet) + mri
        pet = inst(pet_enc, pet, mri) + pet
    return torch.cat([mri.mean(dim=1), pet.mean(dim=1), mri.max(dim=1).values, pet.max(dim=1).values], dim=1)


@pytest.mark.parametrize("heads", [4, 8], ids=["4x32", "8x16"])
@pytest.mark.parametrize("B,N,depth,drop", [(2, 27, 2, False), (3, 216, 3, False), (2, 150, 1, True), (1, 512, 1, False),
                                            (2, 16, 1, False), (8, 216, 3, True), (2, 5, 2, True)])
def test_fused_fusion_kernels_match_fp64_formula(B, N, depth, drop, heads):
    """The whole fusion block on the fused per-instance kernels (csrc/xformer_fused.hip: 1 forward + 2 backward launches
    per Transformer instance, all weight gradients in one launch) against an fp64 evaluation of the reference formula
    (networks.py:114-175, 215-230, 272-281): cls, the gradients of both token tensors and of every parameter; ragged
    token counts (partial 16-row tiles), one to 32 key tiles, and — `drop` — fixed Dropout keep-masks at the three
    Dropout sites of every instance.  Also against the one-launch-per-Linear path of the same entry point (1e-5).  Both head
    geometries of the reference's scripts: 4 heads of 32 (kfold_train_adversarial.py:78-79) and — round 6, the H2 instances of the
    fused kernels — 8 heads of 16 (train_adversarial.py:30-31)."""
    import copy
    ops = _ops()
    from transmf_ad_amd import networks
    torch.manual_seed(7)
    fz = networks.CrossTransformer_MOD_AVG(128, depth, heads, 128 // heads, 512, 0.).to(DEV).train()
    assert ops.fusion_fused_supported(N, 128, heads, 128 // heads, 512)
    with torch.no_grad():
        for p in fz.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    if drop:
        rs = np.random.RandomState(3)
        keep = lambda n: torch.from_numpy((rs.rand(B * N, n) >= 0.3).astype(np.float32) / 0.7)
        for pair in fz.layers:
            for tr in pair:
                at, ff = tr.layers[0][0].fn, tr.layers[0][1].fn
                at.to_out[1] = _FixedMask(keep(128))
                ff.net[2] = _FixedMask(keep(512))
                ff.net[4] = _FixedMask(keep(128))
                tr._drops = None
    m0, p0 = _rand(B, N, 128, seed=201), _rand(B, N, 128, seed=202)
    go = _rand(B, 512, seed=203)
    fz64 = copy.deepcopy(fz).cpu().double().train()
    m64, p64 = m0.double().requires_grad_(True), p0.double().requires_grad_(True)
    c64 = _fusion64(fz64, m64, p64)
    c64.backward(go.double())
    ref = [c64.detach(), m64.grad, p64.grad] + [p.grad for p in fz64.parameters()]
    names = ["cls", "d mri", "d pet"] + [k for k, _ in fz64.named_parameters()]
    res = {}
    for fused in ((True, False) if not drop else (True,)):
        ops.FUSION_FUSED_KERNELS = fused
        try:
            fz.zero_grad()
            m, p = m0.to(DEV).requires_grad_(True), p0.to(DEV).requires_grad_(True)
            c = fz(m, p)
            assert type(c.grad_fn).__name__.startswith("FusionTrain"), c.grad_fn
            c.backward(go.to(DEV))
            torch.cuda.synchronize()
            res[fused] = [c.detach().cpu(), m.grad.cpu(), p.grad.cpu()] + [q.grad.cpu() for q in fz.parameters()]
        finally:
            ops.FUSION_FUSED_KERNELS = True
        assert len(res[fused]) == len(ref)
        for name, a, r in zip(names, res[fused], ref):
            assert torch.isfinite(a).all(), (fused, name)
            assert _relerr(a, r) < 3e-5, (fused, name, _relerr(a, r))
    if not drop:
        for name, a, b in zip(names, res[True], res[False]):
            assert _relerr(a, b) < 1e-5, (name, _relerr(a, b))


@pytest.mark.parametrize("heads", [4, 8], ids=["4x32", "8x16"])
def test_fused_fusion_kernels_are_deterministic_and_leave_no_trace(heads):
    """Two passes over the same inputs are bitwise equal (no atomics, fixed summation orders), also when the saved /
    scratch workspaces start out filled with NaN (nothing uninitialised is read: padded token rows, transposed-copy
    padding)."""
    ops = _ops()
    from transmf_ad_amd import networks
    torch.manual_seed(9)
    fz = networks.CrossTransformer_MOD_AVG(128, 2, heads, 128 // heads, 512, 0.).to(DEV).train()
    m0, p0 = _rand(3, 27, 128, seed=211).to(DEV), _rand(3, 27, 128, seed=212).to(DEV)
    go = _rand(3, 512, seed=213).to(DEV)
    outs = []
    for rep in range(2):
        if rep == 1:            # poison the allocator's free blocks the next pass will be handed
            junk = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 22, 1 << 20, 1 << 18, 1 << 16)]
            del junk
        fz.zero_grad()
        m, p = m0.clone().requires_grad_(True), p0.clone().requires_grad_(True)
        c = fz(m, p)
        c.backward(go)
        torch.cuda.synchronize()
        outs.append([c.detach().clone(), m.grad.clone(), p.grad.clone()] + [q.grad.clone() for q in fz.parameters()])
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


def test_layout_conversion_round_trip():
    from transmf_ad_amd import _lib as lib
    x = _rand(2, 5, 7, 9, 11, seed=121).to(DEV)                  # NCDHW, ragged against the 32 x 32 tiles
    y = torch.empty((2, 7, 9, 11, 5), device=DEV)
    lib.call("tmf_layout_ncdhw_to_ndhwc", x.data_ptr(), y.data_ptr(), 2, 5, 7 * 9 * 11, 0)
    assert torch.equal(y, x.permute(0, 2, 3, 4, 1).contiguous())
    z = torch.empty_like(x)
    lib.call("tmf_layout_ndhwc_to_ncdhw", y.data_ptr(), z.data_ptr(), 2, 5, 7 * 9 * 11, 0)
    assert torch.equal(z, x)


# ---------------------------------------------------------------------------------------------------------
# memory-safety properties of the buffer-addressed kernels: results must not depend on what lies around the
# inputs (reads stay in bounds / masked lanes read nothing), and nothing outside the outputs may be written
# ---------------------------------------------------------------------------------------------------------
def _guarded(t, fill, pad=4096):
    big = torch.full((t.numel() + 2 * pad,), fill, device=t.device, dtype=t.dtype)
    v = big[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v, big


@pytest.mark.parametrize("shape", [(2, 24, 24, 24, 32, 64), (1, 11, 13, 9, 64, 64), (2, 12, 12, 12, 128, 256)])
def test_conv_kernels_ignore_memory_around_their_inputs(shape):
    ops = _ops()
    B, D, H, W, cin, cout = shape
    torch.manual_seed(0)
    x0 = torch.randn((B, D, H, W, cin), device=DEV)
    dz0 = torch.randn((B, D, H, W, cout), device=DEV) * 0.1
    w = torch.randn((cout, cin, 3, 3, 3), device=DEV) * 0.05
    wp, wb = ops.pack_weight(w), ops.pack_weight_bf16(w)
    res = []
    for fill in (0.0, float("nan"), 3e30):
        xg, k1 = _guarded(x0, fill)
        dg, k2 = _guarded(dz0, fill)
        wg, k3 = _guarded(wp, fill)
        x16, k4 = _guarded(x0.bfloat16(), fill)
        d16, k5 = _guarded(dz0.bfloat16(), fill)
        z, part, _ = ops.conv3d_raw(xg, wg, cin, cout, 3, True)
        dw = ops.conv3d_wgrad(xg, dg, cin, cout, 3)
        zb, pb, _ = ops.conv3d_bf16_raw(x16, wb, cin, cout, True, out_bf16=True)
        dwb = ops.conv3d_wgrad_bf16(x16, d16, cin, cout)
        torch.cuda.synchronize()
        res.append([t.float().clone() for t in (z, part, dw, zb, pb, dwb)])
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert torch.isfinite(b).all()
            assert torch.equal(a, b)


@pytest.mark.parametrize("shape", [(2, 24, 24, 24, 64, 64, 3), (1, 11, 13, 9, 64, 32, 3), (1, 6, 6, 6, 256, 128, 0)])
def test_bf16_conv_writes_only_its_output(shape, bf16_kernel_choice):
    ops = _ops()
    from transmf_ad_amd import _lib
    B, D, H, W, cin, cout, io = shape
    x = torch.randn((B, D, H, W, cin), device=DEV)
    if io & 1:
        x = x.bfloat16()
    w = ops.pack_weight_bf16(torch.randn((cout, cin, 3, 3, 3), device=DEV) * 0.05)
    n, pad, sent = B * D * H * W * cout, 1 << 14, 12345.0
    big = torch.full((n + 2 * pad,), sent, device=DEV, dtype=torch.bfloat16 if io & 2 else torch.float32)
    nblk = _lib.query("tmf_conv3d_bf16_stat_blocks", B, D, H, W)
    pbig = torch.full((nblk * 2 * cout + 2 * pad,), sent, device=DEV)
    _lib.call("tmf_conv3d_fwd_bf16_t", x.data_ptr(), w.data_ptr(), big[pad:].data_ptr(), pbig[pad:].data_ptr(),
              B, D, H, W, cin, cout, io, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (big[:pad] == sent).all() and (big[pad + n:] == sent).all()
    assert (pbig[:pad] == sent).all() and (pbig[pad + nblk * 2 * cout:] == sent).all()
    assert int((big[pad:pad + n] == sent).sum()) == 0          # every output element was written


def test_first_block_ignores_memory_around_its_inputs():
    ops = _ops()
    import transmf_ad_amd as T
    for prec, out16 in (("fp32", False), ("bf16", True)):
        T.set_conv_precision(prec)
        T.set_activation_storage("bf16" if out16 else "fp32")
        try:
            torch.manual_seed(0)
            B, S, C = 2, 24, 32
            x = torch.rand((B, S, S, S, 1), device=DEV)
            P = [(torch.randn((C, 1, 3, 3, 3), device=DEV) * 0.2).requires_grad_(True), torch.zeros(C, device=DEV, requires_grad=True),
                 torch.ones(C, device=DEV, requires_grad=True), torch.zeros(C, device=DEV, requires_grad=True)]
            dout = torch.randn((B, S // 2, S // 2, S // 2, C), device=DEV) * 0.1
            if out16:
                dout = dout.bfloat16()
            res = []
            for fill in (0.0, float("nan"), 1e30):
                xg, k1 = _guarded(x, fill)
                dg, k2 = _guarded(dout, fill)
                for p in P:
                    p.grad = None
                y = ops.conv_bn_act_pool(xg, *P, torch.zeros(C, device=DEV), torch.ones(C, device=DEV), True, pool="max", out_bf16=out16)
                y.backward(dg)
                torch.cuda.synchronize()
                res.append([y.detach().float().clone()] + [p.grad.clone() for p in (P[0], P[2], P[3])])
            for other in res[1:]:
                for a, b in zip(res[0], other):
                    assert torch.isfinite(b).all() and torch.equal(a, b)
        finally:
            T.set_conv_precision("fp32")
            T.set_activation_storage("fp32")


def test_conv_kernels_are_deterministic_on_two_concurrent_streams():
    ops = _ops()
    torch.manual_seed(0)
    cin, cout, s = 32, 64, 24
    xa, xb = (torch.randn((4, s, s, s, cin), device=DEV) for _ in range(2))
    wa, wb = (ops.pack_weight(torch.randn((cout, cin, 3, 3, 3), device=DEV) * 0.05) for _ in range(2))
    za0, pa0, _ = ops.conv3d_raw(xa, wa, cin, cout, 3, True)
    zb0, pb0, _ = ops.conv3d_raw(xb, wb, cin, cout, 3, True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(5):
        with torch.cuda.stream(s1):
            za, pa, _n = ops.conv3d_raw(xa, wa, cin, cout, 3, True)
        with torch.cuda.stream(s2):
            zb, pb, _n = ops.conv3d_raw(xb, wb, cin, cout, 3, True)
        torch.cuda.synchronize()
        assert torch.equal(za, za0) and torch.equal(zb, zb0) and torch.equal(pa, pa0) and torch.equal(pb, pb0)


@pytest.mark.parametrize("shape", [(4, 24, 32, 64), (2, 13, 64, 64), (4, 12, 128, 256)])
def test_weight_gradients_write_only_output_and_workspace(shape):
    from transmf_ad_amd import _lib
    B, s, cin, cout = shape
    sent, pad = 777.0, 1 << 14
    st = torch.cuda.current_stream().cuda_stream
    x = torch.randn((B, s, s, s, cin), device=DEV)
    dz = torch.randn((B, s, s, s, cout), device=DEV) * 0.1
    for entry, query, xs, dzs, extra in (
            ("tmf_conv3d_wgrad", "tmf_conv3d_wgrad_workspace_bytes", x, dz, (3, 0)),
            ("tmf_conv3d_wgrad", "tmf_conv3d_wgrad_workspace_bytes", x, dz, (3, 1)),          # reference-layout stores
            ("tmf_conv3d_wgrad_bf16_t", "tmf_conv3d_wgrad_bf16_workspace_bytes", x.bfloat16(), dz.bfloat16(), (1, 1))):
        nbytes = _lib.query(query, B, s, s, s, cin, cout, *((3,) if entry == "tmf_conv3d_wgrad" else ()))
        nws, ndw = max(nbytes, 16) // 4, 27 * cin * cout
        wbig = torch.full((nws + 2 * pad,), sent, device=DEV)
        dbig = torch.full((ndw + 2 * pad,), sent, device=DEV)
        _lib.call(entry, xs.data_ptr(), dzs.data_ptr(), dbig[pad:].data_ptr(), wbig[pad:].data_ptr(), nbytes,
                  B, s, s, s, cin, cout, *extra, st)
        torch.cuda.synchronize()
        assert (wbig[:pad] == sent).all() and (wbig[pad + nws:] == sent).all(), entry
        assert (dbig[:pad] == sent).all() and (dbig[pad + ndw:] == sent).all(), entry
        assert int((dbig[pad:pad + ndw] == sent).sum()) == 0, entry


def test_dropout_keep_masks_one_launch():
    """tmf_dropout_keep_masks (ops.dropout_keep_masks): the scaled keep-masks of several nn.Dropout modules from ONE launch of a
    counter-based Philox generator — values are 0 or 1 / keep, the keep rate is right to 4 sigma, segments and calls differ,
    torch.manual_seed reproduces the masks (they are keyed by the device generator's seed and stream offset), inactive modules get None, a stand-in's own mask passes
    through."""
    ops = _ops()
    from torch import nn

    class Fixed(nn.Module):
        def tmf_keep_mask(self, training):
            return torch.full((4, 8), 2.0) if training else None
    drops = [nn.Dropout(0.5), nn.Dropout(0.3), nn.Dropout(0.0), nn.Dropout(0.5).eval(), Fixed(), nn.Dropout(1.0), nn.Dropout(0.5)]
    shapes = [(8, 512), (1728, 128), (8, 64), (8, 64), (4, 8), (3, 5), (8, 64)]

    def draw():
        return ops.dropout_keep_masks(list(zip(drops, shapes)), torch.device(DEV))
    torch.manual_seed(1234)
    m = draw()
    m2 = draw()
    torch.manual_seed(1234)                      # resets the device generator's stream offset the masks are keyed by
    r = draw()
    torch.cuda.synchronize()
    assert m[2] is None and m[3] is None and torch.equal(m[4].cpu(), torch.full((4, 8), 2.0)) and not m[5].any()
    for i, keep in ((0, 0.5), (1, 0.7), (6, 0.5)):
        v = m[i]
        assert v.shape == shapes[i] and v.dtype == torch.float32 and v.is_contiguous()
        inv = torch.tensor(1.0 / keep, dtype=torch.float32).item()
        assert bool(((v == 0) | (v == inv)).all())
        n = v.numel()
        rate = (v != 0).float().mean().item()
        assert abs(rate - keep) <= 4 * (keep * (1 - keep) / n) ** 0.5, (i, rate)
        assert torch.equal(v, r[i])                                  # same seed, same call sequence: same masks
        assert not torch.equal(v, m2[i])                             # the next call draws other masks
    assert not torch.equal(m[0][:, :64], m[6])                       # segments of one call are independent streams
    # rows are not copies of each other (the counter runs over the whole segment)
    assert (m[1][0] != m[1][1]).any() and (m[0][0] != m[0][1]).any()


WINO_SHAPES = [
    # B, D, H, W, cin, cout
    (1, 4, 8, 8, 8, 32),            # one brick, one chunk
    (2, 7, 9, 13, 8, 32),           # every brick ragged, odd edges (a 2x2x2 tile half outside the volume)
    (2, 6, 10, 12, 32, 64),         # two channel groups, partial bricks on every axis
    (1, 12, 16, 16, 64, 32),        # eight chunks
    (2, 11, 13, 11, 128, 256),      # the reference's fourth level
    (2, 24, 24, 24, 32, 32),
    # four samples x 4x4x4 bricks (the geometry the persistent kernel takes where it executes fewer tiles)
    (8, 12, 12, 12, 32, 64),        # BASELINE configs[1]'s fourth level: 3x3x3 bricks per sample group, no padding
    (7, 11, 13, 11, 16, 32),        # ADNI's fourth level, ragged on every axis, a last group of three samples
    (3, 4, 4, 4, 8, 32),            # one brick, one sample missing
]


def _wino_u_ref(w):
    """U = G g G^T along the three axes, fp64 (the layout-free transformed filter [cout][cin][4][4][4])."""
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    u = torch.einsum("pa,ocaij->ocpij", G, w.double())
    u = torch.einsum("qi,ocpij->ocpqj", G, u)
    return torch.einsum("rj,ocpqj->ocpqr", G, u)


@pytest.mark.parametrize("shape", WINO_SHAPES)
def test_conv3d_winograd_form(shape):
    """tmf_conv3d_fwd_wino (F(2x2x2, 3x3x3) on the fp32 matrix pipe) against fp64 torch and against the direct kernel:
    z, the BatchNorm statistic partials, the data gradient (same entry, u_dgrad, channel roles swapped), the packed
    weight layouts, run-to-run bit reproducibility."""
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=301)
    w = _rand(cout, cin, 3, 3, 3, seed=302, scale=(cin * 27) ** -0.5)
    xg, wg = _ndhwc(x).to(DEV), w.to(DEV)
    want_d = ops.wino_ok(cout, cin)
    uf, ud = ops.pack_weights_wino(wg, True, want_d)
    # packed layouts: u_fwd[p][cin/8][2][cout][4], input channel 8 g + 4 hs + s; one rounding from the fp64 value
    ur = _wino_u_ref(w)                                                        # [co][ci][4][4][4]
    uf_ref = ur.permute(2, 3, 4, 1, 0).reshape(64, cin // 8, 2, 4, cout).permute(0, 1, 2, 4, 3).float()
    assert torch.equal(uf.cpu(), uf_ref)
    if want_d:
        ud_ref = ur.flip(2, 3, 4).permute(2, 3, 4, 0, 1).reshape(64, cout // 8, 2, 4, cin).permute(0, 1, 2, 4, 3).float()
        # (the transformed FLIPPED filter = the transformed filter with positions 0 <-> 3 swapped on every axis, 1 and 2 kept)
        idx = torch.tensor([3, 1, 2, 0])
        ud_ref = ur[:, :, idx][:, :, :, idx][:, :, :, :, idx].permute(2, 3, 4, 0, 1).reshape(64, cout // 8, 2, 4, cin) \
            .permute(0, 1, 2, 4, 3).float()
        assert torch.equal(ud.cpu(), ud_ref)
    z, part, nblk = ops.conv3d_wino_raw(xg, uf, cin, cout, True)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    assert _relerr(_ncdhw(z.cpu()), ref) < 2e-6
    zd, _, _ = ops.conv3d_raw(xg, ops.pack_weight(wg), cin, cout, 3, False)
    assert _relerr(z.cpu(), zd.cpu()) < 2e-6                                   # two fp32 roundings of the same sums
    n0_, n1_ = B * -(-D // 4) * -(-H // 8) * -(-W // 8), -(-B // 4) * -(-D // 4) * -(-H // 4) * -(-W // 4)
    from transmf_ad_amd import _lib
    nbricks = _lib.query("tmf_conv3d_wino_bricks", B, D, H, W)
    assert nbricks == (n1_ if n1_ < n0_ and ops.wino_p_mode() else n0_)
    # one row of partials per workgroup of the persistent kernel (per compute unit), per brick with the other
    assert nblk == (torch.cuda.get_device_properties(0).multi_processor_count if ops.wino_p_mode() else n0_)
    assert tuple(part.shape) == (nblk, 2, cout)
    if shape[0] > 2:
        assert nbricks == n1_                                                   # (these shapes are here for the folded geometry)
    s1, s2 = part[:, 0].double().sum(0).cpu(), part[:, 1].double().sum(0).cpu()
    zz = z.double().cpu()
    assert (s1 - zz.sum((0, 1, 2, 3))).abs().max().item() <= 2e-6 * zz.abs().sum((0, 1, 2, 3)).max().item()
    assert _relerr(s2, (zz ** 2).sum((0, 1, 2, 3))) < 2e-6
    z2, part2, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, True)
    assert torch.equal(z, z2) and torch.equal(part, part2)
    z3, _, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, False)                   # the instance without statistics
    assert torch.equal(z, z3)
    if want_d:
        dz = _rand(B, cout, D, H, W, seed=303)
        dx, _, _ = ops.conv3d_wino_raw(_ndhwc(dz).to(DEV), ud, cout, cin, False)
        dref = F.conv_transpose3d(dz.double(), w.double(), None, 1, 1)
        assert _relerr(_ncdhw(dx.cpu()), dref) < 2e-6


WINOX_SHAPES = [
    # B, D, H, W, cin, cout — launches the split kernel takes (cin, cout multiples of 32, 4x8x8 bricks of one sample)
    (1, 4, 8, 8, 32, 32),           # one brick, one item per workgroup
    (2, 7, 9, 13, 32, 32),          # every brick ragged
    (1, 8, 16, 16, 32, 64),         # two groups of output channels
    (2, 12, 24, 24, 64, 128),       # four chunks, four groups (216 items: ONE per workgroup on 256 CUs; many per workgroup in test_winograd_capped_grid)
    (2, 9, 17, 21, 128, 64),        # eight chunks, odd edges
    (5, 16, 16, 24, 32, 32),        # more items than compute units on a small device are still a strided list
    # round 6: volumes whose items lie better with the 4-voxel side along h — the kernel then runs TRANSPOSED (its d axis = the
    # tensor's h axis; strides and weight positions trade places)
    (2, 22, 27, 22, 64, 64),        # the reference's 91x109x91 two levels down: 63 instead of 72 items per sample
    (1, 8, 4, 8, 32, 32),           # one transposed item
    (3, 15, 21, 9, 32, 64),         # ragged on every axis, two channel groups
]


def _winox_parts(u, cin, cout):
    """The three bf16 parts the pack kernel writes behind the fp32 tensor u [64][K/8][2][N][4] -> [3][64][K][N] floats
    (layout [p][K/16][part][K half][N][8], K index 16 c + 8 s + 4 half + e -> element 4 s + e of its half)."""
    n = 64 * cin * cout
    raw = torch.empty(0, dtype=torch.int16, device=u.device).set_(u.untyped_storage(), (u.storage_offset() + n) * 2, (3 * n,))
    f = (raw.view(64, cin // 16, 3, 2, cout, 8).to(torch.int32) << 16).view(torch.float32)
    return f.view(64, cin // 16, 3, 2, cout, 2, 4).permute(2, 0, 1, 5, 3, 6, 4).reshape(3, 64, cin, cout)


@pytest.mark.parametrize("shape", WINOX_SHAPES)
def test_conv3d_winograd_split_kernel(shape):
    """conv3d_winox_kernel (csrc/conv3d_winox.hip; the default of tmf_conv3d_fwd_wino where it takes the launch): the Winograd
    products on the bf16 matrix pipe through EXACT 3-way bf16 splits of both fp32 operands.  The packed parts sum to the fp32
    transformed weight bit for bit; z, the statistic partials and the data gradient hold the fp32 kernel's tolerances against
    fp64 torch and lie within fp32 round-off of the fp32 kernel (tmf_set_option("wino_x", 0)); results are bit-reproducible."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, cin, cout = shape
    assert _lib.query("tmf_wino_x_mode") == 1
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1) == b"conv3d_winox_kernel<1>"
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cout, cin, 0) == b"conv3d_winox_kernel<0>"
    x = _rand(B, cin, D, H, W, seed=331)
    w = _rand(cout, cin, 3, 3, 3, seed=332, scale=(cin * 27) ** -0.5)
    xg, wg = _ndhwc(x).to(DEV), w.to(DEV)
    uf, ud = ops.pack_weights_wino(wg, True, True)
    for u, ci, co in ((uf, cin, cout), (ud, cout, cin)):
        parts = _winox_parts(u, ci, co)
        u32 = u.permute(0, 1, 2, 4, 3).reshape(64, ci, co)
        assert torch.equal(parts.double().sum(0), u32.double())                # h + m + l == u, exactly
        assert bool((parts[1].abs() <= parts[0].abs() * 2.0 ** -7).all()) and bool((parts[2].abs() <= parts[0].abs() * 2.0 ** -15).all())
    z, part, nblk = ops.conv3d_wino_raw(xg, uf, cin, cout, True)
    ref = F.conv3d(x.double(), w.double(), None, 1, 1)
    assert _relerr(_ncdhw(z.cpu()), ref) < 2e-6
    _lib.call("tmf_set_option", b"wino_x", 0)
    try:
        assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1).startswith(b"conv3d_wino_p_kernel")
        zf, partf, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, True)
    finally:
        _lib.call("tmf_set_option", b"wino_x", 1)
    assert _relerr(z.cpu(), zf.cpu()) < 2e-6 and not torch.equal(z, zf)        # (another kernel: same sums, other rounding)
    assert tuple(part.shape) == tuple(partf.shape) == (nblk, 2, cout)           # one row per workgroup, as the fp32 kernel
    s1, s2 = part[:, 0].double().sum(0).cpu(), part[:, 1].double().sum(0).cpu()
    zz = z.double().cpu()
    assert (s1 - zz.sum((0, 1, 2, 3))).abs().max().item() <= 2e-6 * zz.abs().sum((0, 1, 2, 3)).max().item()
    assert _relerr(s2, (zz ** 2).sum((0, 1, 2, 3))) < 2e-6
    z2, part2, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, True)
    z3, _, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, False)
    assert torch.equal(z, z2) and torch.equal(part, part2) and torch.equal(z, z3)
    dz = _rand(B, cout, D, H, W, seed=333)
    dx, _, _ = ops.conv3d_wino_raw(_ndhwc(dz).to(DEV), ud, cout, cin, False)
    assert _relerr(_ncdhw(dx.cpu()), F.conv_transpose3d(dz.double(), w.double(), None, 1, 1)) < 2e-6
    # exact on small integers (every partial product and every sum is an integer below 2^24: no rounding anywhere)
    xi = torch.randint(-3, 4, (B, D, H, W, cin), device=DEV).float()
    wi = torch.randint(-2, 3, (cout, cin, 3, 3, 3), device=DEV).float()
    ui, _ = ops.pack_weights_wino(wi, True, False)
    zi, _, _ = ops.conv3d_wino_raw(xi, ui, cin, cout, False)
    refi = F.conv3d(xi.permute(0, 4, 1, 2, 3).double(), wi.double(), None, 1, 1).permute(0, 2, 3, 4, 1)
    assert torch.equal(zi.double(), refi)


def test_conv3d_winograd_form_refuses_other_channel_counts():
    import transmf_ad_amd as T
    ops = _ops()
    assert not ops.wino_ok(4, 32) and not ops.wino_ok(8, 16) and ops.wino_ok(8, 32) and ops.wino_ok(256, 128)
    w = torch.zeros((16, 8, 3, 3, 3), device=DEV)
    with pytest.raises(T.TmfError, match="cout % 32"):
        ops.pack_weights_wino(w, True, False)
    x = torch.zeros((1, 4, 8, 8, 12), device=DEV)
    with pytest.raises(T.TmfError, match="cin % 8"):
        ops.conv3d_wino_raw(x, torch.zeros(64 * 12 * 32, device=DEV), 12, 32, False)


WINO_WGRAD_SHAPES = [
    # B, D, H, W, cin, cout
    (1, 4, 4, 8, 32, 32),           # one stage of one workgroup
    (2, 7, 9, 13, 32, 64),          # every half brick ragged, two output-channel blocks
    (2, 6, 10, 12, 64, 32),         # two input-channel blocks
    (3, 12, 12, 12, 128, 64),       # more (ci, co) blocks than slabs per block
    (2, 24, 24, 24, 32, 32),        # 256 slabs -> two-stage reduction
    (8, 12, 12, 12, 128, 256),      # conv4.0 of the 96^3 input: stages of two samples x 4x4x4 voxels (27 per pair instead of 36)
    (5, 6, 7, 12, 32, 32),          # ... an odd batch (the last pair holds one sample), ragged d and h
    (4, 9, 5, 4, 32, 64),           # ... a volume one such brick wide
]


@pytest.mark.parametrize("shape", WINO_WGRAD_SHAPES)
def test_conv3d_winograd_weight_gradient(shape):
    """tmf_conv3d_wgrad_wino (dU_p = V_p^T Z_p on the fp32 matrix pipe, dw = G^T dU G in fp64) against fp64 torch and the direct
    kernel, both output layouts, run-to-run bit reproducibility."""
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=311)
    dz = _rand(B, cout, D, H, W, seed=312)
    xg, dzg = _ndhwc(x).to(DEV), _ndhwc(dz).to(DEV)
    dw = ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True)
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dz.double(), stride=1, padding=1)
    assert _relerr(dw, ref) < 5e-6
    dd = ops.conv3d_wgrad(xg, dzg, cin, cout, 3, reference_layout=True)
    assert _relerr(dw, dd.cpu()) < 5e-6
    dt = ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=False)
    assert torch.equal(dt.view(3, 3, 3, cin, cout).permute(4, 3, 0, 1, 2).contiguous(), dw)
    assert torch.equal(dw, ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True))


def test_conv3d_winograd_weight_gradient_refuses_other_channel_counts():
    import transmf_ad_amd as T
    ops = _ops()
    assert ops.wgrad_wino_ok(32, 64) and not ops.wgrad_wino_ok(16, 32) and not ops.wgrad_wino_ok(32, 48)
    with pytest.raises(T.TmfError, match="cin % 32"):
        ops.conv3d_wgrad_wino(torch.zeros((1, 4, 4, 8, 16), device=DEV), torch.zeros((1, 4, 4, 8, 32), device=DEV), 16, 32)


@pytest.mark.parametrize("shape,pool", [((2, 7, 9, 13, 8, 32), "max"), ((2, 7, 9, 13, 8, 32), None), ((2, 12, 16, 16, 32, 64), "max"),
                                        ((1, 24, 24, 24, 64, 64), None), ((3, 9, 15, 21, 32, 32), "max"), ((2, 7, 10, 13, 64, 96), None),
                                        ((2, 22, 27, 22, 64, 64), "max"), ((1, 8, 12, 8, 32, 32), None)])     # (transposed items)
def test_conv3d_winograd_eval_block_in_one_pass(shape, pool):
    """tmf_conv3d_fwd_wino_affine: the eval-mode block (conv + folded BatchNorm + LeakyReLU + max pool) in ONE Winograd kernel —
    conv3d_winox_kernel<2 | 3> where the split kernel takes the launch, conv3d_wino_p_kernel<2> otherwise — bitwise what the
    two-kernel sequence of the same family (Winograd conv, then tmf_bn_act_pool_fwd) gives, and fp32-close to fp64 torch."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, cin, cout = shape
    x = _rand(B, cin, D, H, W, seed=321)
    w = _rand(cout, cin, 3, 3, 3, seed=322, scale=(cin * 27) ** -0.5)
    sc, sh = 1 + _rand(cout, seed=323, scale=0.2), _rand(cout, seed=324, scale=0.2)
    xg = _ndhwc(x).to(DEV)
    uf, _ = ops.pack_weights_wino(w.to(DEV), True, False)
    scg, shg = sc.to(DEV), sh.to(DEV)
    pc = _lib.pool_code(pool)
    oshape = (B, D // 2, H // 2, W // 2, cout) if pool else (B, D, H, W, cout)
    ys = {}
    for xmode in (1, 0):        # the split kernel's eval modes (where it takes the launch) and the fp32 kernel's: each against ITS two-kernel sequence
        _lib.call("tmf_set_option", b"wino_x", xmode)
        try:
            y = torch.full(oshape, float("nan"), device=DEV)
            _lib.call("tmf_conv3d_fwd_wino_affine", xg.data_ptr(), uf.data_ptr(), scg.data_ptr(), shg.data_ptr(), y.data_ptr(),
                      B, D, H, W, cin, cout, pc, 0.01, ops._stream())
            z, _, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, False)
        finally:
            _lib.call("tmf_set_option", b"wino_x", 1)
        y2 = torch.empty(oshape, device=DEV)
        _lib.call("tmf_bn_act_pool_fwd_t", z.data_ptr(), scg.data_ptr(), shg.data_ptr(), y2.data_ptr(), B, D, H, W, cout, pc, 0.01, 0,
                  ops._stream())
        assert torch.equal(y, y2), xmode
        ys[xmode] = y
    y = ys[1]
    assert (ys[1] - ys[0]).abs().max().item() <= 3e-6 * ys[0].abs().max().item()
    if cin % 32 == 0:
        assert not torch.equal(ys[1], ys[0])                                    # (the split kernel did take it)
    ref = F.leaky_relu(F.conv3d(x.double(), w.double(), None, 1, 1) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1), 0.01)
    if pool:
        ref = F.max_pool3d(ref, 2, 2)
    assert _relerr(_ncdhw(y.cpu()), ref) < 3e-6


@pytest.fixture(params=[1, 7, 16], ids=["cus1", "cus7", "cus16"])
def wino_cus(request):
    """Run a raw-op test with the persistent Winograd kernels capped at n workgroups (tmf_set_option("wino_cus", n)): every
    workgroup walks many items, and a launch splits into windows of n x (item table) items.  1: one workgroup takes every item;
    7: divides no 3- or 5-group cout (the split kernel's workgroups change channel group from item to item); 16: the XCD remap
    of the item order.  Raw ops only — a model's buffers are sized under the setting they were planned with."""
    from transmf_ad_amd import _lib
    _lib.call("tmf_set_option", b"wino_cus", request.param)
    try:
        yield request.param
    finally:
        _lib.call("tmf_set_option", b"wino_cus", 0)


def _wino_tab(kernel):
    """item-table entries per workgroup (= items per workgroup and launch) of a persistent Winograd forward kernel"""
    if kernel.startswith("conv3d_winox_kernel"):
        return 256
    return 448 if kernel.endswith(", 1>") else 768         # conv3d_wino_p_kernel<MODE, GEOM>: PGeom<GEOM>::TAB


def _wino_first_grid(items, ncu, tab):
    """workgroups of a launch's first window (tmf_winox_launch / launch_wino_p_g): min(n, ncu), evened to the rounds it needs"""
    n = min(items, ncu * tab)
    if n <= ncu:
        return n
    rounds = -(-n // ncu)
    return -(-n // rounds)


def _wino_items(B, D, H, W, cin, cout):
    from transmf_ad_amd import _lib
    return _lib.query("tmf_conv3d_wino_bricks2", B, D, H, W, cin, cout) * (cout // 32)


def _wino_fwd_stats(xg, uf, cin, cout):
    """tmf_conv3d_fwd_wino through the C ABI into NaN-prefilled z and statistics ((tmf_conv3d_wino_stat_blocks, 2, cout))"""
    from transmf_ad_amd import _lib
    B, D, H, W = xg.shape[:4]
    rows = _lib.query("tmf_conv3d_wino_stat_blocks", B, D, H, W)
    z = torch.full((B, D, H, W, cout), float("nan"), device=DEV)
    part = torch.full((rows, 2, cout), float("nan"), device=DEV)
    _lib.call("tmf_conv3d_fwd_wino", xg.data_ptr(), uf.data_ptr(), z.data_ptr(), part.data_ptr(), B, D, H, W, cin, cout, _ops()._stream())
    return z, part


def _wino_eval_block(xg, uf, scg, shg, cin, cout, pool):
    from transmf_ad_amd import _lib
    B, D, H, W = xg.shape[:4]
    y = torch.full((B, D // 2, H // 2, W // 2, cout) if pool else (B, D, H, W, cout), float("nan"), device=DEV)
    _lib.call("tmf_conv3d_fwd_wino_affine", xg.data_ptr(), uf.data_ptr(), scg.data_ptr(), shg.data_ptr(), y.data_ptr(),
              B, D, H, W, cin, cout, _lib.pool_code(pool), 0.01, _ops()._stream())
    return y


CAPPED_CASES = [
    # (B, D, H, W, cin, cout), wino_x, forward kernel, what the case is there for (asserted in the test):
    #   windows  more items than one window at cap 1 (later windows add into the rows: stat_accum)
    #   cout3/5, cin3/5  3 or 5 channel groups in the forward (statistics) / in the data gradient
    #   transposed  the split kernel's d axis is the tensor's h axis;  short  a last group of fewer than 4 samples
    #   flush7  at cap 7 the split kernel's workgroups change channel group with every item (statistics flush, affine reload)
    #   remap16  the first window's grid at cap 16 is a multiple of 8 (the XCD remap of the item order)
    ((2, 12, 24, 24, 32, 160), 1, "conv3d_winox_kernel<1>", "windows cout5 flush7 remap16"),
    ((1, 4, 16, 56, 160, 96), 1, "conv3d_winox_kernel<1>", "cout3 cin5 flush7"),
    ((2, 7, 9, 13, 96, 64), 1, "conv3d_winox_kernel<1>", "cin3"),                   # every brick ragged
    ((2, 12, 24, 24, 64, 128), 1, "conv3d_winox_kernel<1>", "remap16"),
    ((2, 22, 27, 22, 64, 64), 1, "conv3d_winox_kernel<1>", "transposed remap16"),
    ((2, 24, 32, 32, 8, 160), 1, "conv3d_wino_p_kernel<1, 0>", "windows cout5 remap16"),
    ((7, 11, 13, 11, 16, 32), 1, "conv3d_wino_p_kernel<1, 1>", "short"),
    ((8, 12, 12, 16, 8, 256), 1, "conv3d_wino_p_kernel<1, 1>", "windows remap16"),
    ((1, 4, 16, 56, 160, 96), 0, "conv3d_wino_p_kernel<1, 0>", "cout3 cin5"),
]
_CAPPED_BASE = {}


def _capped_outputs(xg, uf, ud, dzg, scg, shg, cin, cout):
    z, part = _wino_fwd_stats(xg, uf, cin, cout)
    z2, part2 = _wino_fwd_stats(xg, uf, cin, cout)
    out = {"z": z, "part": part, "z2": z2, "part2": part2}
    if ud is not None:
        out["dx"], _, _ = _ops().conv3d_wino_raw(dzg, ud, cout, cin, False)
    for pool in (None, "max"):
        out[f"y_{pool}"] = _wino_eval_block(xg, uf, scg, shg, cin, cout, pool)
        out[f"y2_{pool}"] = _wino_eval_block(xg, uf, scg, shg, cin, cout, pool)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", CAPPED_CASES, ids=lambda c: "x{}-{}".format(c[1], "x".join(map(str, c[0]))))
def test_winograd_capped_grid(case, wino_cus):
    """The persistent Winograd kernels (conv3d_winox_kernel<0..3>, conv3d_wino_p_kernel<*, 0 | 1>) with their workgroups capped
    (tmf_set_option("wino_cus", n)), so that every workgroup walks a strided list of items: the cross-item prefetch of halo and
    weights, the statistics flush where the channel group changes, the affine reload per group, windows beyond the item table and
    the XCD remap all run.  An item's arithmetic belongs to its workgroup alone: z, dx and the eval block are BIT-identical to the
    uncapped launch; each holds its fp64 bound; the statistic rows (C ABI, NaN-prefilled) are finite, exactly 0 at and past the
    first window's grid, and sum to z's fp64 sums; every output repeats bit for bit."""
    from transmf_ad_amd import _lib
    ops = _ops()
    shape, xmode, kernel, tags = case
    B, D, H, W, cin, cout = shape
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.call("tmf_set_option", b"wino_x", xmode)
    try:
        names = [_lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1),
                 _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cout, cin, 0)]
        assert names[0].decode() == kernel
        tab = _wino_tab(kernel)
        items = _wino_items(B, D, H, W, cin, cout)
        want_d = ops.wino_ok(cout, cin)
        # what the case is there for
        for t in tags.split():
            if t == "windows":
                assert items > tab                                             # more than one window at cap 1
            elif t in ("cout3", "cout5", "cin3", "cin5"):
                n = int(t[-1])
                assert (cout if t[1] == "o" else cin) == 32 * n and (t[1] == "o" or want_d)
            elif t == "transposed":
                assert -(-H // 4) * -(-D // 8) < -(-D // 4) * -(-H // 8)
            elif t == "short":
                assert B % 4 != 0 and tab == 448
            elif t == "flush7":                                                # (the channel group is the split kernel's fast index)
                assert tab == 256 and _wino_first_grid(items, 7, tab) % (cout // 32) != 0
            else:
                assert t == "remap16" and _wino_first_grid(items, 16, tab) % 8 == 0
        if shape + (xmode,) not in _CAPPED_BASE:                               # inputs, fp64 references, the uncapped launch
            x = _rand(B, cin, D, H, W, seed=341)
            w = _rand(cout, cin, 3, 3, 3, seed=342, scale=(cin * 27) ** -0.5)
            dz = _rand(B, cout, D, H, W, seed=343)
            sc, sh = 1 + _rand(cout, seed=344, scale=0.2), _rand(cout, seed=345, scale=0.2)
            g = {"xg": _ndhwc(x).to(DEV), "dzg": _ndhwc(dz).to(DEV), "scg": sc.to(DEV), "shg": sh.to(DEV)}
            g["uf"], g["ud"] = ops.pack_weights_wino(w.to(DEV), True, want_d)
            ref = {"z": F.conv3d(x.double(), w.double(), None, 1, 1)}
            if want_d:
                ref["dx"] = F.conv_transpose3d(dz.double(), w.double(), None, 1, 1)
            ref["y_None"] = F.leaky_relu(ref["z"] * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1), 0.01)
            ref["y_max"] = F.max_pool3d(ref["y_None"], 2, 2)
            _lib.call("tmf_set_option", b"wino_cus", 0)
            try:
                base = _capped_outputs(g["xg"], g["uf"], g["ud"], g["dzg"], g["scg"], g["shg"], cin, cout)
                base_names = [_lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1),
                              _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cout, cin, 0)]
            finally:
                _lib.call("tmf_set_option", b"wino_cus", wino_cus)
            _CAPPED_BASE[shape + (xmode,)] = g, ref, base, base_names
        g, ref, base, base_names = _CAPPED_BASE[shape + (xmode,)]
        assert names == base_names
        got = _capped_outputs(g["xg"], g["uf"], g["ud"], g["dzg"], g["scg"], g["shg"], cin, cout)
    finally:
        _lib.call("tmf_set_option", b"wino_x", 1)
    cap = min(wino_cus, ncu)
    for res, n_cu in ((got, cap), (base, ncu)):
        # bitwise repeatable, and the capped grid computes the uncapped grid's bits
        for k in ("z", "part", "y_None", "y_max"):
            k2 = k.replace("_", "2_") if k.startswith("y") else k + "2"
            assert torch.equal(res[k], res[k2]), (k, n_cu)
        for k in ("z", "dx", "y_None", "y_max"):
            if k in res:
                assert torch.equal(res[k], base[k]), (k, n_cu)
                assert _relerr(_ncdhw(res[k].cpu()), ref[k]) < (3e-6 if k.startswith("y") else 2e-6), (k, n_cu)
        # statistics: one row per workgroup; rows at and past the first window's grid are zeros, none is left unwritten
        part = res["part"].double().cpu()
        grid = _wino_first_grid(items, n_cu, tab)
        assert part.shape == (n_cu, 2, cout) and bool(torch.isfinite(part).all())
        assert bool((part[grid:] == 0).all()), (grid, n_cu)
        s1, s2 = part[:, 0].sum(0), part[:, 1].sum(0)
        zz = res["z"].double().cpu()
        assert (s1 - zz.sum((0, 1, 2, 3))).abs().max().item() <= 2e-6 * zz.abs().sum((0, 1, 2, 3)).max().item(), n_cu
        assert _relerr(s2, (zz ** 2).sum((0, 1, 2, 3))) < 2e-6, n_cu


WINO_FULL_LAYERS = [
    # (B, D, H, W, cin, cout), forward kernel, crops of z / dx (sample, d0, h0, w0) of size `size` (clipped to the volume): the two
    # corners (the far one holds the last sample and the ragged last brick), bricks seams straddled on every axis
    ((8, 48, 48, 48, 32, 64), "conv3d_winox_kernel<1>", (6, 10, 10),         # conv2.3 at BASELINE size: 6 912 items
     [(0, 0, 0, 0), (7, 42, 38, 38), (3, 10, 14, 22), (7, 18, 30, 6)]),
    ((8, 12, 12, 12, 128, 256), "conv3d_wino_p_kernel<1, 1>", (6, 6, 6),     # conv4.0: four samples x 4x4x4 bricks, 432 items
     [(0, 0, 0, 0), (7, 6, 6, 6), (4, 3, 3, 3), (3, 1, 5, 2)]),
    ((2, 45, 54, 45, 32, 64), "conv3d_winox_kernel<1>", (6, 10, 10),         # ADNI 91x109x91, first pooled level: ragged on every axis
     [(0, 0, 0, 0), (1, 39, 44, 35), (0, 18, 22, 14), (0, 37, 3, 33)]),
    ((2, 22, 27, 22, 64, 64), "conv3d_winox_kernel<1>", (10, 6, 10),         # ... two levels down: transposed items (4 voxels along h)
     [(0, 0, 0, 0), (1, 12, 21, 12), (0, 3, 6, 5), (1, 11, 13, 11)]),
]


def _conv_crop_ref(vp, w, b, o, size):
    """fp64 3x3x3 convolution of one crop of the output: the crop's window of the zero-padded NDHWC input vp, no padding"""
    sl = tuple(slice(o[i], o[i] + size[i] + 2) for i in range(3))
    v = vp[(b,) + sl].double().cpu().permute(3, 0, 1, 2).unsqueeze(0)
    return F.conv3d(v, w.double().cpu())[0].permute(1, 2, 3, 0)


@pytest.mark.parametrize("layer", WINO_FULL_LAYERS, ids=lambda l: "x".join(map(str, l[0])))
def test_full_size_winograd_conv_properties(layer):
    """The default Winograd kernels at full size, default grid (the twin of test_full_size_conv_properties): (i) exact power-of-
    two homogeneity of forward, statistics (x 4 / x 16), data and weight gradient — the exact bf16 splits and the fp64 filter
    transform commute with a scale by 4; (ii) adjointness <dz, conv(x, w)> == <wgrad(x, dz), w> == <dgrad(dz, w), x>; (iii) crops
    of z and dx against fp64 torch on the padded input window: corners, brick seams, the ragged last brick, the last sample."""
    from transmf_ad_amd import _lib
    ops = _ops()
    (B, D, H, W, cin, cout), kernel, size, crops = layer
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1).decode() == kernel
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cout, cin, 0).decode() == kernel.replace("<1", "<0")
    if (H, W) == (27, 22):
        assert -(-H // 4) * -(-D // 8) < -(-D // 4) * -(-H // 8)             # (the transposed orientation)
    g = torch.Generator(device=DEV).manual_seed(17)
    x = torch.randn((B, D, H, W, cin), device=DEV, generator=g)
    dz = torch.randn((B, D, H, W, cout), device=DEV, generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), device=DEV, generator=g) * (27 * cin) ** -0.5
    uf, ud = ops.pack_weights_wino(w, True, True)
    z, part, _ = ops.conv3d_wino_raw(x, uf, cin, cout, True)
    z4, part4, _ = ops.conv3d_wino_raw(x * 4.0, uf, cin, cout, True)
    assert torch.equal(z4, z * 4.0)
    assert torch.equal(part4[:, 0], part[:, 0] * 4.0) and torch.equal(part4[:, 1], part[:, 1] * 16.0)
    zs = z.double().sum(dim=(0, 1, 2, 3))
    assert (part[:, 0].double().sum(0) - zs).abs().max().item() <= 2e-6 * z.double().abs().sum(dim=(0, 1, 2, 3)).max().item()
    assert _relerr(part[:, 1].double().sum(0), (z.double() ** 2).sum(dim=(0, 1, 2, 3)).cpu()) < 2e-6
    dx, _, _ = ops.conv3d_wino_raw(dz, ud, cout, cin, False)
    dx4, _, _ = ops.conv3d_wino_raw(dz * 4.0, ud, cout, cin, False)
    assert torch.equal(dx4, dx * 4.0)
    dw = ops.conv3d_wgrad_wino(x, dz, cin, cout, reference_layout=True)
    dw4 = ops.conv3d_wgrad_wino(x * 4.0, dz, cin, cout, reference_layout=True)
    assert torch.equal(dw4, dw * 4.0)
    a = (dz.double() * z.double()).sum().item()
    b = (dw.double() * w.double()).sum().item()
    c = (dx.double() * x.double()).sum().item()
    scale = (dz.double().abs() * z.double().abs()).sum().item()
    assert abs(a - b) <= 1e-6 * scale and abs(a - c) <= 1e-6 * scale, (a, b, c, scale)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    dzp = F.pad(dz, (0, 0, 1, 1, 1, 1, 1, 1))
    wt = w.flip(2, 3, 4).transpose(0, 1)                                      # the data gradient as a convolution
    for b_, d0, h0, w0 in crops:
        o = (d0, h0, w0)
        assert all(0 <= o[i] and o[i] + size[i] <= (D, H, W)[i] for i in range(3)) and 0 <= b_ < B
        sl = (b_,) + tuple(slice(o[i], o[i] + size[i]) for i in range(3))
        assert _relerr(z[sl], _conv_crop_ref(xp, w, b_, o, size)) < 2e-6, (b_, o)
        assert _relerr(dx[sl], _conv_crop_ref(dzp, wt, b_, o, size)) < 2e-6, (b_, o)


def test_full_size_winograd_eval_block_is_the_two_kernel_sequence():
    """The one-pass eval block (conv3d_winox_kernel<3>: conv, folded BatchNorm, LeakyReLU, 2x2x2 max pool) at full size, 8 x 48^3,
    32 -> 64, default grid: bitwise the Winograd conv followed by tmf_bn_act_pool_fwd_t."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, S, cin, cout = 8, 48, 32, 64
    g = torch.Generator(device=DEV).manual_seed(19)
    x = torch.randn((B, S, S, S, cin), device=DEV, generator=g)
    w = torch.randn((cout, cin, 3, 3, 3), device=DEV, generator=g) * (27 * cin) ** -0.5
    sc = 1 + 0.2 * torch.randn((cout,), device=DEV, generator=g)
    sh = 0.2 * torch.randn((cout,), device=DEV, generator=g)
    uf, _ = ops.pack_weights_wino(w, True, False)
    y = _wino_eval_block(x, uf, sc, sh, cin, cout, "max")
    z, _, _ = ops.conv3d_wino_raw(x, uf, cin, cout, False)
    y2 = torch.empty_like(y)
    _lib.call("tmf_bn_act_pool_fwd_t", z.data_ptr(), sc.data_ptr(), sh.data_ptr(), y2.data_ptr(), B, S, S, S, cout,
              _lib.pool_code("max"), 0.01, 0, ops._stream())
    assert torch.equal(y, y2)


@pytest.mark.parametrize("scale", [1.0, 1000.0])
def test_first_block_one_pass_backward_on_uncentred_input(scale):
    """tmf_c1_bwd_fused on a volume that is NOT centred (a smooth field around 3, and the same at raw-intensity scale): in
    dw = s [D - c0 S_t - c1 / sigma ((G w)_t - mu S_t)] the fp32 sum D and c0 S_t nearly cancel there, a step the two-pass form avoids
    by forming the mean-free dz per voxel first (the advisor's finding, round 5).  dw / dgamma / dbeta of the whole block against fp64
    torch and against the two-pass backward (c1_gram 0): the one-pass form is no further from fp64 than 3 x the two-pass one."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, C = 2, 16, 24, 40, 32
    g = torch.Generator().manual_seed(23)
    zz_, yy_, xx_ = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    x = ((3.0 + torch.sin(0.21 * zz_ + 0.13 * yy_) * torch.cos(0.17 * xx_)).float().expand(B, D, H, W)
         + 0.05 * torch.rand((B, D, H, W), generator=g)).contiguous() * scale
    w = torch.randn((C, 1, 3, 3, 3), generator=g) * 0.3 / scale
    conv = torch.nn.Conv3d(1, C, 3, padding=1).to(DEV)
    bn = torch.nn.BatchNorm3d(C).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.to(DEV))
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    go = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g).to(DEV)
    xg = x.to(DEV)
    res = {}
    for gram_opt in (1, 0):
        _lib.call("tmf_set_option", b"c1_gram", gram_opt)
        try:
            for p_ in (conv.weight, bn.weight, bn.bias):
                p_.grad = None
            y = ops.conv_bn_act_pool(xg.unsqueeze(-1), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean.clone(),
                                     bn.running_var.clone(), True, pool="max")
            y.backward(go)
            torch.cuda.synchronize()
        finally:
            _lib.call("tmf_set_option", b"c1_gram", 1)
        res[gram_opt] = (conv.weight.grad.cpu().clone(), bn.weight.grad.cpu().clone(), bn.bias.grad.cpu().clone())
    w64 = w.double().requires_grad_(True)
    g64, b64 = bn.weight.detach().double().cpu().requires_grad_(True), bn.bias.detach().double().cpu().requires_grad_(True)
    zz = F.conv3d(x.double().unsqueeze(1), w64, conv.bias.detach().double().cpu(), padding=1)
    yy = F.max_pool3d(F.leaky_relu(F.batch_norm(zz, None, None, g64, b64, True, 0.1, 1e-5), 0.01), 2)
    yy.backward(go.double().permute(0, 4, 1, 2, 3).cpu())
    for i, ref in enumerate((w64.grad, g64.grad, b64.grad)):
        e1 = (res[1][i].double() - ref).abs().max().item() / ref.abs().max().item()
        e0 = (res[0][i].double() - ref).abs().max().item() / ref.abs().max().item()
        assert e1 <= max(3.0 * e0, 2e-5), (i, e1, e0)


@pytest.mark.parametrize("out_bf16", [False, True])
@pytest.mark.parametrize("shape", [(2, 16, 24, 40, 32), (1, 9, 13, 35, 32), (3, 8, 10, 33, 16)])
def test_first_block_gram_path_in_the_bf16_mode(shape, out_bf16):
    """Round 6: tmf_c1_stats_g_bf16 / tmf_c1_bwd_fused_bf16 — the bf16 mode multiplies the volume and the taps ROUNDED to bf16
    (conv1_fused_kernel<.., true>), so G, S_t are those of the rounded volume and the forms use the rounded taps: G / S_t against an
    explicit fp64 evaluation on the rounded volume, the statistic rows against the sums of the exactly computed z of the rounded
    operands; the whole block (one pass) against the bf16 mode's two-pass backward ("c1_gram" 0) and against fp64 torch on the rounded
    operands — no further from it than the two-pass form, which rounds dz to bf16 once more; bit-identical run to run.  The mode takes
    the path under "c1_gram" 2 only (it is slower there: DESIGN 3.16), so that is what the one-pass runs set."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(12)
    x = torch.rand((B, D, H, W), generator=g) * 0.8 + 0.1
    w = torch.randn((C, 1, 3, 3, 3), generator=g) * 0.3
    xb, wb = x.bfloat16().double(), w.bfloat16().double()
    xg = x.to(DEV)
    wp = ops.pack_weight(w.to(DEV)).view(27, C)
    gbytes = _lib.query("tmf_c1_gram_bytes", B, D, H, W, C)
    assert gbytes > 0
    part = torch.full((2, 2, C), float("nan"), device=DEV)
    gram = torch.empty(gbytes // 8, device=DEV, dtype=torch.float64)
    _lib.call("tmf_c1_stats_g_bf16", xg.data_ptr(), wp.data_ptr(), part.data_ptr(), gram.data_ptr(), gbytes, B, D, H, W, C, ops._stream())
    torch.cuda.synchronize()
    xp = F.pad(xb, (2, 2, 2, 2, 2, 2))
    sh = torch.stack([xp[:, 1 + t // 9:1 + t // 9 + D, 1 + (t // 3) % 3:1 + (t // 3) % 3 + H, 1 + t % 3:1 + t % 3 + W].reshape(-1)
                      for t in range(27)])
    G_ref, S_ref = sh @ sh.t(), sh.sum(1)
    assert (gram[:729].cpu().view(27, 27) - G_ref).abs().max().item() <= 1e-12 * G_ref.abs().max().item()
    assert (gram[729:756].cpu() - S_ref).abs().max().item() <= 1e-12 * S_ref.abs().max().item()
    z = F.conv3d(xb.unsqueeze(1), wb, None, 1, 1)
    s1 = (part[0, 0].double() + part[1, 0].double()).cpu()
    s2 = (part[0, 1].double() + part[1, 1].double()).cpu()
    assert (s1 - z.sum((0, 2, 3, 4))).abs().max().item() <= 1e-9 * z.abs().sum((0, 2, 3, 4)).max().item()
    assert ((s2 - (z * z).sum((0, 2, 3, 4))).abs() / (z * z).sum((0, 2, 3, 4))).max().item() <= 1e-9
    # the whole block in the bf16 mode, both backward forms
    prec = ops.make_precision("bf16", "bf16" if out_bf16 else "fp32")
    conv = torch.nn.Conv3d(1, C, 3, padding=1).to(DEV)
    bn = torch.nn.BatchNorm3d(C).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.to(DEV))
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    go = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g)
    if out_bf16:
        go = go.bfloat16()
    gog = go.to(DEV)
    res = {}
    assert _lib.query("tmf_c1_gram_bytes_bf16", B, D, H, W, C) == 0                  # the default: fp32 only
    for gram_opt in (2, 1, 2):
        _lib.call("tmf_set_option", b"c1_gram", gram_opt)
        try:
            assert (_lib.query("tmf_c1_gram_bytes_bf16", B, D, H, W, C) > 0) == (gram_opt == 2)
            for p_ in (conv.weight, bn.weight, bn.bias):
                p_.grad = None
            y = ops.conv_bn_act_pool(xg.unsqueeze(-1), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean.clone(),
                                     bn.running_var.clone(), True, pool="max", out_bf16=out_bf16, precision=prec)
            assert y.dtype == (torch.bfloat16 if out_bf16 else torch.float32)
            y.backward(gog)
            torch.cuda.synchronize()
        finally:
            _lib.call("tmf_set_option", b"c1_gram", 1)
        res.setdefault(gram_opt, []).append((y.detach().float().cpu(), conv.weight.grad.cpu().clone(), bn.weight.grad.cpu().clone(),
                                             bn.bias.grad.cpu().clone()))
    a, a2 = res[2]
    b = res[1][0]
    assert all(torch.equal(u, v) for u, v in zip(a, a2))
    w64 = wb.clone().requires_grad_(True)
    g64, b64 = bn.weight.detach().double().cpu().requires_grad_(True), bn.bias.detach().double().cpu().requires_grad_(True)
    zz = F.conv3d(xb.unsqueeze(1), w64, conv.bias.detach().double().cpu(), padding=1)
    yy = F.max_pool3d(F.leaky_relu(F.batch_norm(zz, None, None, g64, b64, True, 0.1, 1e-5), 0.01), 2)
    yy.backward(go.double().permute(0, 4, 1, 2, 3))
    assert _relerr(_ncdhw(a[0]), yy.detach()) < (1e-2 if out_bf16 else 2e-5)
    for i, ref in enumerate((w64.grad, g64.grad, b64.grad)):
        e1 = (a[1 + i].double() - ref).abs().max().item() / ref.abs().max().item()
        e0 = (b[1 + i].double() - ref).abs().max().item() / ref.abs().max().item()
        assert e1 <= max(1.5 * e0, 2e-5), (i, e1, e0)


@pytest.mark.parametrize("shape", [(2, 16, 24, 40, 32), (1, 9, 13, 35, 32), (3, 8, 10, 33, 16), (2, 17, 16, 19, 8)])
def test_first_block_z_as_exact_bf16_splits(shape):
    """Round 6, "c1_split" (default 1): the fp32 passes of the first block compute z on the bf16 matrix pipe from EXACT 3-way bf16
    splits of the volume and the taps (six partial products; conv1_fused_kernel<.., SPLIT>).  Against the fp32-MFMA passes
    ("c1_split" 0) and fp64: the block's output, statistics and all three gradients — no further from fp64 than the fp32 form (x 1.5)
    —, EXACT equality with it on small integers (every product and sum representable), and bit-identical results run to run."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(31)
    assert _lib.query("tmf_c1_split_mode") == 1

    def block(x, w, gamma, beta, go, split, gram):
        _lib.call("tmf_set_option", b"c1_split", split)
        _lib.call("tmf_set_option", b"c1_gram", gram)
        try:
            conv = torch.nn.Conv3d(1, C, 3, padding=1).to(DEV)
            bn = torch.nn.BatchNorm3d(C).to(DEV)
            with torch.no_grad():
                conv.weight.copy_(w.to(DEV)); bn.weight.copy_(gamma.to(DEV)); bn.bias.copy_(beta.to(DEV))
                conv.bias.fill_(0.25)
            y = ops.conv_bn_act_pool(x.to(DEV).unsqueeze(-1), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
                                     bn.running_var, True, pool="max")
            y.backward(go.to(DEV))
            torch.cuda.synchronize()
            return [t.detach().cpu().clone() for t in (y, conv.weight.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]
        finally:
            _lib.call("tmf_set_option", b"c1_split", 1)
            _lib.call("tmf_set_option", b"c1_gram", 1)

    x = torch.rand((B, D, H, W), generator=g) * 3.0 + 0.1
    w = torch.randn((C, 1, 3, 3, 3), generator=g) * 0.3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) * 0.4 - 0.2
    go = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g)
    w64 = w.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    zz = F.conv3d(x.double().unsqueeze(1), w64, None, padding=1)
    yy = F.max_pool3d(F.leaky_relu(F.batch_norm(zz, None, None, g64, b64, True, 0.1, 1e-5), 0.01), 2)
    yy.backward(go.double().permute(0, 4, 1, 2, 3))
    ref = [yy.detach(), w64.grad, g64.grad, b64.grad]
    for gram in (1, 0):                                   # the one-pass (Gram) and the recomputing passes: all five kernel modes
        a, a2, b = block(x, w, gamma, beta, go, 1, gram), block(x, w, gamma, beta, go, 1, gram), block(x, w, gamma, beta, go, 0, gram)
        assert all(torch.equal(u, v) for u, v in zip(a, a2))
        assert _relerr(_ncdhw(a[0]), ref[0]) < 3e-6
        for i in (1, 2, 3):
            e1 = (a[i].double() - ref[i]).abs().max().item() / ref[i].abs().max().item()
            e0 = (b[i].double() - ref[i]).abs().max().item() / ref[i].abs().max().item()
            assert e1 <= max(1.5 * e0, 5e-6), (gram, i, e1, e0)
        for u, v in zip(a[4:], b[4:]):
            assert (u - v).abs().max().item() <= 2e-6 * max(1.0, v.abs().max().item())
    # small integers: every partial product and every sum is exact in both forms -> the same z bit for bit, hence the same block
    xi = torch.randint(-4, 5, (B, D, H, W), generator=g).float()
    wi = torch.randint(-3, 4, (C, 1, 3, 3, 3), generator=g).float()
    a, b = block(xi, wi, gamma, beta, go, 1, 0), block(xi, wi, gamma, beta, go, 0, 0)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    # ... and values that NEED all three parts (24 significant bits)
    xf = (torch.randint(1 << 23, 1 << 24, (B, D, H, W), generator=g).float() * 2.0 ** -20)
    wf = (torch.randint(1 << 23, 1 << 24, (C, 1, 3, 3, 3), generator=g).float() * 2.0 ** -26) * (torch.randint(0, 2, (C, 1, 3, 3, 3), generator=g) * 2 - 1)
    a = block(xf, wf, gamma, beta, go, 1, 1)
    zz = F.conv3d(xf.double().unsqueeze(1), wf.double(), None, padding=1)
    yy = F.max_pool3d(F.leaky_relu(F.batch_norm(zz, None, None, gamma.double(), beta.double(), True, 0.1, 1e-5), 0.01), 2)
    assert _relerr(_ncdhw(a[0]), yy) < 3e-6


C1_FUSED_SHAPES = [(2, 16, 24, 40, 32), (1, 9, 13, 35, 32), (3, 8, 10, 33, 16), (5, 17, 16, 19, 8), (8, 48, 48, 48, 32)]


@pytest.mark.parametrize("shape", C1_FUSED_SHAPES)
def test_first_block_gram_data_and_one_pass_backward(shape):
    """tmf_c1_stats_g (csrc/conv1_gram.hip): the exact tap Gram matrix G[t][t'] = sum_v x~(v + t) x~(v + t') and the shifted sums S_t
    of the zero-padded volume against an explicit fp64 evaluation; tmf_c1_bwd_fused (BatchNorm sums and D = x (*) dy in ONE
    recomputing pass, dw from G) against the two-pass backward (tmf_c1_bwd_reduce + tmf_bn_bwd_finalize + tmf_c1_bwd_wgrad) and
    against fp64 torch through the whole block; bit-identical run to run."""
    from transmf_ad_amd import _lib
    ops = _ops()
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(11)
    x = torch.rand((B, D, H, W), generator=g) * 0.8 + 0.1
    w = torch.randn((C, 1, 3, 3, 3), generator=g) * 0.3
    xg = x.to(DEV)
    wp = ops.pack_weight(w.to(DEV)).view(27, C)
    nblk = _lib.query("tmf_c1_blocks", B, D, H, W, C)
    gbytes = _lib.query("tmf_c1_gram_bytes", B, D, H, W, C)
    assert gbytes > 0
    part = torch.full((nblk, 2, C), float("nan"), device=DEV)
    gram = torch.empty(gbytes // 8, device=DEV, dtype=torch.float64)
    _lib.call("tmf_c1_stats_g", xg.data_ptr(), wp.data_ptr(), part.data_ptr(), gram.data_ptr(), gbytes, B, D, H, W, C, ops._stream())
    torch.cuda.synchronize()
    xp = F.pad(x.double(), (2, 2, 2, 2, 2, 2))                                    # shifted copies of the zero-padded volume over V
    sh = torch.stack([xp[:, 1 + t // 9:1 + t // 9 + D, 1 + (t // 3) % 3:1 + (t // 3) % 3 + H, 1 + t % 3:1 + t % 3 + W].reshape(-1)
                      for t in range(27)])
    G_ref, S_ref = sh @ sh.t(), sh.sum(1)
    G = gram[:729].cpu().view(27, 27)
    assert (G - G_ref).abs().max().item() <= 1e-12 * G_ref.abs().max().item()
    assert (gram[729:756].cpu() - S_ref).abs().max().item() <= 1e-12 * S_ref.abs().max().item()
    assert abs(gram[756].item() - x.double().sum().item()) <= 1e-12 * x.double().sum().item()
    # statistics rows 0 / 1 (high + low halves) = the sums of the exactly computed z
    z = F.conv3d(x.double().unsqueeze(1), w.double(), None, 1, 1)
    s1 = (part[0, 0].double() + part[1, 0].double()).cpu()
    s2 = (part[0, 1].double() + part[1, 1].double()).cpu()
    assert (s1 - z.sum((0, 2, 3, 4))).abs().max().item() <= 1e-9 * z.abs().sum((0, 2, 3, 4)).max().item()
    assert ((s2 - (z * z).sum((0, 2, 3, 4))).abs() / (z * z).sum((0, 2, 3, 4))).max().item() <= 1e-9
    # ... and on a smooth volume with an offset (wide filters cancel there): mean and 1 / sigma after tmf_bn_finalize against fp64
    # and against the recomputing pass ("c1_gram" 0: tmf_c1_gram_bytes() = 0, callers run conv1_fused_kernel<0>)
    zz_, yy_, xx_ = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    xs = ((3.0 + torch.sin(0.21 * zz_ + 0.13 * yy_) * torch.cos(0.17 * xx_)).float().expand(B, D, H, W) + 0.01 * torch.rand((B, D, H, W), generator=g)).contiguous()
    xsg = xs.to(DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)

    def finalize(p_, rows):
        mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
        _lib.call("tmf_bn_finalize", p_.data_ptr(), rows, C, float(B * D * H * W), gamma.data_ptr(), beta.data_ptr(), None, None, None,
                  0.1, 1e-5, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), ops._stream())
        torch.cuda.synchronize()
        return mean.cpu().double(), invstd.cpu().double()
    _lib.call("tmf_c1_stats_g", xsg.data_ptr(), wp.data_ptr(), part.data_ptr(), gram.data_ptr(), gbytes, B, D, H, W, C, ops._stream())
    m1, i1 = finalize(part, 2)
    pd = torch.empty((nblk, 2, C), device=DEV)
    _lib.call("tmf_c1_stats", xsg.data_ptr(), wp.data_ptr(), pd.data_ptr(), B, D, H, W, C, ops._stream())
    m0, i0 = finalize(pd, nblk)
    zs = F.conv3d(xs.double().unsqueeze(1), w.double(), None, 1, 1)
    mref, iref = zs.mean((0, 2, 3, 4)), (zs.var((0, 2, 3, 4), unbiased=False) + 1e-5).rsqrt()
    assert (m1 - mref).abs().max().item() <= 2e-6 * zs.abs().mean().item()
    e1, e0 = ((i1 - iref).abs() / iref).max().item(), ((i0 - iref).abs() / iref).max().item()
    assert e1 <= 2e-5 and e1 <= max(2.0 * e0, 2e-6), (e1, e0)
    _lib.call("tmf_set_option", b"c1_gram", 0)
    try:
        assert _lib.query("tmf_c1_gram_bytes", B, D, H, W, C) == 0
    finally:
        _lib.call("tmf_set_option", b"c1_gram", 1)
    # the whole block, both backward forms
    conv = torch.nn.Conv3d(1, C, 3, padding=1).to(DEV)
    bn = torch.nn.BatchNorm3d(C).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w.to(DEV))
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.2, 0.2)
    go = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g).to(DEV)
    res = {}
    for gram_opt in (1, 0, 1):
        _lib.call("tmf_set_option", b"c1_gram", gram_opt)
        try:
            for p_ in (conv.weight, bn.weight, bn.bias):
                p_.grad = None
            y = ops.conv_bn_act_pool(xg.unsqueeze(-1), conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean.clone(),
                                     bn.running_var.clone(), True, pool="max")
            y.backward(go)
            torch.cuda.synchronize()
        finally:
            _lib.call("tmf_set_option", b"c1_gram", 1)
        res.setdefault(gram_opt, []).append((y.detach().cpu(), conv.weight.grad.cpu().clone(), bn.weight.grad.cpu().clone(), bn.bias.grad.cpu().clone()))
    a, a2 = res[1]
    b = res[0][0]
    assert all(torch.equal(u, v) for u, v in zip(a, a2))
    for u, v in zip(a[1:], b[1:]):
        assert (u - v).abs().max().item() <= 2e-5 * v.abs().max().item()
    if B * D * H * W <= 40000:
        w64 = w.double().requires_grad_(True)
        g64, b64 = bn.weight.detach().double().cpu().requires_grad_(True), bn.bias.detach().double().cpu().requires_grad_(True)
        zz = F.conv3d(x.double().unsqueeze(1), w64, conv.bias.detach().double().cpu(), padding=1)
        yy = F.max_pool3d(F.leaky_relu(F.batch_norm(zz, None, None, g64, b64, True, 0.1, 1e-5), 0.01), 2)
        yy.backward(go.double().permute(0, 4, 1, 2, 3).cpu())
        e1 = (a[1].double() - w64.grad).abs().max().item() / w64.grad.abs().max().item()
        e0 = (b[1].double() - w64.grad).abs().max().item() / w64.grad.abs().max().item()
        assert e1 <= max(3.0 * e0, 5e-6), (e1, e0)
        assert (a[2].double() - g64.grad).abs().max().item() <= 5e-6 * g64.grad.abs().max().item()
