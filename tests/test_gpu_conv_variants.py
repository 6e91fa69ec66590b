"""Every direct fp32 convolution kernel the planners can select (MI355X): the rows of tests/_conv_variants.py, each under its
conv_waves, against fp64 torch on the host — forward with the BatchNorm statistic partials, data gradient, weight gradient
and the fused eval epilogue (tmf_conv3d_fwd_affine, called directly so that conv_wino cannot reroute it) — plus exact integer
probes, run-to-run equality and write bounds.  Tolerances are those of tests/test_gpu_kernels.py for the same operations
(test_conv3d_fwd_and_stats, test_conv3d_wgrad_and_dgrad, test_eval_block_single_pass; K = 27 cin <= 1080 here against up to
3456 there).  Each case prints the errors it saw ("CONVVAR <row> <quantity> <error>")."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _conv_variants as V
from _conv_util import _lib, _ncdhw, _ndhwc, _ops, _rand, _relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = float(np.float32(0.01))
POOLS = (None, "max", "avg")


def _say(row, what, value):
    print("CONVVAR {} {} {:.3e}".format(V.row_id(row), what, value))


def _names(shape):
    B, D, H, W, cin, cout, k = shape
    q = _lib().query
    return (q("tmf_conv3d_fwd_kernel_name", B, D, H, W, cin, cout, k).decode(),
            q("tmf_conv3d_fwd_kernel_name", B, D, H, W, cout, cin, k).decode(),
            q("tmf_conv3d_wgrad_kernel_name", B, D, H, W, cin, cout, k).decode() if k == 3 else None)


@pytest.fixture
def row(request):
    """The row under its conv_waves (16 again afterwards); the library must select the row's kernels there, so that a row
    cannot silently run another kernel."""
    r = request.param
    _lib().call("tmf_set_option", b"conv_waves", r[0])
    try:
        assert _names(r[1]) == (r[2], r[3], r[4])
        yield r
    finally:
        _lib().call("tmf_set_option", b"conv_waves", 16)


def _rows(keep=lambda r: True):
    return pytest.mark.parametrize("row", [r for r in V.ROWS if keep(r)], ids=V.row_id, indirect=True)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Seeded inputs and the fp64 results of a (B, D, H, W, cin, cout, k), computed once and shared (read only) by the rows
    and tests of that shape."""
    B, D, H, W, cin, cout, k = shape
    x = _rand(B, cin, D, H, W, seed=1)
    w = _rand(cout, cin, k, k, k, seed=2, scale=(cin * k ** 3) ** -0.5)
    dz = _rand(B, cout, D, H, W, seed=5)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    z = F.conv3d(xr, wr, padding=k // 2)
    z.backward(dz.double())
    return dict(x=x, w=w, dz=dz, z=z.detach(), dx=xr.grad, dw=wr.grad,
                scale=_rand(cout, seed=6), shift=_rand(cout, seed=8, scale=0.5))


@functools.lru_cache(maxsize=None)
def _fused_ref(shape, pool):
    c = _case(shape)
    y = F.leaky_relu(c["z"] * c["scale"].double().view(1, -1, 1, 1, 1) + c["shift"].double().view(1, -1, 1, 1, 1), SLOPE)
    return y if pool is None else (F.max_pool3d(y, 2, 2) if pool == "max" else F.avg_pool3d(y, 2, 2))


def _fused(xg, wp, sc, sh, shape, pool, out=None):
    """tmf_conv3d_fwd_affine on its own (ops.conv_bn_act_pool would send most of these to the Winograd kernels)."""
    lib = _lib()
    B, D, H, W, cin, cout, k = shape
    oshape = (B, D, H, W, cout) if pool is None else (B, D // 2, H // 2, W // 2, cout)
    if out is None:
        out = torch.full(oshape, float("nan"), device=DEV)           # an element the kernel leaves out fails the comparison
    lib.call("tmf_conv3d_fwd_affine", xg.data_ptr(), wp.data_ptr(), sc.data_ptr(), sh.data_ptr(), out.data_ptr(),
             B, D, H, W, cin, cout, k, lib.pool_code(pool), SLOPE, torch.cuda.current_stream().cuda_stream)
    return out.view(oshape) if out.dim() == 1 else out


# ---------------------------------------------------------------------------------------------------------------------
# every row against fp64
# ---------------------------------------------------------------------------------------------------------------------
@_rows()
def test_forward_and_statistic_partials(row):
    ops, lib = _ops(), _lib()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    ref = c["z"]
    xg, wp = _ndhwc(c["x"]).to(DEV), ops.pack_weight(c["w"].to(DEV))
    z, part, nblk = ops.conv3d_raw(xg, wp, cin, cout, k, True)
    torch.cuda.synchronize()
    assert nblk == lib.query("tmf_conv3d_stat_blocks", B, D, H, W, cin, cout, k) and tuple(part.shape) == (nblk, 2, cout)
    e = _relerr(_ncdhw(z.cpu()), ref)
    _say(row, "fwd", e)
    s = part.double().sum(0).cpu()
    r = ref.permute(1, 0, 2, 3, 4).reshape(cout, -1)
    e1 = (s[0] - r.sum(1)).abs().max().item() / max(1.0, r.abs().sum(1).max().item())
    e2 = (s[1] - (r * r).sum(1)).abs().max().item() / (r * r).sum(1).max().item()
    _say(row, "stat_sum", e1)
    _say(row, "stat_sumsq", e2)
    # the statistic partials are those of the z the kernel stored
    zc = z.double().reshape(-1, cout).cpu()
    e3 = (s[0] - zc.sum(0)).abs().max().item() / max(1.0, zc.abs().sum(0).max().item())
    e4 = (s[1] - (zc * zc).sum(0)).abs().max().item() / (zc * zc).sum(0).max().item()
    _say(row, "stat_sum_of_z", e3)
    _say(row, "stat_sumsq_of_z", e4)
    assert e < 1e-5
    assert e1 <= 1e-4 and e2 <= 1e-5
    assert e3 <= 1e-4 and e4 <= 1e-5
    z2, part2, _ = ops.conv3d_raw(xg, wp, cin, cout, k, True)
    assert torch.equal(z2, z) and torch.equal(part2, part)
    # without statistics: the same z
    z3, _, _ = ops.conv3d_raw(xg, wp, cin, cout, k, False)
    assert torch.equal(z3, z)


@_rows()
def test_data_gradient(row):
    """The same kernel family with the flipped, transposed weights (pack_weight_dgrad): the row's data-gradient kernel."""
    ops = _ops()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    dzg, wd = _ndhwc(c["dz"]).to(DEV), ops.pack_weight_dgrad(c["w"].to(DEV))
    dx, _, _ = ops.conv3d_raw(dzg, wd, cout, cin, k, False)
    e = _relerr(_ncdhw(dx.cpu()), c["dx"])
    _say(row, "dgrad", e)
    assert e < 1e-5
    dx2, _, _ = ops.conv3d_raw(dzg, wd, cout, cin, k, False)
    assert torch.equal(dx2, dx)


@_rows(lambda r: r[1][6] == 3)
def test_weight_gradient(row):
    ops = _ops()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    xg, dzg = _ndhwc(c["x"]).to(DEV), _ndhwc(c["dz"]).to(DEV)
    dw = ops.unpack_wgrad(ops.conv3d_wgrad(xg, dzg, cin, cout, k), cout, cin, k)
    e = _relerr(dw, c["dw"])
    _say(row, "wgrad", e)
    assert e < 5e-6
    # the final reduction stores the nn.Conv3d layout itself: bit-identical values
    assert torch.equal(ops.conv3d_wgrad(xg, dzg, cin, cout, k, reference_layout=True), dw)
    assert torch.equal(ops.unpack_wgrad(ops.conv3d_wgrad(xg, dzg, cin, cout, k), cout, cin, k), dw)


@_rows(V.takes_fused)
def test_fused_eval_epilogue(row):
    """pool(leaky_relu(scale conv + shift)) in one kernel, scale of both signs, without pool, with max and with average pool:
    the three pooled branches of the epilogue (tests/test_host_conv_variants.py holds the rows to all three)."""
    ops = _ops()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    assert (c["scale"] > 0).any() and (c["scale"] < 0).any()
    xg, wp = _ndhwc(c["x"]).to(DEV), ops.pack_weight(c["w"].to(DEV))
    sc, sh = c["scale"].to(DEV), c["shift"].to(DEV)
    for pool in POOLS:
        ref = _fused_ref(shape, pool)
        y = _fused(xg, wp, sc, sh, shape, pool)
        torch.cuda.synchronize()
        assert tuple(y.shape) == tuple(_ndhwc(ref).shape)
        e = _relerr(_ncdhw(y.cpu()), ref)
        _say(row, "fused_{}_{}".format(pool or "none", V.pool_branch(row[2])), e)
        assert e < 2e-5, pool
        assert torch.equal(_fused(xg, wp, sc, sh, shape, pool), y), pool


def _int_conv(cin, cout, k, vol, dense):
    """Small-integer x and asymmetric integer (and 1/2) weights: every product and every sum is exact in fp32 in any order
    (|sum| <= 27 * 192 * 4 < 2^24), so the fp64 result on the host IS the fp32 result.  dense = False is the probe of
    test_mfma_layout_is_transpose_sensitive (one lit voxel), dense = True fills the volume, every tap and every channel."""
    B, D, H, W = vol
    if dense:
        g = torch.Generator().manual_seed(100 * cin + cout + k)
        x = torch.randint(-2, 3, (B, cin, D, H, W), generator=g).float()
        w = torch.randint(-2, 3, (cout, cin, k, k, k), generator=g).float()
    else:
        x = torch.zeros(B, cin, D, H, W)
        x[0, :, 3, 4, 5] = torch.arange(cin, dtype=torch.float32) + 1
        x[B - 1, :, D - 1, H - 1, W - 1] = torch.arange(cin, dtype=torch.float32) - 3          # in the last, overhanging brick
        w = torch.zeros(cout, cin, k, k, k)
        co, ci = torch.arange(cout).view(-1, 1), torch.arange(cin).view(1, -1)
        w[:, :, k // 2, k // 2, k // 2] = ((co * 37 + ci * 11) % 23 - 7).float()
        if k == 3:
            w[:, :, 0, 1, 2] = 0.5
    return x, w, F.conv3d(x.double(), w.double(), padding=k // 2).float()


@_rows()
def test_exact_on_small_integers(row):
    """Swapped rows or columns of an MT = 2 or 8-wave fragment, a voxel or a tap in the wrong place: not a rounding error.  The
    row's forward kernel, and its data-gradient kernel run as the forward convolution cout -> cin."""
    ops = _ops()
    B, D, H, W, cin, cout, k = row[1]
    for a, b in ((cin, cout), (cout, cin)):
        for dense in (False, True):
            x, w, ref = _int_conv(a, b, k, (B, D, H, W), dense)
            z, _, _ = ops.conv3d_raw(_ndhwc(x).to(DEV), ops.pack_weight(w.to(DEV)), a, b, k, False)
            assert torch.equal(_ncdhw(z.cpu()), ref), (a, b, dense)


# ---------------------------------------------------------------------------------------------------------------------
# writes stay inside the outputs, reads inside the inputs: one row per brick geometry and per weight-gradient kernel
# ---------------------------------------------------------------------------------------------------------------------
SENT, PAD = 12345.0, 1 << 14


def _sentinel(n):
    return torch.full((n + 2 * PAD,), SENT, device=DEV)


def _bands_intact(big, n):
    return bool((big[:PAD] == SENT).all()) and bool((big[PAD + n:] == SENT).all())


def _all_written(big, n):
    return int((big[PAD:PAD + n] == SENT).sum()) == 0


def _guarded(t, fill, pad=4096):
    big = torch.full((t.numel() + 2 * pad,), fill, device=t.device, dtype=t.dtype)
    v = big[pad:pad + t.numel()].view(t.shape)
    v.copy_(t)
    return v, big


@pytest.mark.parametrize("row", V.guard_rows(), ids=V.row_id, indirect=True)
def test_kernels_write_only_their_outputs(row):
    ops, lib = _ops(), _lib()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    st = torch.cuda.current_stream().cuda_stream
    xg, dzg, wp = _ndhwc(c["x"]).to(DEV), _ndhwc(c["dz"]).to(DEV), ops.pack_weight(c["w"].to(DEV))
    # z and the statistic partials
    nz, nblk = B * D * H * W * cout, lib.query("tmf_conv3d_stat_blocks", B, D, H, W, cin, cout, k)
    zbig, pbig = _sentinel(nz), _sentinel(nblk * 2 * cout)
    lib.call("tmf_conv3d_fwd", xg.data_ptr(), wp.data_ptr(), zbig[PAD:].data_ptr(), pbig[PAD:].data_ptr(), B, D, H, W, cin, cout, k, st)
    torch.cuda.synchronize()
    assert _bands_intact(zbig, nz) and _all_written(zbig, nz)
    assert _bands_intact(pbig, nblk * 2 * cout) and _all_written(pbig, nblk * 2 * cout)
    # the data gradient's kernel: dx
    nx = B * D * H * W * cin
    xbig = _sentinel(nx)
    lib.call("tmf_conv3d_fwd", dzg.data_ptr(), ops.pack_weight_dgrad(c["w"].to(DEV)).data_ptr(), xbig[PAD:].data_ptr(), None,
             B, D, H, W, cout, cin, k, st)
    torch.cuda.synchronize()
    assert _bands_intact(xbig, nx) and _all_written(xbig, nx)
    # the fused epilogue's (pooled) output
    if V.takes_fused(row):
        sc, sh = c["scale"].to(DEV), c["shift"].to(DEV)
        for pool in POOLS:
            ny = nz if pool is None else B * (D // 2) * (H // 2) * (W // 2) * cout
            ybig = _sentinel(ny)
            _fused(xg, wp, sc, sh, shape, pool, out=ybig[PAD:PAD + ny])
            torch.cuda.synchronize()
            assert _bands_intact(ybig, ny) and _all_written(ybig, ny), pool
    # dw (both layouts) and the workspace
    nbytes = lib.query("tmf_conv3d_wgrad_workspace_bytes", B, D, H, W, cin, cout, k)
    nws, ndw = max(nbytes, 16) // 4, 27 * cin * cout
    for layout in (0, 1):
        wbig, dbig = _sentinel(nws), _sentinel(ndw)
        lib.call("tmf_conv3d_wgrad", xg.data_ptr(), dzg.data_ptr(), dbig[PAD:].data_ptr(), wbig[PAD:].data_ptr(), nbytes,
                 B, D, H, W, cin, cout, k, layout, st)
        torch.cuda.synchronize()
        assert _bands_intact(wbig, nws) and _bands_intact(dbig, ndw) and _all_written(dbig, ndw), layout


@pytest.mark.parametrize("row", V.guard_rows(), ids=V.row_id, indirect=True)
def test_kernels_ignore_memory_around_their_inputs(row):
    """x, w and dz between NaN-filled guards give bitwise what they give between zero-filled ones."""
    ops = _ops()
    B, D, H, W, cin, cout, k = shape = row[1]
    c = _case(shape)
    x0, dz0 = _ndhwc(c["x"]).to(DEV), _ndhwc(c["dz"]).to(DEV)
    wp0, wd0 = ops.pack_weight(c["w"].to(DEV)), ops.pack_weight_dgrad(c["w"].to(DEV))
    sc0, sh0 = c["scale"].to(DEV), c["shift"].to(DEV)
    res = []
    for fill in (0.0, float("nan")):
        (xg, _k1), (dg, _k2), (wg, _k3), (wdg, _k4) = (_guarded(t, fill) for t in (x0, dz0, wp0, wd0))
        (sc, _k5), (sh, _k6) = _guarded(sc0, fill), _guarded(sh0, fill)
        z, part, _ = ops.conv3d_raw(xg, wg, cin, cout, k, True)
        dx, _, _ = ops.conv3d_raw(dg, wdg, cout, cin, k, False)
        out = [z, part, dx, ops.conv3d_wgrad(xg, dg, cin, cout, k)]
        if V.takes_fused(row):
            out += [_fused(xg, wg, sc, sh, shape, pool) for pool in POOLS]
        torch.cuda.synchronize()
        res.append([t.clone() for t in out])
    for a, b in zip(*res):
        assert torch.isfinite(b).all()
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# the fused epilogue lives in the ring kernel only
# ---------------------------------------------------------------------------------------------------------------------
def test_fused_epilogue_never_takes_the_register_tiled_kernel():
    """conv_rt 2 sends this shape's plain forward to the register-tiled kernel (6x6x12 bricks tile it); tmf_conv3d_fwd_affine
    must plan without it (plan_fwd(..., allow_rt = false)) and give bitwise what it gives at conv_rt 0."""
    ops, lib = _ops(), _lib()
    shape = (1, 12, 12, 12, 16, 32, 3)
    B, D, H, W, cin, cout, k = shape
    c = _case(shape)
    xg, wp = _ndhwc(c["x"]).to(DEV), ops.pack_weight(c["w"].to(DEV))
    sc, sh = c["scale"].to(DEV), c["shift"].to(DEV)
    try:
        assert not lib.query("tmf_conv3d_fwd_kernel_name", B, D, H, W, cin, cout, k).decode().startswith("RtCfg")
        y0 = [_fused(xg, wp, sc, sh, shape, pool) for pool in POOLS]
        lib.call("tmf_set_option", b"conv_rt", 2)
        assert lib.query("tmf_conv3d_fwd_kernel_name", B, D, H, W, cin, cout, k).decode().startswith("RtCfg")
        y2 = [_fused(xg, wp, sc, sh, shape, pool) for pool in POOLS]
        torch.cuda.synchronize()
    finally:
        lib.call("tmf_set_option", b"conv_rt", 0)
    for pool, a, b in zip(POOLS, y0, y2):
        assert torch.equal(a, b), pool
        assert _relerr(_ncdhw(b.cpu()), _fused_ref(shape, pool)) < 2e-5, pool
