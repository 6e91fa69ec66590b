"""The persistent Winograd kernels at grids that are NO multiple of 8 (where their XCD placement used to be switched off) against
fp64 torch: forward with statistic partials, data gradient, weight gradient, run-to-run bits.  Tolerances: those of
test_conv3d_winograd_split_kernel / test_conv3d_winograd_weight_gradient (test_gpu_kernels.py)."""
import pytest
import torch
import torch.nn.functional as F

from _conv_util import _ncdhw, _ndhwc, _rand, _relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


# (B, D, H, W, cin, cout), items of the split kernel's forward launch, its grid on 256 compute units
PLACEMENT_SHAPES = [
    ((2, 12, 40, 40, 32, 96), 450, 225),      # 2 rounds, 3 channel groups: 225 % 8 = 1, a workgroup changes group between its items
    ((1, 8, 24, 40, 32, 32), 30, 30),         # fewer items than compute units: 30 % 8 = 6
    ((2, 22, 27, 22, 64, 64), 252, 252),      # transposed items (4 voxels along h): 252 % 8 = 4
]
_INPUTS = {}


def _inputs(shape):
    """inputs and fp64 references of a shape, computed once and shared by its two cases"""
    if shape not in _INPUTS:
        from transmf_ad_amd import ops
        B, D, H, W, cin, cout = shape
        x = _rand(B, cin, D, H, W, seed=351)
        w = _rand(cout, cin, 3, 3, 3, seed=352, scale=(cin * 27) ** -0.5)
        dz = _rand(B, cout, D, H, W, seed=353)
        uf, ud = ops.pack_weights_wino(w.to(DEV), True, True)
        _INPUTS[shape] = dict(xg=_ndhwc(x).to(DEV), dzg=_ndhwc(dz).to(DEV), uf=uf, ud=ud,
                              z=F.conv3d(x.double(), w.double(), None, 1, 1),
                              dx=F.conv_transpose3d(dz.double(), w.double(), None, 1, 1))
    return _INPUTS[shape]


@pytest.mark.parametrize("xmode", [1, 0], ids=["split", "fp32"])
@pytest.mark.parametrize("case", PLACEMENT_SHAPES, ids=lambda c: "x".join(map(str, c[0])))
def test_winograd_forward_and_dgrad_at_grids_off_the_multiples_of_8(case, xmode):
    """conv3d_winox_kernel<1 | 0> and, with "wino_x" 0, conv3d_wino_p_kernel<1 | 0, 0>: z and dx against fp64 conv3d, the
    statistic rows (NaN-prefilled: every row written, zeros at and past the launch's grid) against the fp64 sums of z and z^2,
    two runs bit-equal.  The shapes put the split kernel's grids off the multiples of 8 on a 256-CU device (asserted there)."""
    from transmf_ad_amd import _lib, ops
    shape, items, grid256 = case
    B, D, H, W, cin, cout = shape
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.call("tmf_set_option", b"wino_x", xmode)
    try:
        name = _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1).decode()
        assert name == ("conv3d_winox_kernel<1>" if xmode else "conv3d_wino_p_kernel<1, 0>")
        grid = _lib.query("tmf_conv3d_wino_grid", B, D, H, W, cin, cout)
        rows = _lib.query("tmf_conv3d_wino_stat_blocks", B, D, H, W)
        assert rows == ncu and 1 <= grid <= ncu
        if xmode:
            assert _lib.query("tmf_conv3d_wino_bricks2", B, D, H, W, cin, cout) * (cout // 32) == items
            if ncu == 256:
                assert grid == grid256 and grid % 8 != 0
        g = _inputs(shape)
        runs = []
        for _ in range(2):
            z = torch.full((B, D, H, W, cout), float("nan"), device=DEV)
            part = torch.full((rows, 2, cout), float("nan"), device=DEV)
            _lib.call("tmf_conv3d_fwd_wino", g["xg"].data_ptr(), g["uf"].data_ptr(), z.data_ptr(), part.data_ptr(),
                      B, D, H, W, cin, cout, ops._stream())
            dx, _, _ = ops.conv3d_wino_raw(g["dzg"], g["ud"], cout, cin, False)
            runs.append((z, part, dx))
        torch.cuda.synchronize()
    finally:
        _lib.call("tmf_set_option", b"wino_x", 1)
    (z, part, dx), (z2, part2, dx2) = runs
    assert torch.equal(z, z2) and torch.equal(part, part2) and torch.equal(dx, dx2)
    assert _relerr(_ncdhw(z.cpu()), g["z"]) < 2e-6
    assert _relerr(_ncdhw(dx.cpu()), g["dx"]) < 2e-6
    p = part.double().cpu()
    assert bool(torch.isfinite(p).all()) and bool((p[grid:] == 0).all())
    zz = z.double().cpu()
    assert (p[:, 0].sum(0) - zz.sum((0, 1, 2, 3))).abs().max().item() <= 2e-6 * zz.abs().sum((0, 1, 2, 3)).max().item()
    assert _relerr(p[:, 1].sum(0), (zz ** 2).sum((0, 1, 2, 3))) < 2e-6


@pytest.mark.parametrize("shape", [(2, 12, 40, 40, 32, 96),        # 300 stages in 75 splits of 4, three channel blocks: 75 % 8 = 3
                                   (8, 12, 12, 12, 128, 256)],     # conv4.0: stages of two samples x 4x4x4 voxels
                         ids=lambda s: "x".join(map(str, s)))
def test_winograd_weight_gradient_with_placed_splits(shape):
    """conv3d_wino_wgrad_p_kernel<0 | 1> walks split xcd_slot(blockIdx.x) and writes that split's slab: dw against fp64 torch
    and against the kernels of "wino_p" 0, which place nothing (another kernel family: the same sums, other rounding), at the
    tolerance of test_conv3d_winograd_weight_gradient; two runs bit-equal."""
    from transmf_ad_amd import _lib, ops
    B, D, H, W, cin, cout = shape
    kernel = _lib.query("tmf_conv3d_wgrad_wino_kernel_name", B, D, H, W, cin, cout).decode()
    assert kernel == ("conv3d_wino_wgrad_p_kernel<1>" if D == 12 and H == 12 else "conv3d_wino_wgrad_p_kernel<0>")
    x = _rand(B, cin, D, H, W, seed=361)
    dz = _rand(B, cout, D, H, W, seed=362)
    xg, dzg = _ndhwc(x).to(DEV), _ndhwc(dz).to(DEV)
    dw = ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True)
    assert torch.equal(dw, ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True))
    _lib.call("tmf_set_option", b"wino_p", 0)
    try:
        d0 = ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True)
    finally:
        _lib.call("tmf_set_option", b"wino_p", 1)
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dz.double(), stride=1, padding=1)
    assert _relerr(dw, ref) < 5e-6 and _relerr(d0, ref) < 5e-6
    assert _relerr(dw, d0.cpu()) < 5e-6
