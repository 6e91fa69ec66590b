"""The persistent Winograd kernels where the work their results never needed was cut: the weight gradient
where one launch holds interior and face stages (a copy path of their own for the interior ones was measured and not kept: the
cases stay, whatever the kernel does with such stages) and where the row carry-over between the two h steps of a td meets the
prologue and the overhang behind the last stage; the split kernel's
epilogue (role coefficients, statistic cells kept in registers over an item) in MODE 0 and MODE 1.  fp64 references at the
tolerances of test_conv3d_winograd_weight_gradient / test_conv3d_winograd_split_kernel (test_gpu_kernels.py); the statistic rows
against the sums of the z the kernel itself wrote at 2e-7; every output repeats bit for bit.  Measured on an MI355X: dw 2.2 - 3.0e-7,
z and dx 2.4 - 3.5e-7, the rows 2.0e-9 - 2.7e-8 (sums) and 1.7 - 6.3e-8 (sums of squares)."""
import pytest
import torch
import torch.nn.functional as F

from _conv_util import _ncdhw, _ndhwc, _rand, _relerr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stages(shape, geom):
    """(stages, interior stages) of a weight-gradient launch: a stage is a 4x4x8 half brick of one sample (geom 0) or a 4x4x4
    brick of a sample pair (geom 1); it is interior where its halo (one voxel around it) lies inside the volume and, for geom 1,
    the pair holds two samples — every mask test of its copies passes"""
    B, D, H, W = shape[:4]
    bw, bs = (8, 1) if geom == 0 else (4, 2)
    n = inner = 0
    for b in range(0, B, bs):
        for d0 in range(0, D, 4):
            for h0 in range(0, H, 4):
                for w0 in range(0, W, bw):
                    n += 1
                    inner += (b + bs <= B and 1 <= d0 and d0 + 5 <= D and 1 <= h0 and h0 + 5 <= H and 1 <= w0 and w0 + bw + 1 <= W)
    return n, inner


WGRAD_CASES = [
    # (B, D, H, W, cin, cout), geometry, stages, interior stages
    ((1, 12, 12, 24, 32, 32), 0, 27, 1),      # exactly one interior stage among 27
    ((2, 7, 9, 13, 32, 64), 0, 24, 0),        # every stage ragged
    ((1, 4, 4, 8, 32, 32), 0, 1, 0),          # one stage: prologue and last-stage overhang of the row carry-over
    ((4, 12, 12, 12, 32, 32), 1, 54, 2),      # sample pairs, one interior brick per pair
    # three samples: pairs are no fewer stages than half bricks (54 = 54), so the planner keeps geometry 0 — 12 voxels of w hold
    # no interior half brick; two input-channel blocks
    ((3, 12, 12, 12, 64, 32), 0, 54, 0),
    ((5, 12, 12, 12, 32, 32), 1, 81, 2),      # sample pairs, the last pair holds one sample: its centre brick is no interior stage
]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_weight_gradient_interior_and_face_stages(case):
    """conv3d_wino_wgrad_p_kernel<0 | 1>: dw against the fp64 convolution gradient at 5e-6, three runs bit-equal."""
    from transmf_ad_amd import _lib, ops
    shape, geom, nst, ninner = case
    B, D, H, W, cin, cout = shape
    assert _lib.query("tmf_conv3d_wgrad_wino_kernel_name", B, D, H, W, cin, cout).decode() == "conv3d_wino_wgrad_p_kernel<%d>" % geom
    assert _stages(shape, geom) == (nst, ninner)
    x = _rand(B, cin, D, H, W, seed=371)
    dz = _rand(B, cout, D, H, W, seed=372)
    xg, dzg = _ndhwc(x).to(DEV), _ndhwc(dz).to(DEV)
    runs = [ops.conv3d_wgrad_wino(xg, dzg, cin, cout, reference_layout=True) for _ in range(3)]
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dz.double(), stride=1, padding=1)
    err = _relerr(runs[0], ref)
    print("WINOCUTS wgrad {} relerr {:.3e}".format("x".join(map(str, shape)), err))
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
    assert err < 5e-6


SPLIT_SHAPES = [
    (1, 4, 8, 8, 32, 32),           # one item
    (2, 7, 9, 13, 32, 64),          # every brick ragged: lanes outside the volume add zeros to the statistics
    (2, 12, 24, 24, 32, 64),        # 108 items, two channel groups
]


@pytest.mark.parametrize("shape", SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_split_kernel_epilogue(shape):
    """conv3d_winox_kernel<1> (z + statistic rows) and <0> (no statistics: z again, and dx with the channel roles swapped): z and
    dx against fp64 at 2e-6; the rows (NaN-prefilled: all written, zeros at and past the grid) against the per-channel sums of the
    z the kernel wrote at 2e-7; two runs bit-equal."""
    from transmf_ad_amd import _lib, ops
    B, D, H, W, cin, cout = shape
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 1) == b"conv3d_winox_kernel<1>"
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cin, cout, 0) == b"conv3d_winox_kernel<0>"
    assert _lib.query("tmf_conv3d_wino_kernel_name2", B, D, H, W, cout, cin, 0) == b"conv3d_winox_kernel<0>"
    grid = _lib.query("tmf_conv3d_wino_grid", B, D, H, W, cin, cout)
    rows = _lib.query("tmf_conv3d_wino_stat_blocks", B, D, H, W)
    assert 1 <= grid <= rows
    x = _rand(B, cin, D, H, W, seed=381)
    w = _rand(cout, cin, 3, 3, 3, seed=382, scale=(cin * 27) ** -0.5)
    dz = _rand(B, cout, D, H, W, seed=383)
    xg, dzg = _ndhwc(x).to(DEV), _ndhwc(dz).to(DEV)
    uf, ud = ops.pack_weights_wino(w.to(DEV), True, True)
    runs = []
    for _ in range(2):
        z = torch.full((B, D, H, W, cout), float("nan"), device=DEV)
        part = torch.full((rows, 2, cout), float("nan"), device=DEV)
        _lib.call("tmf_conv3d_fwd_wino", xg.data_ptr(), uf.data_ptr(), z.data_ptr(), part.data_ptr(), B, D, H, W, cin, cout, ops._stream())
        z0, _, _ = ops.conv3d_wino_raw(xg, uf, cin, cout, False)
        dx, _, _ = ops.conv3d_wino_raw(dzg, ud, cout, cin, False)
        runs.append((z, part, z0, dx))
    torch.cuda.synchronize()
    (z, part, z0, dx), second = runs
    p, zz = part.double().cpu(), z.double().cpu()
    ez = _relerr(_ncdhw(z.cpu()), F.conv3d(x.double(), w.double(), None, 1, 1))
    ex = _relerr(_ncdhw(dx.cpu()), F.conv_transpose3d(dz.double(), w.double(), None, 1, 1))
    e1 = ((p[:, 0].sum(0) - zz.sum((0, 1, 2, 3))).abs().max() / zz.abs().sum((0, 1, 2, 3)).max()).item()
    e2 = _relerr(p[:, 1].sum(0), (zz ** 2).sum((0, 1, 2, 3)))
    print("WINOCUTS split {} z {:.3e} dx {:.3e} sum {:.3e} sumsq {:.3e}".format("x".join(map(str, shape)), ez, ex, e1, e2))
    for a, b in zip(runs[0], second):
        assert torch.equal(a, b)
    assert torch.equal(z, z0)                                                  # the instance without statistics: the same z
    assert ez < 2e-6 and ex < 2e-6
    assert bool(torch.isfinite(p).all()) and bool((p[grid:] == 0).all())
    assert e1 <= 2e-7 and e2 < 2e-7
