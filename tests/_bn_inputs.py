"""Inputs and references of the BatchNorm + LeakyReLU + pool, finalize and slab-reduction tests
(tests/test_host_bn_reduce.py, tests/test_gpu_bn_reduce.py).

Every reference is plain torch on the host and takes z, dout, scale, shift, mean, invstd and coef as free inputs, the way
the kernels do: a test can feed values no convolution would produce.  `dtype` is torch.float64 for the reference itself and
torch.float32 for its restatement, the yardstick the conditioning family measures its tolerance with.

Tensors are channels-last (B, D, H, W, C) as in the library; pool codes are the library's (0 none, 1 max, 2 average)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

POOL_NONE, POOL_MAX, POOL_AVG = 0, 1, 2
POOLS = (POOL_NONE, POOL_MAX, POOL_AVG)
IO_MODES = (0, 1, 3)                    # bit 0: z / dz are bf16 tensors, bit 1: out / dout are bf16 tensors
U32 = 2.0 ** -24


def f32(v):
    """The double a C float argument holds (slope, eps, momentum travel as floats)."""
    return float(np.float32(v))


def z_dtype(io):
    return torch.bfloat16 if io & 1 else torch.float32


def y_dtype(io):
    return torch.bfloat16 if io & 2 else torch.float32


def pooled_shape(shape, pool):
    B, D, H, W = shape
    return (B, D, H, W) if pool == POOL_NONE else (B, D // 2, H // 2, W // 2)


def windows(t):
    """(B, D, H, W, C) -> (B, D/2, H/2, W/2, C, 8): the full 2x2x2 windows, k = 4 d + 2 h + w (floor mode)."""
    B, D, H, W, C = t.shape
    t = t[:, :D // 2 * 2, :H // 2 * 2, :W // 2 * 2]
    t = t.reshape(B, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return t.reshape(B, D // 2, H // 2, W // 2, C, 8)


def first_max(y):
    """(index, several equal maxima) of the first maximum over the last axis (8 window voxels in torch's scan order)."""
    hit = y == y.max(-1, keepdim=True).values
    return hit.float().argmax(-1), hit.sum(-1) > 1           # argmax: the first of equal values


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def _ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def _pool(a, pool):
    """a (B, C, D, H, W); an empty pooled output (an axis of length 1) is an empty tensor, not an error."""
    if pool == POOL_NONE:
        return a
    B, C, D, H, W = a.shape
    if 0 in (D // 2, H // 2, W // 2):
        return a[:, :, :D // 2 * 2:2, :H // 2 * 2:2, :W // 2 * 2:2] * 0
    return F.max_pool3d(a, 2, 2) if pool == POOL_MAX else F.avg_pool3d(a, 2, 2)


def forward_ref(z, scale, shift, slope, pool, dtype=torch.float64):
    """pool(leaky_relu(z * scale + shift, slope)), floor mode -> (B, D', H', W', C)."""
    y = _ncdhw(z.to(dtype)) * scale.to(dtype).view(1, -1, 1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1, 1)
    return _pool(F.leaky_relu(y, slope), pool).permute(0, 2, 3, 4, 1).contiguous()


def dy_ref(z, dout, scale, shift, slope, pool, dtype=torch.float64):
    """Autograd of forward_ref with respect to y = z * scale + shift (max pool: torch's first-maximum routing)."""
    y = (_ncdhw(z.to(dtype)) * scale.to(dtype).view(1, -1, 1, 1, 1) + shift.to(dtype).view(1, -1, 1, 1, 1)).detach()
    y.requires_grad_(True)
    out = _pool(F.leaky_relu(y, slope), pool)
    if out.numel() == 0:
        return torch.zeros(z.shape, dtype=dtype)
    out.backward(_ncdhw(dout.to(dtype)))
    return y.grad.permute(0, 2, 3, 4, 1).contiguous()


def _sum_voxels(t):
    """Sum over all axes but the last.  Below fp64 as a fixed pairwise tree of elementwise additions (halves added onto each
    other), so that the restatement does not depend on how a library sum splits its work over threads and vector lanes."""
    t = t.reshape(-1, t.shape[-1])
    if t.dtype == torch.float64:
        return t.sum(0)
    while t.shape[0] > 1:
        h = t.shape[0] // 2
        t = torch.cat([t[:h] + t[h:2 * h], t[2 * h:]])
    return t[0]


def sums_ref(z, dy, mean, invstd, dtype=torch.float64):
    """(S1, S2)[c] = (sum dy, sum dy * (z - mean) * invstd) over ALL voxels, border voxels included."""
    xhat = (z.to(dtype) - mean.to(dtype)) * invstd.to(dtype)
    dy = dy.to(dtype)
    return _sum_voxels(dy), _sum_voxels(dy * xhat)


def dz_ref(z, dy, scale, mean, invstd, coef, dtype=torch.float64):
    """scale * (dy - coef0 - xhat * coef1) for every voxel; coef (2, C)."""
    xhat = (z.to(dtype) - mean.to(dtype)) * invstd.to(dtype)
    coef = coef.to(dtype)
    return scale.to(dtype) * (dy.to(dtype) - coef[0] - xhat * coef[1])


def dz_ref_folded(z, dy, scale, mean, invstd, coef, dtype=torch.float64):
    """The same value in the form the 8-wide max-pool apply pass uses: z * K1 + K0 + scale * dy."""
    scale, mean, invstd, coef = (t.to(dtype) for t in (scale, mean, invstd, coef))
    K1 = -scale * coef[1] * invstd
    K0 = scale * (coef[1] * mean * invstd - coef[0])
    return z.to(dtype) * K1 + K0 + scale * dy.to(dtype)


def bn_finalize_ref(part, count, gamma, beta, conv_bias, rmean, rvar, momentum, eps):
    """The closing formulas of tmf_bn_finalize in fp64 on the fp32 partials part (nblk, 2, C).  -> dict of fp64 tensors; `terms`
    holds sum |terms| of the closing expression of shift and of the running buffers (the scale of their tolerance)."""
    s = part.double().sum(0)
    m = s[0] / count
    var = (s[1] / count - m * m).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + f32(eps))
    g, b = gamma.double(), beta.double()
    scale = g * invstd
    r = dict(mean=m, var=var, invstd=invstd, scale=scale, shift=b - m * scale, terms={})
    r["terms"]["shift"] = b.abs() + (m * scale).abs()
    mom = f32(momentum)
    if rmean is not None:
        mb = m + (conv_bias.double() if conv_bias is not None else 0.0)
        r["running_mean"] = (1.0 - mom) * rmean.double() + mom * mb
        r["terms"]["running_mean"] = ((1.0 - mom) * rmean.double()).abs() + abs(mom) * (
            m.abs() + (conv_bias.double().abs() if conv_bias is not None else 0.0))
    if rvar is not None:
        unb = var * count / (count - 1.0) if count > 1 else var
        r["running_var"] = (1.0 - mom) * rvar.double() + mom * unb
        r["terms"]["running_var"] = ((1.0 - mom) * rvar.double()).abs() + abs(mom) * unb.abs()
    return r


def bn_bwd_finalize_ref(part, count):
    """(dgamma, dbeta, coef (2, C)) of tmf_bn_bwd_finalize in fp64: dbeta = S1, dgamma = S2, coef = S / count."""
    s = part.double().sum(0)
    return s[1], s[0], s / count


def bn_eval_coeffs_ref(gamma, beta, conv_bias, rmean, rvar, eps):
    """(scale, shift, sum |terms| of shift) of tmf_bn_eval_coeffs in fp64."""
    scale = gamma.double() / torch.sqrt(rvar.double() + f32(eps))
    bias = conv_bias.double() if conv_bias is not None else torch.zeros_like(scale)
    return scale, beta.double() + (bias - rmean.double()) * scale, beta.double().abs() + (bias.abs() + rmean.double().abs()) * scale.abs()


def ulp_at(mag, dtype):
    """One unit in the last place of `dtype` (float32 / bfloat16) at magnitude `mag` (an fp64 tensor); 0 where mag is 0."""
    p = 24 if dtype == torch.float32 else 8
    _, e = torch.frexp(mag.double().abs())                      # |mag| = m 2^e, m in [0.5, 1)
    return torch.where(mag == 0, torch.zeros_like(mag, dtype=torch.float64), torch.ldexp(torch.ones_like(mag, dtype=torch.float64), e - p))


def per_channel_distance(got, ref, top=None):
    """max over channels of (max |got - ref| of the channel / `top` of the channel); the channel is the last axis and `top` is
    the channel's own max |ref| unless given."""
    got, ref = got.double().reshape(-1, ref.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    if ref.shape[0] == 0:
        return 0.0
    top = ref.abs().max(0).values if top is None else top.double().reshape(-1)
    err = (got - ref).abs().max(0).values
    return float(torch.where(top > 0, err / top, err).max())


# ---------------------------------------------------------------------------------------------------------------------
# A. exact-arithmetic family
# ---------------------------------------------------------------------------------------------------------------------
# Dyadic grids on which every product and every sum below is exact in fp32 under any order of additions and with or
# without FMA contraction (tests/test_host_bn_reduce.py proves the budget in integers):
#   z multiples of 1/2 in [-2, 2] - scale +-0.5, +-1, +-2 (0 for one channel) - shift k/8 + 1/16, |shift| < 1.1, so that
#   y = z scale + shift is an odd multiple of 1/16 (never 0, |y| <= 5 + 1/16) - mean multiples of 1/2 in [-1, 1] -
#   invstd 1 or 2 - coef multiples of 1/4 in [-2, 2] - dout integers in [-2, 2] - slope 1/4.
EXACT_SLOPE = 0.25
EXACT_SHAPES = [(2, 5, 7, 6), (1, 1, 4, 4), (1, 2, 2, 2), (3, 8, 6, 10)]
EXACT_CHANNELS = [1, 6, 12, 20, 64, 255, 256, 1024]
# more rows / windows than the 2048-workgroup cap of the elementwise plan (rows of one lane-row each at C = 1024)
EXACT_GRID_STRIDE = [((1, 14, 14, 14), 1024, POOL_NONE), ((2, 22, 20, 22), 1024, POOL_MAX)]


def exact_inputs(shape, C, pool, seed=0):
    """dict(z, dout, scale, shift, mean, invstd, coef) of float32 tensors on the grids above.  The rows h < hcut of z (two
    thirds of H, whole windows) are constant per channel, so every window there has eight equal maxima; elsewhere nine values
    over eight voxels tie often enough."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed + 7919 * C + 131 * D + 17 * H + W + 3 * pool)
    z = torch.randint(-4, 5, (B, D, H, W, C), generator=g).float() / 2
    hcut = max(2, (2 * H // 3) // 2 * 2)
    z[:, :, :hcut] = (torch.randint(-4, 5, (C,), generator=g).float() / 2).view(1, 1, 1, 1, C)
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 6, (C,), generator=g)]
    if C > 1:
        scale[min(C - 1, 3)] = 0.0
    shift = torch.randint(-8, 8, (C,), generator=g).float() / 8 + 1.0 / 16
    mean = torch.randint(-2, 3, (C,), generator=g).float() / 2
    invstd = torch.randint(1, 3, (C,), generator=g).float()
    coef = torch.randint(-8, 9, (2, C), generator=g).float() / 4
    dout = torch.randint(-2, 3, pooled_shape(shape, pool) + (C,), generator=g).float()
    return dict(z=z, dout=dout, scale=scale, shift=shift, mean=mean, invstd=invstd, coef=coef)


def tie_share(z, scale, shift):
    """Share of the full windows (per channel) whose maximum of y = z scale + shift is attained more than once."""
    if 0 in windows(z).shape:
        return 1.0
    y = windows(z.double()) * scale.double().view(1, 1, 1, 1, -1, 1) + shift.double().view(1, 1, 1, 1, -1, 1)
    return float(first_max(y)[1].float().mean())


# ---------------------------------------------------------------------------------------------------------------------
# B. conditioning family
# ---------------------------------------------------------------------------------------------------------------------
COND_SLOPE = 0.01
COND_EPS = 1e-5
COND_SHAPES = [(2, 9, 11, 10), (2, 22, 20, 22)]
COND_CASES = [(C, io, shape, pool) for (C, ios) in ((12, (0,)), (64, (0, 3))) for io in ios for shape in COND_SHAPES for pool in POOLS]
COND_RATIOS = (0.0, 3.0, 30.0)            # |mean| / sd of a channel, mixed inside one tensor
COND_AMBIGUOUS = 1e-5                     # of the channel's sd of y: a smaller gap / |y| makes the fp64 reference itself ambiguous
COND_MAX_EXCLUDED = 0.01


def cond_inputs(C, io, shape, pool, seed=0):
    """z = m_c + s_c randn with m_c / s_c from COND_RATIOS (signs mixed), gamma of both signs; mean, invstd, scale, shift are
    the fp64 batch statistics of that z (after its rounding to the tensor type) rounded to fp32; dout is random, and zero where
    the routing / the LeakyReLU branch of the reference is ambiguous.  -> (dict as exact_inputs, excluded share)."""
    B, D, H, W = shape
    g = torch.Generator().manual_seed(seed + 1000 * C + 100 * io + 10 * D + pool)
    sd = 0.5 + torch.rand(C, generator=g)
    ratio = torch.tensor(COND_RATIOS)[torch.arange(C) % 3]
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    z = (sign * ratio * sd + sd * torch.randn((B, D, H, W, C), generator=g)).to(z_dtype(io)).float()
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 4 < 2, 1.0, -1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    zd = z.double()
    m = zd.mean((0, 1, 2, 3))
    var = (zd * zd).mean((0, 1, 2, 3)) - m * m
    invstd = 1.0 / torch.sqrt(var + f32(COND_EPS))
    scale = gamma.double() * invstd
    shift = beta.double() - m * scale
    mean, invstd, scale, shift = (t.float() for t in (m, invstd, scale, shift))
    dout = torch.randn(pooled_shape(shape, pool) + (C,), generator=g).to(y_dtype(io)).float()
    y = zd * scale.double() + shift.double()
    thr = COND_AMBIGUOUS * y.std((0, 1, 2, 3))
    if pool == POOL_NONE:
        bad = y.abs() < thr
    else:
        yw, zw = windows(y), windows(zd)
        if pool == POOL_AVG:
            bad = (yw.abs() < thr.view(-1, 1)).any(-1)
        else:
            top = yw.topk(2, -1)
            ztop = zw.gather(-1, top.indices)
            near = (top.values[..., 0] - top.values[..., 1] < thr) & (ztop[..., 0] != ztop[..., 1])   # equal z: an exact tie in any arithmetic
            bad = near | (top.values[..., 0].abs() < thr)
    dout[bad] = 0.0
    return dict(z=z, dout=dout, scale=scale, shift=shift, mean=mean, invstd=invstd), float(bad.float().mean())


def cond_quantities(inp, slope, pool, dtype):
    """The judged quantities of a conditioning case in `dtype`: out, dz (with coef = the fp64 sums / count rounded to fp32, the
    same in both precisions), dbeta = S1 and dgamma = S2; and `top`, the scale each channel of a quantity is judged against:
    its own max |fp64 value| for the tensors, and for the two sums the channel's sum of |terms| (fp64).  A sum of zero-mean
    terms lands anywhere in +-sqrt(n) rms, now and then next to 0, while the error of ANY fp32 evaluation (one rounding per
    product, then the additions) scales with the terms: |error| <= gamma_n sum |terms| is the bound of a floating-point sum,
    and |S| itself as the scale would judge the luck of the seed, not the arithmetic."""
    z, dout = inp["z"], inp["dout"]
    count = z.numel() // z.shape[-1]
    dy64 = dy_ref(z, dout, inp["scale"], inp["shift"], slope, pool)
    s1, s2 = sums_ref(z, dy64, inp["mean"], inp["invstd"])
    coef = (torch.stack([s1, s2]) / count).float()
    dy = dy64 if dtype == torch.float64 else dy_ref(z, dout, inp["scale"], inp["shift"], slope, pool, dtype)
    q1, q2 = sums_ref(z, dy, inp["mean"], inp["invstd"], dtype)
    r = dict(out=forward_ref(z, inp["scale"], inp["shift"], slope, pool, dtype),
             dz=dz_ref(z, dy, inp["scale"], inp["mean"], inp["invstd"], coef, dtype),
             dbeta=q1.view(1, -1), dgamma=q2.view(1, -1), coef=coef)
    if dtype == torch.float64:
        xhat = (z.double() - inp["mean"].double()) * inp["invstd"].double()
        r["top"] = dict(out=r["out"].abs().reshape(-1, z.shape[-1]).max(0).values if r["out"].numel() else torch.zeros(z.shape[-1]),
                        dz=r["dz"].abs().reshape(-1, z.shape[-1]).max(0).values,
                        dbeta=dy64.abs().sum((0, 1, 2, 3)), dgamma=(dy64 * xhat).abs().sum((0, 1, 2, 3)))
    return r


COND_QUANTITIES = ("out", "dz", "dbeta", "dgamma")


def cond_restatement_distance(C, io, shape, pool):
    """Largest per-channel distance of the fp32 restatement to the fp64 reference, per judged quantity."""
    inp, _ = cond_inputs(C, io, shape, pool)
    r64 = cond_quantities(inp, f32(COND_SLOPE), pool, torch.float64)
    r32 = cond_quantities(inp, f32(COND_SLOPE), pool, torch.float32)
    return {k: per_channel_distance(r32[k], r64[k], r64["top"][k]) for k in COND_QUANTITIES}


COND_MARGIN = 4.0          # a kernel may differ from fp64 by this many restatement distances (another order of additions, FMA)
# The distances cond_restatement_distance measured (torch 2.x CPU, fp32 against fp64), keyed by (C, io, shape, pool); the
# kernels are held to COND_MARGIN times these, tests/test_host_bn_reduce.py recomputes them and fails on a drift beyond 2x.
COND_DISTANCE = {
    (12, 0, (2, 9, 11, 10), 0): dict(out=6.98e-07, dz=9.49e-08, dbeta=9.62e-09, dgamma=1.04e-08),
    (12, 0, (2, 9, 11, 10), 1): dict(out=6.33e-07, dz=1.05e-07, dbeta=7.35e-09, dgamma=1.24e-08),
    (12, 0, (2, 9, 11, 10), 2): dict(out=8.91e-07, dz=9.94e-08, dbeta=1.03e-08, dgamma=9.77e-09),
    (12, 0, (2, 22, 20, 22), 0): dict(out=3.84e-07, dz=8.61e-08, dbeta=3.20e-09, dgamma=1.85e-09),
    (12, 0, (2, 22, 20, 22), 1): dict(out=4.42e-07, dz=9.43e-08, dbeta=5.41e-09, dgamma=4.19e-09),
    (12, 0, (2, 22, 20, 22), 2): dict(out=6.39e-07, dz=9.71e-08, dbeta=5.54e-09, dgamma=4.00e-09),
    (64, 0, (2, 9, 11, 10), 0): dict(out=5.49e-07, dz=1.23e-07, dbeta=1.41e-08, dgamma=1.31e-08),
    (64, 0, (2, 9, 11, 10), 1): dict(out=5.71e-07, dz=1.24e-07, dbeta=1.63e-08, dgamma=1.78e-08),
    (64, 0, (2, 9, 11, 10), 2): dict(out=1.28e-06, dz=1.13e-07, dbeta=1.82e-08, dgamma=1.76e-08),
    (64, 0, (2, 22, 20, 22), 0): dict(out=5.72e-07, dz=1.36e-07, dbeta=4.07e-09, dgamma=5.08e-09),
    (64, 0, (2, 22, 20, 22), 1): dict(out=4.39e-07, dz=1.02e-07, dbeta=6.65e-09, dgamma=8.53e-09),
    (64, 0, (2, 22, 20, 22), 2): dict(out=7.81e-07, dz=1.06e-07, dbeta=4.82e-09, dgamma=5.26e-09),
    (64, 3, (2, 9, 11, 10), 0): dict(out=5.28e-07, dz=1.17e-07, dbeta=8.11e-09, dgamma=1.74e-08),
    (64, 3, (2, 9, 11, 10), 1): dict(out=5.98e-07, dz=1.41e-07, dbeta=7.92e-09, dgamma=2.05e-08),
    (64, 3, (2, 9, 11, 10), 2): dict(out=1.02e-06, dz=1.20e-07, dbeta=1.89e-08, dgamma=2.26e-08),
    (64, 3, (2, 22, 20, 22), 0): dict(out=4.83e-07, dz=1.21e-07, dbeta=4.91e-09, dgamma=4.29e-09),
    (64, 3, (2, 22, 20, 22), 1): dict(out=4.65e-07, dz=1.01e-07, dbeta=2.97e-09, dgamma=6.34e-09),
    (64, 3, (2, 22, 20, 22), 2): dict(out=1.18e-06, dz=1.30e-07, dbeta=4.21e-09, dgamma=5.43e-09),
}


# ---------------------------------------------------------------------------------------------------------------------
# C. finalize kernels with chosen partials
# ---------------------------------------------------------------------------------------------------------------------
FIN_NBLK = (1, 2, 255, 256, 257, 5000)
FIN_CHANNELS = (1, 3, 64, 260)
EVAL_CHANNELS = (1, 255, 256, 257, 1000)


def stat_partials(nblk, C, count, seed=0):
    """fp32 partials (nblk, 2, C) of sum z and sum z^2 as equal blocks of a tensor of `count` voxels per channel would leave
    them: channel c has sd 1 and mean / sd = 10^(c % 4) (up to 1e3), except channels 1 and 2 (when there are such), which are
    CONSTANT (z = 37.3 and 5.7): their fp32-rounded sums put the variance a rounding error away from zero, on either side.  The
    partials of a channel are of one magnitude, so their fp64 sum carries a few roundings of 2^-53 at the most, in any order."""
    rs = np.random.RandomState(seed + 13 * nblk + C)
    per = count / nblk                                          # voxels per block (a real number: only the sums matter)
    mean = (10.0 ** (np.arange(C) % 4)) * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    s1 = per * mean[None, :] + math.sqrt(per) * rs.standard_normal((nblk, C))
    s2 = per * (mean[None, :] ** 2 + 1.0) + math.sqrt(per) * 2.0 * np.abs(mean)[None, :] * rs.standard_normal((nblk, C))
    for c, v in ((1, 37.3), (2, 5.7)):
        if c < C:
            s1[:, c] = per * v
            s2[:, c] = per * (v * v)
    part = np.stack([s1, np.abs(s2)], axis=1).astype(np.float32)
    return torch.from_numpy(part)


def grad_partials(nblk, C, seed=0):
    """fp32 partials (nblk, 2, C) of sum dy and sum dy xhat: zero-mean, so the fp64 sums cancel."""
    rs = np.random.RandomState(seed + 29 * nblk + C)
    return torch.from_numpy((rs.standard_normal((nblk, 2, C)) * 10.0).astype(np.float32))


def channel_vectors(C, seed=0):
    """(gamma of both signs, beta, conv_bias, running_mean, running_var > 0), float32 (C,)."""
    rs = np.random.RandomState(seed + C)
    gamma = ((0.5 + rs.rand(C)) * np.where(rs.rand(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    beta, bias, rmean = (rs.standard_normal(C).astype(np.float32) for _ in range(3))
    rvar = (0.1 + 2.0 * rs.rand(C)).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (gamma, beta, bias, rmean, rvar))


# ---------------------------------------------------------------------------------------------------------------------
# column sums and weight gradients in integers
# ---------------------------------------------------------------------------------------------------------------------
COLSUM_NBLK = (1, 15, 16, 17, 63, 64, 65, 200)
COLSUM_NCOL = (1, 63, 64, 65, 400)


def colsum_partials(nblk, ncol, seed=0):
    """Integer partials (nblk, ncol) of magnitude up to 2^20 whose column sums cancel to integers of magnitude <= 8: pairs
    (v, -v) in a shuffled row order plus one small row.  Every partial sum is an integer below 2^28 - exact in fp64 (and the
    result in fp32) under any order of additions."""
    rs = np.random.RandomState(seed + 1000 * nblk + ncol)
    p = np.zeros((nblk, ncol), dtype=np.int64)
    half = (nblk - 1) // 2
    v = rs.randint(-(1 << 20), (1 << 20) + 1, (half, ncol))
    p[:half], p[half:2 * half] = v, -v
    p[2 * half:] = rs.randint(-4, 5, (nblk - 2 * half, ncol))
    for c in range(ncol):
        p[:, c] = p[rs.permutation(nblk), c]
    return torch.from_numpy(p)


def wgrad_inputs(shape, cin, cout, seed=0):
    """Integer x (B, D, H, W, cin) and dz (B, D, H, W, cout) in [-2, 2]: every product, slab, fp64 sum and the fp32 scratch round
    trip of the weight gradient are integers below 4 B D H W < 2^24."""
    B, D, H, W = shape
    assert 4 * B * D * H * W < 1 << 24
    g = torch.Generator().manual_seed(seed + 100 * cin + cout + D)
    return (torch.randint(-2, 3, (B, D, H, W, cin), generator=g).float(),
            torch.randint(-2, 3, (B, D, H, W, cout), generator=g).float())


def wgrad_ref(x, dz, ksize):
    """fp64 weight gradient of conv3d (stride 1, same padding) in the reference layout (cout, cin, k, k, k)."""
    cin, cout = x.shape[-1], dz.shape[-1]
    w = torch.zeros((cout, cin, ksize, ksize, ksize), dtype=torch.float64, requires_grad=True)
    F.conv3d(_ncdhw(x.double()), w, None, 1, ksize // 2).backward(_ncdhw(dz.double()))
    return w.grad


def tap_major(dw_ref):
    """(cout, cin, k, k, k) -> the kernels' own layout [t][cin][cout]."""
    cout, cin = dw_ref.shape[:2]
    return dw_ref.reshape(cout, cin, -1).permute(2, 1, 0).contiguous()
