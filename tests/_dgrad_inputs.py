"""Inputs and the fp64 reference of the first block's data gradient (tests/test_host_input_grad.py,
tests/test_gpu_input_grad.py; the kernel is csrc/conv1_dgrad.hip, the notation include/tmf_hip.h's).

    z_c(v)  = sum_t w[t][c] x~(v + t - 1)                      y = scale_c z + shift_c
    dy_c(v) = dpool_c(window of v) [v is the window's FIRST maximum of y] (y > 0 ? 1 : slope)
    dz_c(v) = scale_c (dy_c(v) - coef[0][c] - coef[1][c] invstd_c (z_c(v) - mean_c))      for EVERY voxel
    dx(u)   = sum_t sum_c w[t][c] dz_c(u - t + 1)

The reference is plain torch on the host (conv3d, leaky_relu, max_pool3d, autograd) and takes scale, shift, mean, invstd and
coef as free inputs, the way the kernel does.  `dtype` is torch.float64 for the reference itself and torch.float32 for its
restatement, the yardstick of the conditioning family.

x (B, D, H, W); w (27, C) tap-major, tap = 9 kd + 3 kh + kw; dpool (B, D/2, H/2, W/2, C)."""
import torch
import torch.nn.functional as F

from _bn_inputs import COND_AMBIGUOUS, COND_MARGIN, COND_MAX_EXCLUDED, f32, windows  # noqa: F401  (re-exported)

# (B, D, H, W, C): the smallest shapes that reach every branch of the kernel
SHAPES = [
    (3, 8, 10, 33, 16),     # C below one channel group, odd W, bricks cut in W
    (1, 9, 13, 35, 40),     # partial second channel group, all three axes odd
    (2, 5, 7, 6, 32),       # barely larger than one brick: the masked border form of the BatchNorm part everywhere
    (1, 4, 8, 8, 128),      # four channel groups, exactly one brick of z, no interior voxel
    (2, 18, 20, 22, 32),    # several bricks with a true interior
]
EMPTY_POOL_SHAPE = (1, 1, 4, 4, 8)      # no pooling window at all: dx is the BatchNorm part alone


def _vec(t, dtype):
    return t.to(dtype).view(1, -1, 1, 1, 1)


def conv_weight(w, dtype):
    """(27, C) tap-major -> the nn.Conv3d layout (C, 1, 3, 3, 3)."""
    return w.to(dtype).t().reshape(-1, 1, 3, 3, 3).contiguous()


def z_ref(x, w, dtype=torch.float64):
    """(B, C, D, H, W)"""
    return F.conv3d(x.to(dtype).unsqueeze(1), conv_weight(w, dtype), padding=1)


def dy_ref(z, scale, shift, dpool, slope, dtype=torch.float64):
    """Autograd of max_pool3d(leaky_relu(y)) with respect to y (torch's first-maximum routing); z, result (B, C, D, H, W)."""
    y = (z * _vec(scale, dtype) + _vec(shift, dtype)).detach().requires_grad_(True)
    if dpool.numel() == 0:
        return torch.zeros_like(y)
    out = F.max_pool3d(F.leaky_relu(y, slope), 2, 2)
    out.backward(dpool.to(dtype).permute(0, 4, 1, 2, 3))
    return y.grad


def dx_ref(inp, slope, dtype=torch.float64):
    """dx (B, D, H, W) of the formulas above in `dtype`."""
    z = z_ref(inp["x"], inp["w"], dtype)
    dy = dy_ref(z, inp["scale"], inp["shift"], inp["dpool"], slope, dtype)
    coef = inp["coef"].to(dtype)
    dz = _vec(inp["scale"], dtype) * (dy - _vec(coef[0], dtype) - _vec(coef[1], dtype) * _vec(inp["invstd"], dtype) * (z - _vec(inp["mean"], dtype)))
    return F.conv_transpose3d(dz, conv_weight(inp["w"], dtype), padding=1)[:, 0].contiguous()


def distance(got, ref):
    """max |got - ref| over the elements, relative to max |ref| (fp64 reference)."""
    top = float(ref.double().abs().max())
    err = float((got.double() - ref.double()).abs().max()) if ref.numel() else 0.0
    return err / top if top > 0 else err


# ---------------------------------------------------------------------------------------------------------------------
# A. exact family: every product and every sum is exact in fp32 under ANY order of additions, FMA or not, factored or not
# ---------------------------------------------------------------------------------------------------------------------
# x integers in [-2, 2] (the first h-rows constant: whole windows tie) - w in {-1, -1/2, 0, 1/2, 1} - scale +-1/2, +-1, +-2
# (0 for one channel: every window of it ties eight ways) - shift k/8 + 1/16 (y is an odd multiple of 1/16, never 0) -
# mean k/2 - invstd 1 or 2 - coef k/2 in [-1, 1] (train) or 0 (eval) - dpool integers in [-2, 2] - slope 1/4.
# Units: dz is a multiple of 1/8, dx of 1/16.
EXACT_SLOPE = 0.25
EXACT_UNIT = 1.0 / 16
EXACT_LIMIT = 2.0 ** 24


def bn_factors(inp):
    """The channel-free form of the BatchNorm part in fp64: a[27], M[27][27] and the collapsed interior stencil N[5][5][5]
       dx_bn(u) = - sum_{t: v = u - t + 1 inside} (a_t + sum_t' M[t][t'] x~(v + t' - 1))."""
    w, scale, mean, invstd, coef = (inp[k].double() for k in ("w", "scale", "mean", "invstd", "coef"))
    a = (w * (scale * (coef[0] - coef[1] * invstd * mean))).sum(1)
    M = torch.einsum("tc,uc,c->tu", w, w, scale * coef[1] * invstd)
    N = torch.zeros(5, 5, 5, dtype=torch.float64)
    for t in range(27):
        for u in range(27):
            N[u // 9 - t // 9 + 2, (u // 3) % 3 - (t // 3) % 3 + 2, u % 3 - t % 3 + 2] += M[t, u]
    return a, M, N


def exact_budget(inp, slope=EXACT_SLOPE):
    """Largest sum of |terms| of a dx element in units of its finest bit: of the formulas as written (every product expanded),
    and of a factored evaluation (routed part + a, M, N stencils on x) — both must stay below 2^24 for exactness."""
    x, w, scale, mean, invstd, coef = (inp[k].double() for k in ("x", "w", "scale", "mean", "invstd", "coef"))
    dt = torch.float64
    z = z_ref(x, w)
    dy = dy_ref(z, inp["scale"], inp["shift"], inp["dpool"], slope)
    zabs = F.conv3d(x.abs().unsqueeze(1), conv_weight(w.abs(), dt), padding=1)
    dzabs = _vec(scale.abs(), dt) * (dy.abs() + _vec(coef[0].abs(), dt) + _vec((coef[1] * invstd).abs(), dt) * (zabs + _vec(mean.abs(), dt)))
    direct = float(F.conv_transpose3d(dzabs, conv_weight(w.abs(), dt), padding=1).max()) / EXACT_UNIT
    a, M, N = bn_factors(inp)
    for t in (a, M, N):
        assert torch.equal(t.float().double(), t), "a prepared coefficient is not an fp32 number"
        assert float(t.abs().max()) / EXACT_UNIT < EXACT_LIMIT
    routed = float(F.conv_transpose3d(_vec(scale.abs(), dt) * dy.abs(), conv_weight(w.abs(), dt), padding=1).max())
    xmax = float(x.abs().max())
    factored = (routed + float(a.abs().sum()) + max(float(M.abs().sum()), float(N.abs().sum())) * xmax) / EXACT_UNIT
    return direct, factored


def exact_inputs(shape, train, seed=0):
    """dict(x, w, scale, shift, mean, invstd, coef, dpool) of float32 tensors on the grids above; asserts the budget."""
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(seed + 7919 * C + 131 * D + 17 * H + W)
    x = torch.randint(-2, 3, (B, D, H, W), generator=g).float()
    nconst = 5 if H >= 7 else 2
    x[:, :, :nconst] = torch.randint(-2, 3, (B,), generator=g).float().view(B, 1, 1, 1)
    w = torch.randint(-2, 3, (27, C), generator=g).float() / 2
    scale = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0])[torch.randint(0, 6, (C,), generator=g)]
    if C > 1:
        scale[min(C - 1, 3)] = 0.0
    shift = torch.randint(-8, 8, (C,), generator=g).float() / 8 + 1.0 / 16
    mean = torch.randint(-2, 3, (C,), generator=g).float() / 2
    invstd = torch.randint(1, 3, (C,), generator=g).float()
    coef = torch.randint(-2, 3, (2, C), generator=g).float() / 2
    if not train:
        coef = torch.zeros(2, C)
    dpool = torch.randint(-2, 3, (B, D // 2, H // 2, W // 2, C), generator=g).float()
    inp = dict(x=x, w=w, scale=scale, shift=shift, mean=mean, invstd=invstd, coef=coef, dpool=dpool)
    direct, factored = exact_budget(inp)
    assert direct < EXACT_LIMIT and factored < EXACT_LIMIT, (shape, direct, factored)
    return inp


def tie_share(inp):
    """Share of the pooling windows (per channel) whose maximum of y is attained more than once."""
    z = z_ref(inp["x"], inp["w"])
    y = (z * _vec(inp["scale"], torch.float64) + _vec(inp["shift"], torch.float64)).permute(0, 2, 3, 4, 1)
    yw = windows(y)
    if 0 in yw.shape:
        return 1.0
    return float(((yw == yw.max(-1, keepdim=True).values).sum(-1) > 1).float().mean())


# ---------------------------------------------------------------------------------------------------------------------
# B. conditioning family
# ---------------------------------------------------------------------------------------------------------------------
COND_SLOPE = 0.01
COND_EPS = 1e-5


def cond_inputs(shape, train, seed=0):
    """x = 0.7 + 1.5 randn, w = 0.2 randn, gamma of both signs; mean, invstd, scale, shift from the fp64 batch statistics of z
    (var: biased), rounded to fp32; dpool = randn, zero where the routing / the LeakyReLU branch of the fp64 reference is ambiguous; coef = the
    fp64 sums / count rounded (train) or 0 (eval).  -> (dict as exact_inputs, excluded share)."""
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(seed + 1000 * C + 10 * D + W)
    x = (0.7 + 1.5 * torch.randn((B, D, H, W), generator=g)).float()
    w = (0.2 * torch.randn((27, C), generator=g)).float()
    gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 4 < 2, 1.0, -1.0)
    beta = 0.3 * torch.randn(C, generator=g)
    z = z_ref(x, w)
    m = z.mean((0, 2, 3, 4))
    var = (z * z).mean((0, 2, 3, 4)) - m * m
    invstd = 1.0 / torch.sqrt(var + f32(COND_EPS))
    scale = gamma.double() * invstd
    shift = beta.double() - m * scale
    mean, invstd, scale, shift = (t.float() for t in (m, invstd, scale, shift))
    dpool = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g).float()
    y = (z * _vec(scale, torch.float64) + _vec(shift, torch.float64)).permute(0, 2, 3, 4, 1)
    thr = COND_AMBIGUOUS * y.std((0, 1, 2, 3))
    yw, zw = windows(y), windows(z.permute(0, 2, 3, 4, 1))
    top = yw.topk(2, -1)
    ztop = zw.gather(-1, top.indices)
    near = (top.values[..., 0] - top.values[..., 1] < thr) & (ztop[..., 0] != ztop[..., 1])
    bad = near | (top.values[..., 0].abs() < thr)
    dpool[bad] = 0.0
    excluded = float(bad.float().mean())
    assert excluded <= COND_MAX_EXCLUDED, (shape, excluded)
    inp = dict(x=x, w=w, scale=scale, shift=shift, mean=mean, invstd=invstd, dpool=dpool, coef=torch.zeros(2, C),
               gamma=gamma, beta=beta.float(), var=var.float())      # (the last three: the module-level view of the block tests)
    if train:
        dy = dy_ref(z, scale, shift, dpool, f32(COND_SLOPE))
        xhat = (z - _vec(mean, torch.float64)) * _vec(invstd, torch.float64)
        count = B * D * H * W
        inp["coef"] = (torch.stack([dy.sum((0, 2, 3, 4)), (dy * xhat).sum((0, 2, 3, 4))]) / count).float()
    return inp, excluded


def cond_restatement_distance(shape, train):
    inp, _ = cond_inputs(shape, train)
    return distance(dx_ref(inp, f32(COND_SLOPE), torch.float32), dx_ref(inp, f32(COND_SLOPE), torch.float64))


# The distances cond_restatement_distance measured (torch CPU, fp32 against fp64), keyed by (shape, train); the kernel is held
# to COND_MARGIN times these, tests/test_host_input_grad.py recomputes them and fails on a drift beyond 2x.
COND_DISTANCE = {
    ((3, 8, 10, 33, 16), True): 6.68e-07,
    ((3, 8, 10, 33, 16), False): 2.29e-07,
    ((1, 9, 13, 35, 40), True): 1.85e-07,
    ((1, 9, 13, 35, 40), False): 1.44e-07,
    ((2, 5, 7, 6, 32), True): 5.54e-07,
    ((2, 5, 7, 6, 32), False): 1.74e-07,
    ((1, 4, 8, 8, 128), True): 2.53e-07,
    ((1, 4, 8, 8, 128), False): 1.00e-07,
    ((2, 18, 20, 22, 32), True): 7.88e-07,
    ((2, 18, 20, 22, 32), False): 2.15e-07,
}
