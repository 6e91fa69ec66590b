"""Shared parts of the Gaussian-smoothing tests (tests/test_host_smooth.py, tests/test_gpu_smooth.py): a vectorised numpy fp64
reference built from the index formulas of include/tmf_hip.h, the maps, the masks, the case list and the derived error bound."""
import numpy as np
import torch

MODES = ("reflect", "constant", "nearest")
TRUNCATE = 4.0
MAX_RADIUS = 32

# shape (B, D, H, W): what it exercises
SHAPES = (
    (1, 1, 1, 1),         # the smallest volume
    (2, 1, 5, 9),         # a one-voxel axis, W below a wave
    (1, 3, 4, 70),        # one element per lane, W beyond a wave
    (2, 9, 8, 36),        # 16 bytes per lane
    (1, 5, 1, 36),        # a one-voxel H axis on the 16-byte path
    (3, 17, 12, 33),      # odd extents, several samples
)
SIGMAS = ((1.0, 1.0, 1.0), (0.0, 2.5, 0.6), (3.0, 0.4, 4.0), (4.0, 4.0, 4.0))
# shapes with a sigma of their own
LIMIT_CASE = ((1, 4, 6, 40), (8.0, 8.0, 8.0))              # r = 32 = the limit, r >> n on two axes
TILES_CASE = ((1, 40, 72, 100), (2.265, 2.265, 2.265))     # FWHM 8 at 1.5: r = 9; several tiles / workgroups along every axis
WORKLOAD_CASE = ((2, 96, 96, 96), (2.265, 2.265, 2.265))   # the workload's own volume
CASES = tuple((s, g, m) for s in SHAPES for g in SIGMAS for m in MODES) \
    + tuple((c[0], c[1], m) for c in (LIMIT_CASE, TILES_CASE) for m in MODES)
MASKED_SHAPES = ((2, 1, 5, 9), (1, 3, 4, 70), (2, 9, 8, 36), (3, 17, 12, 33))
MASKED_CASES = tuple((s, g, m) for s in MASKED_SHAPES for g in SIGMAS for m in MODES)

MAPS = ("normal", "heavy", "zero", "constant", "impulse", "corner", "integers")
STACK = MAPS + ("abs_normal", "abs_heavy")      # what all_maps stacks: every map, and two without negative values
MASKS = ("sparse", "half", "dense", "single", "bricks")


def case_id(case):
    shape, sig, mode = case
    return "x".join(map(str, shape)) + "-s" + "_".join(f"{s:g}" for s in sig) + "-" + mode


def radius(sigma, truncate=TRUNCATE):
    return int(truncate * sigma + 0.5)


def taps64(sigma, truncate=TRUNCATE):
    """The double taps of include/tmf_hip.h: scipy.ndimage.gaussian_filter's kernel."""
    r = radius(sigma, truncate)
    if r == 0:
        return np.ones(1)
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * i * i / (sigma * sigma))
    return w / w.sum()


def source_index(n, r, mode):
    """(n, 2r+1): the source index of output o and tap i = -r..r, -1 where the tap contributes 0."""
    j = np.arange(n)[:, None] + np.arange(-r, r + 1)[None, :]
    if mode == "reflect":
        p = np.mod(j, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)
    if mode == "nearest":
        return np.clip(j, 0, n - 1)
    assert mode == "constant"
    return np.where((j >= 0) & (j < n), j, -1)


def filter_axis(x, axis, w, mode):
    """One 1-D pass of the fp64 array x along `axis`: the taps scattered through the index formula into the n x n matrix of the
    pass, M[o, source(o, i)] += w[i], then one fp64 matrix product along the axis."""
    if w.size == 1:
        return x * w[0]
    n = x.shape[axis]
    src = source_index(n, (w.size - 1) // 2, mode)
    M = np.zeros((n, n))
    o = np.broadcast_to(np.arange(n)[:, None], src.shape)
    np.add.at(M, (o[src >= 0], src[src >= 0]), np.broadcast_to(w[None, :], src.shape)[src >= 0])
    return np.moveaxis(np.tensordot(M, x, axes=([1], [axis])), 0, axis)


def G(x, sigma3, mode, truncate=TRUNCATE):
    """The separable filter over the last three axes of the fp64 array x."""
    for k, s in enumerate(sigma3):
        x = filter_axis(x, x.ndim - 3 + k, taps64(s, truncate), mode)
    return x


def reference(a, sigma3, mode, mask=None, truncate=TRUNCATE):
    """a (B, D, H, W) tensor or array -> the exact result in fp64: G(a), or G(a*m) / G(m) inside the mask and 0 outside."""
    x = np.asarray(a.double().numpy() if torch.is_tensor(a) else a, dtype=np.float64)
    if mask is None:
        return G(x, sigma3, mode, truncate)
    m = (np.asarray(mask.numpy() if torch.is_tensor(mask) else mask) != 0)
    num, den = G(x * m, sigma3, mode, truncate), G(m.astype(np.float64), sigma3, mode, truncate)
    return np.where(m, num / np.where(m, den, 1.0), 0.0)


def bound(a, sigma3, mask=None, truncate=TRUNCATE):
    """(B, 1, 1, 1): the bound include/tmf_hip.h derives.  Each pass is a K = 2r+1 term fp32 dot product of positive weights that
    sum to 1 within rounding: E = the sum over the filtered axes of (2r + 4), |out - exact| <= E * 2^-24 * max|a[b]|; with a mask
    (2E + 2) * 2^-24 * max|a[b]*m|."""
    x = np.abs(np.asarray(a.double().numpy() if torch.is_tensor(a) else a, dtype=np.float64))
    E = sum(2 * radius(s, truncate) + 4 for s in sigma3 if s > 0)
    if mask is not None:
        x = x * (np.asarray(mask.numpy() if torch.is_tensor(mask) else mask) != 0)
        E = 2 * E + 2
    return E * 2.0 ** -24 * x.reshape(x.shape[0], -1).max(1).reshape(-1, 1, 1, 1)


def _seed(kind, shape):
    return sum(ord(c) for c in kind) * 1009 + sum((i + 1) * s for i, s in enumerate(shape))


def maps(kind, B, size):
    """(B, D, H, W) float32."""
    if kind.startswith("abs_"):
        return maps(kind[4:], B, size).abs()
    g = torch.Generator().manual_seed(_seed(kind, (B,) + tuple(size)))
    shape = (B,) + tuple(size)
    if kind == "normal":
        return torch.randn(shape, generator=g)
    if kind == "heavy":
        return torch.randn(shape, generator=g) * torch.exp(3 * torch.randn(shape, generator=g))
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "constant":
        return torch.full(shape, 3.7)
    if kind == "integers":
        return torch.randint(-8, 9, shape, generator=g).float()
    a = torch.zeros(shape)
    if kind == "impulse":
        a[(slice(None),) + tuple(s // 2 for s in size)] = 5.0
    else:
        assert kind == "corner"
        a[:, -1, -1, -1] = -2.5
    return a


def all_maps(B, size):
    """Every map of STACK along the batch: (len(STACK) * B, D, H, W), map k in rows k*B .. k*B + B - 1."""
    return torch.cat([maps(k, B, size) for k in STACK])


def rows(kind, B):
    k = STACK.index(kind)
    return slice(k * B, (k + 1) * B)


def mask(kind, size):
    """(D, H, W) int32; every mask has at least one inside voxel."""
    g = torch.Generator().manual_seed(_seed(kind, size))
    size = tuple(size)
    if kind in ("sparse", "half", "dense"):
        m = (torch.rand(size, generator=g) < {"sparse": 0.05, "half": 0.5, "dense": 0.95}[kind]).to(torch.int32)
        m.view(-1)[int(torch.randint(0, m.numel(), (1,), generator=g))] = 1
        return m
    if kind == "single":
        m = torch.zeros(size, dtype=torch.int32)
        m[tuple(s // 2 for s in size)] = 1
        return m
    assert kind == "bricks"                 # an atlas: bricks of 3^3 voxels labelled 0, 1, 2, ... 6 in turn (0 is outside), one -1
    d, h, w = (torch.arange(s) // 3 for s in size)
    lab = (d[:, None, None] * 5 + h[None, :, None] * 3 + w[None, None, :]) % 7
    lab.view(-1)[0] = 4
    lab.view(-1)[-1] = -1
    return lab.to(torch.int32)
