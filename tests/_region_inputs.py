"""Atlases, maps and the numpy fp64 reference of the region statistics tests (tests/test_host_region_stats.py,
tests/test_gpu_region_stats.py): the kernels of csrc/region_stats.hip and transmf_ad_amd.region_stats.

  Bins.  Bin r in 1..R holds the voxels with label r, bin 0 every other voxel (label 0, negative labels, labels above R).
  count, max (the largest a + 0.0 of the bin, -inf where empty) and argmax (the lowest index that attains it, -1 where empty)
  are exact; sum, abs_sum and pos_sum are judged against fp64 sums (their own error, n * 2^-53 * sum |a|, is far below every
  bound used) within the bound include/tmf_hip.h states: n_r * peak_b * 2^-shift + 2^-23 * |exact|, shift = 62 - ceil(log2 V).

Nothing here touches a GPU or reads a file."""
import numpy as np
import torch

F32, I32 = torch.float32, torch.int32
REGION_MAX = 1024

# (B, D, H, W): one voxel; V = 210, V % 4 != 0: one element per lane; fewer voxels than one workgroup's span; several
# workgroups per sample: the flush by global atomics adds up
SHAPES = [(1, 1, 1, 1), (2, 5, 6, 7), (3, 8, 8, 8), (2, 32, 32, 32)]
REGIONS = (1, 7, 116, REGION_MAX)
CASES = [(s, R) for s in SHAPES for R in REGIONS if R <= s[1] * s[2] * s[3]]
ATLASES = ("blocks", "random", "stripes", "single", "background", "out_of_range", "empty_last")
MAPS = ("randn", "decades", "zero", "negative", "integers", "constant", "signed_zeros")


def case_id(case):
    (B, D, H, W), R = case
    return f"{B}x{D}x{H}x{W}-R{R}"


def atlas(kind, size, R, seed=0):
    """(D, H, W) int32.
    blocks        coherent 4 x 4 x 4 bricks, labels 0..R in brick order (a wave's lanes share bins: the run path)
    random        a different label at every voxel, 0..R
    stripes       period 1 along w: neighbouring voxels never share a label (no lane combines its four voxels)
    single        every voxel has label 1
    background    every voxel has label 0
    out_of_range  random with -5, R + 1 and 2^31 - 1 mixed in: they belong to bin 0
    empty_last    random over 0..R-1: region R has no voxel (R == 1: all background)"""
    D, H, W = size
    g = torch.Generator().manual_seed(7 + 13 * D + 17 * H + 19 * W + 23 * R + 29 * seed + ATLASES.index(kind))
    if kind == "blocks":
        z, y, x = torch.meshgrid(torch.arange(D) // 4, torch.arange(H) // 4, torch.arange(W) // 4, indexing="ij")
        lab = ((z * ((H + 3) // 4) + y) * ((W + 3) // 4) + x) % (R + 1)
    elif kind == "random":
        lab = torch.randint(0, R + 1, size, generator=g)
    elif kind == "stripes":
        lab = (torch.arange(W) % (R + 1)).expand(D, H, W).clone()
    elif kind == "single":
        lab = torch.ones(size, dtype=torch.int64)
    elif kind == "background":
        lab = torch.zeros(size, dtype=torch.int64)
    elif kind == "out_of_range":
        lab = torch.randint(0, R + 1, size, generator=g)
        pick = torch.randint(0, 8, size, generator=g)
        lab[pick == 0] = -5
        lab[pick == 1] = R + 1
        lab[pick == 2] = 2 ** 31 - 1
    else:
        lab = torch.randint(0, R, size, generator=g)
    return lab.to(I32)


def maps(kind, B, size, seed=0):
    """(B, D, H, W) float32.
    randn         standard normal
    decades       normal times 10^u, u uniform in -5..5: ten decades of scale in one sample
    zero          all zero: sums 0, max 0, argmax = the bin's lowest index
    negative      -|normal| - 0.5: max < 0, pos_sum 0
    integers      integers in -64..64: every sum is exact
    constant      one value: every voxel ties, argmax = the bin's lowest index
    signed_zeros  normal with +0.0 and -0.0 mixed in (a bin of zeros of both signs has max +0.0)"""
    g = torch.Generator().manual_seed(101 + 3 * B + 5 * sum(size) + 11 * seed + MAPS.index(kind))
    shape = (B,) + tuple(size)
    x = torch.randn(shape, generator=g)
    if kind == "randn":
        return x
    if kind == "decades":
        return x * torch.pow(10.0, torch.rand(shape, generator=g) * 10 - 5)
    if kind == "zero":
        return torch.zeros(shape)
    if kind == "negative":
        return -x.abs() - 0.5
    if kind == "integers":
        return torch.randint(-64, 65, shape, generator=g).to(F32)
    if kind == "constant":
        return torch.full(shape, -0.37)
    pick = torch.randint(0, 3, shape, generator=g)
    x = -x.abs()
    x[pick == 0] = 0.0
    x[pick == 1] = -0.0
    return x


def bins_of(lab, R):
    lab = np.asarray(lab, dtype=np.int64).reshape(-1)
    return np.where((lab >= 0) & (lab <= R), lab, 0)


def reference(a, lab, R):
    """a (B, ...) tensor, lab integers with as many elements as a sample -> dict of numpy arrays: count (R+1,) int64; sum,
    abs_sum, pos_sum (B, R+1) float64; max (B, R+1) in a's precision; argmax (B, R+1) int64; peak (B,) float64."""
    B = a.shape[0]
    a0 = a.detach().cpu().reshape(B, -1) + 0.0                      # -0.0 -> +0.0, in a's own dtype
    x = a0.double().numpy()
    a0 = a0.float().numpy() if a0.dtype in (torch.bfloat16, torch.float16) else a0.numpy()
    V = x.shape[1]
    bins = bins_of(lab, R)
    assert bins.shape == (V,)
    out = {"count": np.bincount(bins, minlength=R + 1), "peak": np.abs(x).max(1)}
    for name, w in (("sum", x), ("abs_sum", np.abs(x)), ("pos_sum", np.maximum(x, 0))):
        out[name] = np.stack([np.bincount(bins, weights=w[b], minlength=R + 1) for b in range(B)])
    mx = np.full((B, R + 1), -np.inf, dtype=a0.dtype)
    arg = np.full((B, R + 1), V, dtype=np.int64)
    for b in range(B):
        np.maximum.at(mx[b], bins, a0[b])
        np.minimum.at(arg[b], bins, np.where(a0[b] == mx[b][bins], np.arange(V), V))
    arg[arg == V] = -1
    out["max"], out["argmax"] = mx, arg
    return out


def shift_of(V):
    return 62 - int(V - 1).bit_length()                             # 62 - ceil(log2 V)


def bound(ref, name, V):
    """The header's bound of sum / abs_sum / pos_sum: n_r * peak_b * 2^-shift + 2^-23 * |exact|, (B, R+1)."""
    return ref["count"][None, :] * ref["peak"][:, None] * 2.0 ** -shift_of(V) + 2.0 ** -23 * np.abs(ref[name])


def check(got, ref, V, what, exact_sums=False, sums_bound=None):
    """got: dict name -> host tensor / array of the six outputs (a missing name is not judged)."""
    g = {k: (v.detach().cpu().float().numpy() if torch.is_tensor(v) and v.dtype in (torch.bfloat16, torch.float16)
             else v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in got.items()}
    if "count" in g:
        assert np.array_equal(g["count"].astype(np.int64), ref["count"]), (what, "count")
    if "max" in g:
        assert np.array_equal(g["max"], ref["max"]) and not np.signbit(g["max"][g["max"] == 0]).any(), (what, "max")
    if "argmax" in g:
        assert np.array_equal(g["argmax"].astype(np.int64), ref["argmax"]), (what, "argmax")
    worst = 0.0
    for name in ("sum", "abs_sum", "pos_sum"):
        if name not in g:
            continue
        err = np.abs(g[name].astype(np.float64) - ref[name])
        if exact_sums:
            assert not err.any(), (what, name, "exact")
        tol = bound(ref, name, V) if sums_bound is None else sums_bound(ref, name)
        assert (err <= tol).all(), (what, name, float((err / np.maximum(tol, 1e-300)).max()))
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0)
    return worst
