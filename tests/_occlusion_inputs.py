"""Cases, fp64 formulas and tolerances of the occlusion-sensitivity tests (tests/test_host_occlusion.py,
tests/test_gpu_occlusion.py): the kernels of csrc/occlusion.hip and transmf_ad_amd.occlusion_sensitivity.

  Window grid.  Per axis with extent S, patch p, stride s (1 <= s <= p): n = ceil(max(S - p, 0) / s) + 1 windows, window i
    covers [i*s, min(i*s + p, S)); nW = nd*nh*nw, window w = (id*nh + ih)*nw + iw.
  Regions.  labels (D, H, W) with 0..R: job r-1 occludes label r; 0 and anything outside 0..R occludes nothing.
  Jobs.  Job j = b*nW + w: sample b with window / region w set to fill[b].
  Voxel map.  Grid: the mean of drop[b, w] over the windows that contain the voxel.  Regions: drop[b, label-1], else 0.

The writers are pure copies: judged by torch.equal against clone() plus slice assignment (occlude_ref).  The voxel map with
stride == patch is a gather of single drops: torch.equal.  With overlap it is a sum of up to 2^3 (here 4) drops and a
division: per sample row  |kernel - fp64| <= MARGIN x D x max |fp64 row|,  D = the worst such row distance of the fp32 torch
scatter-add formula (volume_formula32) from fp64 on that case, recorded in VOLUME_DISTANCE, never below VOLUME_FLOOR.
Nothing here touches a GPU or reads a file.

    python tests/_occlusion_inputs.py        # prints the table below"""
import itertools

import torch

from _bn_inputs import COND_MARGIN

MARGIN = COND_MARGIN        # = 4: a kernel may differ from fp64 by this many distances of the fp32 formula
VOLUME_FLOOR = 2.0 ** -23   # one fp32 ulp of the row's maximum: a sum and a division are two roundings even where the formula hits fp64

# (B, D, H, W, patch, stride): the smallest volume; odd extents without a multiple of 4 voxels (scalar path) and a stride below
# the patch on one axis; overlap on every axis, 16-byte path, three samples; extents that are no multiple of the patch (short
# last windows), 11 x 13 x 11 from the pooled ADNI shape; a patch larger than the volume (one window); a row of 260 voxels,
# longer than one pass of a workgroup's 256 lanes, with windows 64 wide and 2 high every 1 (overlap along h); the ragged
# fixture shape (35 x 38 x 33 = 43890 voxels, % 4 == 2: scalar path over more than one workgroup).
OCCLUDE_CASES = [
    (1, 4, 4, 4, 2, 2),
    (2, 5, 7, 3, (2, 3, 2), (2, 3, 1)),
    (3, 16, 16, 16, 8, 4),
    (1, 11, 13, 11, 4, 4),
    (1, 6, 6, 6, 8, 8),
    (1, 2, 3, 260, (1, 2, 64), (1, 1, 64)),
    (2, 35, 38, 33, 12, 12),
]
# (size, R) of the atlas cases, two samples each: 3 and 17 labels on an odd shape (scalar path) and on 16^3 (16-byte path)
ATLAS_CASES = [((5, 7, 3), 3), ((5, 7, 3), 17), ((16, 16, 16), 3), ((16, 16, 16), 17)]
ATLAS_BATCH = 2
ATLAS_ABSENT = 2            # the label no voxel carries


def triple(v):
    return (v,) * 3 if isinstance(v, int) else tuple(v)


def geometry(case):
    """-> (B, size, patch, stride) with 3-tuples."""
    B, D, H, W, patch, stride = case
    return B, (D, H, W), triple(patch), triple(stride)


def case_id(case):
    B, size, patch, stride = geometry(case)
    return f"{B}x" + "x".join(map(str, size)) + "-p" + ".".join(map(str, patch)) + "-s" + ".".join(map(str, stride))


def axis_windows(S, p, s):
    """Brute force, not the closed form: windows start every s voxels until one reaches the end of the axis."""
    assert 1 <= s <= p and S >= 1
    wins, start = [], 0
    while True:
        wins.append((start, min(start + p, S)))
        if start + p >= S:
            return wins
        start += s


def windows(size, patch, stride):
    """[(z0, z1, y0, y1, x0, x1)] in window order w = (id*nh + ih)*nw + iw, and (nd, nh, nw)."""
    axes = [axis_windows(S, p, s) for S, p, s in zip(size, patch, stride)]
    wins = [(a[0], a[1], b[0], b[1], c[0], c[1]) for a, b, c in itertools.product(*axes)]
    return wins, tuple(len(a) for a in axes)


def chunkings(B, nW):
    """The (j0, K) chunks every writer case runs: K = 1 (the last job of sample 0); a chunk that starts mid-sample and crosses
    into the next sample (B == 1: runs from mid-sample to the end); the short last chunk of a walk in chunks of 5."""
    total = B * nW
    mid = nW // 2
    cross = (mid, nW if mid else 2) if B > 1 else (mid, nW - mid)
    last = (total - 1) // 5 * 5
    return [(nW - 1, 1), cross, (last, total - last)]


def occlude_inputs(case):
    """-> (vol (B, 1, D, H, W) float32, fill (B,) float32): fill values no voxel holds."""
    B, size, _p, _s = geometry(case)
    g = torch.Generator().manual_seed(11 + 7919 * B + size[0] * 10007 + size[1] * 101 + size[2])
    vol = torch.rand((B, 1) + size, generator=g)
    fill = -1.0 - torch.rand((B,), generator=g)
    return vol, fill


def occlude_ref(vol, fill, patch, stride, j0, K):
    """clone() plus slice assignment, job by job."""
    size = tuple(vol.shape[-3:])
    wins, grid = windows(size, patch, stride)
    nW = len(wins)
    out = []
    for j in range(j0, j0 + K):
        b, w = divmod(j, nW)
        z0, z1, y0, y1, x0, x1 = wins[w]
        x = vol[b].clone()
        x[..., z0:z1, y0:y1, x0:x1] = fill[b]
        out.append(x)
    return torch.stack(out)


def atlas_labels(size, R):
    """int32 (D, H, W): labels 0..R at random with label ATLAS_ABSENT on no voxel, one voxel at R + 3 and one at -1 (both
    outside 0..R: they occlude nothing and map to 0)."""
    g = torch.Generator().manual_seed(5 + R * 1009 + size[0])
    lab = torch.randint(0, R + 1, size, generator=g, dtype=torch.int32)
    lab[lab == ATLAS_ABSENT] = 1
    flat = lab.view(-1)
    flat[3], flat[flat.numel() - 2] = R + 3, -1
    return lab


def atlas_inputs(size, R):
    g = torch.Generator().manual_seed(23 + R + size[2])
    vol = torch.rand((ATLAS_BATCH, 1) + tuple(size), generator=g)
    fill = -1.0 - torch.rand((ATLAS_BATCH,), generator=g)
    return vol, atlas_labels(size, R), fill


def occlude_labels_ref(vol, labels, fill, R, j0, K):
    out = []
    for j in range(j0, j0 + K):
        b, r = divmod(j, R)
        x = vol[b].clone()
        x[..., labels == r + 1] = fill[b]
        out.append(x)
    return torch.stack(out)


def drops_for(B, nW, seed=0):
    """Random drops of mixed signs (B, nW) float32, a few exact zeros."""
    g = torch.Generator().manual_seed(97 + 31 * B + nW + seed)
    d = torch.randn((B, nW), generator=g) * 0.01
    d[:, ::7] = 0.0
    return d


def volume_ref64(drops, size, patch, stride):
    """fp64, voxel by window membership written out: the mean over the windows that contain the voxel."""
    wins, _grid = windows(size, patch, stride)
    B = drops.shape[0]
    acc = torch.zeros((B,) + tuple(size), dtype=torch.float64)
    cnt = torch.zeros(tuple(size), dtype=torch.float64)
    zz, yy, xx = torch.meshgrid(*(torch.arange(S) for S in size), indexing="ij")
    for w, (z0, z1, y0, y1, x0, x1) in enumerate(wins):
        inside = (zz >= z0) & (zz < z1) & (yy >= y0) & (yy < y1) & (xx >= x0) & (xx < x1)
        acc += inside.double() * drops[:, w].double().view(B, 1, 1, 1)
        cnt += inside.double()
    assert bool((cnt >= 1).all())
    return acc / cnt


def volume_formula32(drops, size, patch, stride):
    """The fp32 torch scatter-add formula, as one writes it without the kernel: ascending w, one division."""
    wins, _grid = windows(size, patch, stride)
    B = drops.shape[0]
    acc = torch.zeros((B,) + tuple(size), dtype=torch.float32)
    cnt = torch.zeros(tuple(size), dtype=torch.float32)
    for w, (z0, z1, y0, y1, x0, x1) in enumerate(wins):
        acc[:, z0:z1, y0:y1, x0:x1] += drops[:, w].float().view(B, 1, 1, 1)
        cnt[z0:z1, y0:y1, x0:x1] += 1
    return acc / cnt


def volume_labels_ref(drops, labels, R):
    lab = labels.long()
    out = torch.zeros((drops.shape[0],) + tuple(labels.shape), dtype=drops.dtype)
    for r in range(1, R + 1):
        out[:, lab == r] = drops[:, r - 1].view(-1, 1)
    return out


def row_errors(got, ref64):
    """Per sample: max |got - fp64| / max |fp64 row| (the absolute error where that is 0); non-finite -> inf."""
    B = ref64.shape[0]
    ref = ref64.double().reshape(B, -1)
    got = got.double().reshape(B, -1)
    err = (got - ref).abs().amax(1)
    scale = ref.abs().amax(1)
    rel = torch.where(scale > 0, err / scale.clamp_min(1e-300), err)
    return torch.where(torch.isfinite(got).all(1), rel, torch.full_like(rel, float("inf")))


def overlapping(case):
    _B, _size, patch, stride = geometry(case)
    return patch != stride and any(s < min(p, S) for S, p, s in zip(_size, patch, stride))


def volume_distance(case):
    """The worst row distance of the fp32 formula from fp64 on the case's drops."""
    B, size, patch, stride = geometry(case)
    wins, _g = windows(size, patch, stride)
    d = drops_for(B, len(wins))
    return float(row_errors(volume_formula32(d, size, patch, stride), volume_ref64(d, size, patch, stride)).max())


def volume_tolerance(case):
    """MARGIN x the recorded distance, not below VOLUME_FLOOR: relative to max |fp64 row|."""
    return MARGIN * max(VOLUME_DISTANCE[case_id(case)], VOLUME_FLOOR)


# ---------------------------------------------------------------------------------------------------------------------
# recorded distances of the fp32 scatter-add formula from fp64 (torch 2.x CPU) on the overlapping cases;
# tests/test_host_occlusion.py measures them again and fails on a drift beyond 2x.  Enters a tolerance through volume_tolerance().
# ---------------------------------------------------------------------------------------------------------------------
# BEGIN TABLES
VOLUME_DISTANCE = {
    '2x5x7x3-p2.3.2-s2.3.1': 2.65e-08,
    '3x16x16x16-p8.8.8-s4.4.4': 3.46e-08,
    '1x2x3x260-p1.2.64-s1.1.64': 1.01e-08,
}
# END TABLES


if __name__ == "__main__":
    print("VOLUME_DISTANCE = {")
    for case_ in OCCLUDE_CASES:
        if overlapping(case_):
            print(f"    {case_id(case_)!r}: {volume_distance(case_):.2e},")
    print("}")
