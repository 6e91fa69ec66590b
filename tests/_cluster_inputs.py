"""Inputs and the numpy reference of the cluster tests (test_host_clusters.py, test_gpu_clusters.py).  No GPU, no file reads, numpy
only.

reference_labels: every foreground voxel starts with its own linear index and takes the minimum over its neighbourhood (shifted
copies of the array), then jumps to its pointer's pointer, to a fixed point; the roots (voxels that kept their own index) of the
clusters with at least min_size voxels are numbered in raster order.  test_host_clusters.py checks it against
scipy.ndimage.label on every mask below.
reference_table: numpy ufunc.at over the labelled voxels.

Masks.  The kernels label 8 x 8 x 32 tiles (d x h x w), so the largest shape (2, 17, 33, 70) crosses a tile boundary in each
axis and has ragged tiles at every far face; (2, 5, 6, 7) is smaller than one tile with V % 4 != 0.
Values.  The foreground of a mask gets magnitudes 1 + |randn|, the background magnitudes below 0.25, the threshold is THR = 0.5;
mode "pos" takes them as they are, "neg" negated, "abs" with random signs - so one mask serves the three modes."""
import functools

import numpy as np

THR = 0.5
TILE = (8, 8, 32)
SHAPES = ((1, 1, 1, 1), (2, 5, 6, 7), (1, 16, 16, 16), (2, 17, 33, 70))
CONNECTIVITIES = (6, 18, 26)
MODES = ("pos", "neg", "abs")
MASKS = ("empty", "full", "checker", "random10", "random31", "random50", "snake", "comb", "diagonals", "two_samples", "planes_d",
         "planes_h", "planes_w")
VALUES = ("randn", "zeros_nan", "constant")


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def offsets(connectivity):
    """The neighbour offsets (dd, dh, dw): |dd| + |dh| + |dw| <= 1 (6), 2 (18), 3 (26)."""
    most = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dd, dh, dw) for dd in (-1, 0, 1) for dh in (-1, 0, 1) for dw in (-1, 0, 1)
            if 0 < abs(dd) + abs(dh) + abs(dw) <= most]


def _shifted(x, off, fill):
    """y[p] = x[p + off], `fill` where p + off lies outside."""
    out = np.full_like(x, fill)
    src, dst = [], []
    for o, n in zip(off, x.shape):
        if abs(o) >= n:
            return out
        dst.append(slice(max(-o, 0), n - max(o, 0)))
        src.append(slice(max(o, 0), n - max(-o, 0)))
    out[tuple(dst)] = x[tuple(src)]
    return out


def reference_labels(mask, connectivity, min_size=1):
    """mask (D, H, W) bool -> (labels (D, H, W) int32, n)."""
    mask = np.asarray(mask, dtype=bool)
    V = mask.size
    idx = np.arange(V, dtype=np.int64).reshape(mask.shape)
    lab = np.where(mask, idx, V)
    offs = offsets(connectivity)
    flat_mask = mask.reshape(-1)
    while True:
        new = lab
        for off in offs:
            new = np.minimum(new, _shifted(lab, off, V))
        new = np.where(mask, new, V).reshape(-1)
        while True:                                         # pointer jumping: a voxel's pointer lies in its own cluster
            jumped = np.where(flat_mask, new[np.where(flat_mask, new, 0)], V)
            if np.array_equal(jumped, new):
                break
            new = jumped
        new = new.reshape(mask.shape)
        if np.array_equal(new, lab):
            break
        lab = new
    lab = lab.reshape(-1)
    size = np.bincount(lab[flat_mask], minlength=V + 1)[:V]
    keep = flat_mask & (lab == idx.reshape(-1)) & (size >= min_size)
    number = np.where(keep, np.cumsum(keep), 0)
    labels = np.where(flat_mask, number[np.where(flat_mask, lab, 0)], 0)
    return labels.astype(np.int32).reshape(mask.shape), int(keep.sum())


def score(a, mode):
    return a if mode == "pos" else -a if mode == "neg" else np.abs(a)


def foreground(a, thr, mode):
    """a (B, D, H, W), thr (B,) of a's dtype -> bool; NaN is never foreground."""
    with np.errstate(invalid="ignore"):
        return score(a, mode) >= np.asarray(thr, dtype=a.dtype).reshape(-1, 1, 1, 1)


def reference_clusters(a, thr, mode, connectivity, min_size=1):
    """a (B, D, H, W) -> (labels (B, D, H, W) int32, n (B,) int32)."""
    fg = foreground(a, thr, mode)
    out = [reference_labels(m, connectivity, min_size) for m in fg]
    return np.stack([l for l, _n in out]), np.array([n for _l, n in out], dtype=np.int32)


def reference_table(a, labels, mode, K):
    """a, labels (B, D, H, W) -> dict size (B, K) int32, peak (B, K) of a's dtype (NaN for an empty row), argmax (B, K) int32 (-1),
    coord_sum (B, K, 3) int64, bbox (B, K, 6) int32 ((D, H, W, -1, -1, -1))."""
    B, D, H, W = a.shape
    V = D * H * W
    size = np.zeros((B, K), np.int32)
    peak = np.full((B, K), np.nan, a.dtype)
    argmax = np.full((B, K), -1, np.int32)
    coord_sum = np.zeros((B, K, 3), np.int64)
    bbox = np.tile(np.array([D, H, W, -1, -1, -1], np.int32), (B, K, 1))
    for b in range(B):
        lab = labels[b].reshape(-1).astype(np.int64)
        at = np.flatnonzero((lab >= 1) & (lab <= K))
        if at.size == 0:
            continue
        row = lab[at] - 1
        s = score(a[b].reshape(-1)[at], mode) + 0.0
        zyx = np.stack([at // (H * W), at // W % H, at % W], 1)
        np.add.at(size[b], row, 1)
        best = np.full(K, -np.inf)
        np.maximum.at(best, row, s.astype(np.float64))
        hit = s == best[row]
        first = np.full(K, V, np.int64)
        np.minimum.at(first, row[hit], at[hit])
        live = first < V
        argmax[b, live] = first[live]
        peak[b, live] = a[b].reshape(-1)[first[live]]
        for c in range(3):
            np.add.at(coord_sum[b, :, c], row, zyx[:, c])
            np.minimum.at(bbox[b, :, c], row, zyx[:, c].astype(np.int32))
            np.maximum.at(bbox[b, :, 3 + c], row, zyx[:, c].astype(np.int32))
    return dict(size=size, peak=peak, argmax=argmax, coord_sum=coord_sum, bbox=bbox)


# ---------------------------------------------------------------------------------------------------------------------
# masks
# ---------------------------------------------------------------------------------------------------------------------

def _snake(D, H, W):
    """One serpentine path: the rows of even h in the planes of even d, joined at alternating ends, the planes joined by one voxel."""
    m = np.zeros((D, H, W), bool)
    end = 0                                                  # the w where the path stands
    for d in range(0, D, 2):
        rows = list(range(0, H, 2))
        if (d // 2) % 2:
            rows.reverse()
        for j, h in enumerate(rows):
            m[d, h, :] = True
            end = W - 1 - end
            if j + 1 < len(rows):
                m[d, (h + rows[j + 1]) // 2, end] = True
        if d + 1 < D:
            m[d + 1, rows[-1], end] = True
    return m


def _diagonals(D, H, W):
    """Pairs that touch by an edge only (three orientations, one of them across +h, -w) or by a corner only, anchored at the
    coordinates 3 mod 4: 3 -> 4 lies inside a tile, 7 -> 8 crosses one in d and h, 31 -> 32 in w."""
    m = np.zeros((D, H, W), bool)
    partner = ((0, 1, 1), (1, 1, 1), (1, 1, 0), (1, 0, 1))
    for d in range(3, D, 4):
        for h in range(3, H, 4):
            for w in range(3, W, 4):
                kind = (d // 4 + h // 4 + w // 4) % 5
                if kind == 4:                               # (d, h, w + 1) and (d, h + 1, w): the backward neighbour lies at +w
                    if h + 1 < H and w + 1 < W:
                        m[d, h, w + 1] = m[d, h + 1, w] = True
                    continue
                pd, ph, pw = d + partner[kind][0], h + partner[kind][1], w + partner[kind][2]
                m[d, h, w] = True
                if pd < D and ph < H and pw < W:
                    m[pd, ph, pw] = True
    return m


@functools.lru_cache(maxsize=None)
def mask(kind, shape):
    """(B, D, H, W) bool, read-only."""
    B, D, H, W = shape
    d, h, w = np.ogrid[:D, :H, :W]
    rng = np.random.default_rng(sum(map(ord, kind)) * 1000 + D * H * W + B)
    if kind == "empty":
        m = np.zeros(shape, bool)
    elif kind == "full":
        m = np.ones(shape, bool)
    elif kind == "checker":
        m = np.broadcast_to((d + h + w) % 2 == 0, shape).copy()
    elif kind.startswith("random"):
        m = rng.random(shape) < int(kind[6:]) / 100
    elif kind == "snake":
        m = np.stack([_snake(D, H, W)] * B)
    elif kind == "comb":                                    # teeth along d at even h, w, joined only in the LAST plane
        one = np.broadcast_to((h % 2 == 0) & (w % 2 == 0) & (d < D), (D, H, W)).copy()
        one[D - 1] = True
        m = np.stack([one] * B)
    elif kind == "diagonals":
        m = np.stack([_diagonals(D, H, W)] * B)
    elif kind == "two_samples":                             # sample 0 full, the others empty
        m = np.zeros(shape, bool)
        m[0] = True
    elif kind.startswith("planes_"):
        axis = {"d": d, "h": h, "w": w}[kind[7:]]
        m = np.broadcast_to(axis % 2 == 0, shape).copy()
    else:
        raise KeyError(kind)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def values(kind, mask_kind, shape, mode):
    """float32 (B, D, H, W), read-only, whose foreground at THR under `mode` is mask(mask_kind, shape)."""
    m = mask(mask_kind, shape)
    rng = np.random.default_rng(sum(map(ord, kind + mask_kind)) + m.size)
    if kind == "constant":                                  # every peak ties: the lowest index wins
        mag = np.where(m, 1.0, 0.0)
    else:
        mag = np.where(m, 1.0 + np.abs(rng.standard_normal(shape)), 0.25 * rng.random(shape))
    if mode == "abs":
        a = mag * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    else:
        a = mag if mode == "pos" else -mag
    a = a.astype(np.float32)
    if kind == "zeros_nan":                                 # +0.0 / -0.0 in the background and a NaN or two
        bg = np.flatnonzero(~m.reshape(-1))
        flat = a.reshape(-1)
        flat[bg[::2]] = 0.0
        flat[bg[1::2]] = -0.0
        flat[bg[:: max(1, bg.size // 2 + 1)]] = np.nan
        if bg.size > 3:
            flat[bg[bg.size // 3]] = np.nan
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def labels_of(mask_kind, shape, connectivity, min_size=1):
    """reference_labels of every sample of a mask, computed once: (labels (B, D, H, W) int32, n (B,) int32), read-only."""
    seen = {}                                                # equal samples are labelled once
    out = []
    for m in mask(mask_kind, shape):
        key = m.tobytes()
        if key not in seen:
            seen[key] = reference_labels(m, connectivity, min_size)
        out.append(seen[key])
    lab, n = np.stack([l for l, _n in out]), np.array([k for _l, k in out], dtype=np.int32)
    lab.setflags(write=False)
    n.setflags(write=False)
    return lab, n
