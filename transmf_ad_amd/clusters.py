"""The cluster table of a voxel map: threshold input_gradients, integrated_gradients, grad_cam(...).volume(),
occlusion_sensitivity(...).volume() or an attention map, find the connected clusters, report each cluster's size, peak, peak
voxel, centre and extent.

    from transmf_ad_amd import clusters
    cl = clusters(attribution, top=0.05)         # attribution (B, D, H, W) or (B, 1, D, H, W); or threshold=...
    cl.labels                                    # (B, D, H, W) int32: 0 background, 1..n[b] the clusters of sample b
    cl.n                                         # (B,) int32 on the device
    cl.size, cl.peak, cl.argmax, cl.bbox         # (B, K), (B, K), (B, K), (B, K, 6)
    cl.centroid, cl.peak_voxel(k), cl.order("size"), cl.stats(attribution), cl.table()

Semantics (include/tmf_hip.h states the same for the kernels):
  Foreground.  s(a) >= threshold of the sample, s = a ("pos"), -a ("neg"), |a| ("abs"), compared as floats: a NaN voxel is
    never foreground.  top=p: the threshold of sample b is its ceil(p*V)-th largest s(a), found on the device without a sort
    (ops.rank_thresholds) and handed over there; ties go together, so more than ceil(p*V) voxels may pass.
  Neighbours.  connectivity 6: faces; 18: faces and edges; 26: faces, edges and corners (scipy's generate_binary_structure(3, 1 /
    2 / 3)).  Samples never connect.
  Numbering.  Per sample the clusters of at least min_size voxels are numbered 1, 2, ... in ascending order of their lowest
    linear voxel index - the order of scipy.ndimage.label; smaller clusters and the background are 0.
  A label volume IS an integer atlas: region_stats(a[b:b+1], cl.labels[b]) and occlusion_sensitivity(..., atlas=cl.labels[b])
    take it as it is.

Contiguous float32 maps on a HIP device take the kernels (ops.cluster_label: tmf_cluster_label, eight stream operations whatever
the data; ops.cluster_table: tmf_cluster_table, three launches; csrc/clusters.hip; no host synchronisation in either); every
other tensor - another dtype or layout, the CPU - takes ops.cluster_label_torch and ops.cluster_table_torch, the same functions
in stock torch ops, which return identical integers."""
import math

import torch

from . import ops
from ._explain import _attribution, _dhw, _int, _on, _peak_voxel
from .region_stats import region_stats, region_stats_torch

__all__ = ["clusters", "clusters_torch", "Clusters"]


class Clusters:
    """labels (B, D, H, W) int32; n (B,) int32; size, argmax (B, K) int32; peak (B, K); coord_sum (B, K, 3) int64; bbox (B, K, 6)
    int32 = min d, h, w, max d, h, w; K rows (row k-1 is cluster k); shape = (D, H, W); mode."""

    def __init__(self, labels, n, size, peak, argmax, coord_sum, bbox, mode, torch_only=False):
        self.labels, self.n, self.size, self.peak, self.argmax, self.coord_sum, self.bbox = labels, n, size, peak, argmax, coord_sum, bbox
        self.K, self.shape, self.mode, self._torch_only = size.shape[1], tuple(labels.shape[1:]), mode, torch_only

    @property
    def centroid(self):
        """(B, K, 3) float64: coord_sum / size, NaN for an empty row."""
        n = self.size.double().unsqueeze(2)
        return torch.where(n > 0, self.coord_sum.double() / n.clamp(min=1), torch.full_like(n, float("nan")))

    def peak_voxel(self, k):
        """(B, 3) int64: the (d, h, w) of cluster k's peak, (-1, -1, -1) where the row is empty."""
        return _peak_voxel(self.argmax[:, _int(k, f"k must be a cluster in 1..{self.K}", 1, self.K) - 1], self.shape)

    def order(self, by="size"):
        """(B, K) int64 cluster numbers: the largest first by "size", or the highest s(peak) first by "peak"; ties: the lower
        number first; empty rows last."""
        if by not in ("size", "peak"):
            raise ValueError(f"by must be \"size\" or \"peak\", got {by!r}")
        if by == "size":
            v = self.size.double()
        else:
            s = ops._cluster_score(self.peak.double(), self.mode)
            v = torch.where(self.size > 0, s, torch.full_like(s, float("-inf")))
        return v.sort(dim=1, descending=True, stable=True).indices + 1

    def stats(self, attribution):
        """A list of B RegionStats: region_stats(attribution[b:b+1], labels[b], R=min(K, ops.REGION_MAX)) - the sums of ANY map
        of the same shape per cluster of sample b (bin 0: everything outside the clusters 1..R)."""
        a = _attribution(attribution, self.labels.shape)
        fn = region_stats_torch if self._torch_only else region_stats
        return [fn(a[b:b + 1], self.labels[b], R=min(self.K, ops.REGION_MAX)) for b in range(a.shape[0])]

    def table(self):
        """One host copy -> a list of dict rows (sample, cluster, size, peak, peak_voxel, centroid, bbox), sample-major, empty
        rows left out."""
        B, K = self.size.shape
        host = torch.cat([self.size.double().unsqueeze(2), self.peak.double().unsqueeze(2), self.argmax.double().unsqueeze(2),
                          self.centroid, self.bbox.double()], 2).cpu()
        rows = []
        for b in range(B):
            for k in range(K):
                n, peak, arg = int(host[b, k, 0]), float(host[b, k, 1]), int(host[b, k, 2])
                if n == 0:
                    continue
                rows.append(dict(sample=b, cluster=k + 1, size=n, peak=peak, peak_voxel=_dhw(arg, self.shape),
                                 centroid=tuple(float(x) for x in host[b, k, 3:6]), bbox=tuple(int(x) for x in host[b, k, 6:12])))
        return rows


def _run(attribution, threshold, top, mode, connectivity, min_size, max_clusters, torch_only):
    a = _attribution(attribution)
    B, V = a.shape[0], a[0].numel()
    if (threshold is None) == (top is None):
        raise ValueError("exactly one of threshold and top must be given")
    if mode not in ops.CLUSTER_MODES:
        raise ValueError(f"mode must be one of {tuple(ops.CLUSTER_MODES)}, got {mode!r}")
    if connectivity not in ops.CLUSTER_CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {ops.CLUSTER_CONNECTIVITIES}, got {connectivity!r}")
    _int(min_size, "min_size must be an integer >= 1", 1)
    if max_clusters is not None:
        _int(max_clusters, "max_clusters must be None or an integer >= 1", 1)
    if top is not None and (isinstance(top, bool) or not isinstance(top, (int, float)) or not 0 < top <= 1):
        raise ValueError(f"top must be a fraction in (0, 1], got {top!r}")
    if threshold is not None and torch.is_tensor(threshold):
        if tuple(threshold.shape) != (B,) or not threshold.dtype.is_floating_point:
            raise ValueError(f"a threshold tensor must be floating point ({B},), got {tuple(threshold.shape)} {threshold.dtype}")
    elif threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, (int, float))):
        raise ValueError(f"threshold must be a number or a ({B},) tensor, got {threshold!r}")
    kernels = not torch_only and a.is_contiguous()
    thr_dtype = torch.float32 if a.dtype != torch.float64 else torch.float64
    with torch.no_grad(), _on(a):
        if top is not None:
            count = min(V, max(1, math.ceil(top * V)))
            s = ops._cluster_score(a, mode).reshape(B, V)
            thr = ops.rank_thresholds(s.contiguous() if kernels else s.double(), [count])[0][:, 0]   # stays on the device
            thr = thr.to(thr_dtype).contiguous()
        elif torch.is_tensor(threshold):
            thr = threshold.detach().to(device=a.device, dtype=thr_dtype).contiguous()
        else:
            thr = torch.full((B,), float(threshold), device=a.device, dtype=thr_dtype)
        label = ops.cluster_label if kernels else ops.cluster_label_torch
        labels, n = label(a, thr, mode, connectivity, min_size)
        if max_clusters is None:
            most = int(n.max())                                        # a host read; pass max_clusters to avoid it
            if most < 0:
                raise RuntimeError("tmf_cluster_label hit an internal bound (n = -1): the labels are not valid")
            K = max(1, most)
        else:
            K = min(max_clusters, V)
        table = ops.cluster_table if kernels else ops.cluster_table_torch
        return Clusters(labels, n, *table(a, labels, mode, K), mode, torch_only)


def clusters(attribution, threshold=None, top=None, mode="pos", connectivity=26, min_size=1, max_clusters=None):
    """The connected clusters of the thresholded `attribution` (B, D, H, W) or (B, 1, D, H, W) and their table -> Clusters.
    Exactly one of threshold (a number, or a (B,) tensor, which stays on the device) and top (a fraction in (0, 1]: per sample
    the ceil(top*V)-th largest s(a), ties together).  mode "pos" / "neg" / "abs"; connectivity 6 / 18 / 26; clusters below
    min_size voxels are dropped and the others renumbered.  max_clusters: the rows K of the table (default: the largest n of the
    batch, at least 1 - which is ONE host read of n.max(); an integer avoids it, clusters above it keep their labels but have no
    row).  ValueError for a bad shape, neither or both of threshold / top, a bad mode, connectivity, min_size or max_clusters;
    RuntimeError if a read n is -1."""
    return _run(attribution, threshold, top, mode, connectivity, min_size, max_clusters, False)


def clusters_torch(attribution, threshold=None, top=None, mode="pos", connectivity=26, min_size=1, max_clusters=None):
    """clusters forced onto the stock torch ops (ops.cluster_label_torch, ops.cluster_table_torch): any device and dtype, the
    same integers.  What clusters itself falls back to for tensors the kernels do not take."""
    return _run(attribution, threshold, top, mode, connectivity, min_size, max_clusters, True)
