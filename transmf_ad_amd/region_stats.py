"""Which brain regions carry a voxel map: atlas region statistics of input_gradients, integrated_gradients,
grad_cam(...).volume(), occlusion_sensitivity(...).volume() and attention maps, and the group table a paper prints.

    from transmf_ad_amd import region_stats, RegionAccumulator
    rs = region_stats(attribution, atlas)        # attribution (B, D, H, W) or (B, 1, D, H, W); atlas (D, H, W) integers
    rs.count                                     # (R+1,) int32: the voxels of each bin, a property of the atlas
    rs.sum, rs.abs_sum, rs.pos_sum, rs.max       # (B, R+1): per sample and bin
    rs.argmax                                    # (B, R+1) int32: the lowest linear voxel index that attains max, -1 for an empty bin
    rs.mean, rs.share("abs"), rs.peak_voxel(r), rs.top(10), rs.table(names)

    acc = RegionAccumulator(rs.R, num_classes=2)
    acc.update(rs.share("abs"), label)           # once per batch: one launch, no host read
    acc.compute()                                # once per epoch: n, mean, std per class and region, Welch's t for two classes

Semantics (include/tmf_hip.h states the same for the kernels):
  Bins.  Bin r in 1..R holds the voxels with atlas label r; bin 0 every other voxel: label 0 (background), negative labels
    and labels above R.  R defaults to the atlas maximum.  ONE atlas serves all samples: the volumes are registered.
  max is the largest attribution + 0.0 of the bin (-0.0 reads as +0.0), -inf for an empty bin.
  Sums.  On the kernels they are integer sums of the values scaled by a power of two: the same bits on every call and for
    every batch a sample is part of, within n_r * peak_b * 2^-shift + 2^-23 * |exact| of exact arithmetic (peak_b = the
    sample's largest |value|, shift = 62 - ceil(log2 V)).  Non-finite values are not supported.

Contiguous float32 maps on a HIP device with R <= ops.REGION_MAX take the kernels (ops.region_stats: tmf_region_stats,
csrc/region_stats.hip: four stream operations, no host synchronisation); every other tensor - another dtype or layout, the
CPU - takes region_stats_torch, the same function in bincount, index_add_ and scatter_reduce.  region_stats refuses more than
ops.REGION_MAX regions; region_stats_torch, called directly, has no limit."""
import math

import torch

from . import ops
from ._explain import _attribution, _int, _on, _peak_voxel

__all__ = ["region_stats", "region_stats_torch", "RegionStats", "RegionAccumulator"]


class RegionStats:
    """count (R+1,) int32; sum, abs_sum, pos_sum, max (B, R+1); argmax (B, R+1) int32; R; size = (D, H, W)."""

    def __init__(self, count, sum, abs_sum, pos_sum, max, argmax, size):
        self.count, self.sum, self.abs_sum, self.pos_sum, self.max, self.argmax = count, sum, abs_sum, pos_sum, max, argmax
        self.R, self.size = count.shape[0] - 1, tuple(size)

    @property
    def mean(self):
        """sum / count, 0 where the bin is empty."""
        n = self.count.to(self.sum.dtype)
        return torch.where(n > 0, self.sum / n.clamp(min=1), torch.zeros_like(self.sum))

    def _mass(self, kind):
        if kind not in ("abs", "pos"):
            raise ValueError(f"kind must be \"abs\" or \"pos\", got {kind!r}")
        return self.abs_sum if kind == "abs" else self.pos_sum

    def share(self, kind="abs"):
        """(B, R+1): the bin's mass (abs_sum or pos_sum) over the mass of the bins 1..R - the background, column 0, is not part
        of the total.  Zeros for a sample without mass, never NaN."""
        mass = self._mass(kind)
        total = mass[:, 1:].sum(1, keepdim=True)
        return torch.where(total > 0, mass / torch.where(total > 0, total, torch.ones_like(total)), torch.zeros_like(mass))

    def peak_voxel(self, r):
        """(B, 3) int64: the (d, h, w) of bin r's argmax, (-1, -1, -1) where the bin is empty."""
        return _peak_voxel(self.argmax[:, _int(r, f"r must be a bin in 0..{self.R}", 0, self.R)], self.size)

    def top(self, k, by="abs"):
        """(indices (B, k) int64 in 1..R, values (B, k)): the k regions with the largest share(by), the largest first."""
        v, i = self.share(by)[:, 1:].topk(_int(k, f"k must lie in 1..{self.R}", 1, self.R), dim=1)
        return i + 1, v

    def table(self, names=None):
        """One host copy -> a list of dict rows (sample, region, name, count, sum, abs_sum, pos_sum, mean, max, argmax, share_abs,
        share_pos), sample-major, for printing or pandas.  names: a sequence of R + 1 names (bin 0 first) or a dict bin -> name."""
        if names is not None and not isinstance(names, dict):
            names = list(names)
            if len(names) != self.R + 1:
                raise ValueError(f"names must hold {self.R + 1} names (bin 0 first), got {len(names)}")
        cols = [self.sum, self.abs_sum, self.pos_sum, self.mean, self.max, self.share("abs"), self.share("pos")]
        host = torch.stack([c.double() for c in cols] + [self.argmax.double(), self.count.double().expand_as(self.sum)]).cpu()
        name = lambda r: (names.get(r, str(r)) if isinstance(names, dict) else names[r]) if names is not None else str(r)
        rows = []
        for b in range(host.shape[1]):
            for r in range(self.R + 1):
                s, a, p, m, mx, sa, sp, arg, n = (float(x) for x in host[:, b, r])
                rows.append(dict(sample=b, region=r, name=name(r), count=int(n), sum=s, abs_sum=a, pos_sum=p, mean=m, max=mx,
                                 argmax=int(arg), share_abs=sa, share_pos=sp))
        return rows


def _run(attribution, atlas, R, torch_only):
    a = _attribution(attribution)
    size = tuple(int(s) for s in a.shape[-3:])
    if not torch.is_tensor(atlas) or atlas.dtype.is_floating_point or atlas.dtype == torch.bool or tuple(atlas.shape) != size:
        raise ValueError(f"atlas must be an integer label volume of shape {size}")
    if R is None:
        R = int(atlas.max())                                           # a host read; pass R to avoid it
    _int(R, "R must be an integer >= 1 (the atlas needs a label above 0)", 1)
    if not torch_only and R > ops.REGION_MAX:
        raise ValueError(f"R = {R} is above the limit of {ops.REGION_MAX} regions; region_stats_torch has none")
    B = a.shape[0]
    # moved and converted once: contiguous int32 on the map's device
    lab = atlas.detach().to(device=a.device, dtype=torch.int32).contiguous().view(-1)
    with torch.no_grad(), _on(a):
        if torch_only or not a.is_contiguous():
            out = ops.region_stats_torch(a.reshape(B, -1), lab, R)
        else:
            out = ops.region_stats(a.view(B, -1), lab, R)             # routes other dtypes and devices to the torch ops itself
    return RegionStats(*out, size)


def region_stats(attribution, atlas, R=None):
    """The statistics of `attribution` (B, D, H, W) or (B, 1, D, H, W) over the regions of `atlas` (D, H, W), an integer label
    volume -> RegionStats.  R: the number of regions (default: the atlas maximum, which is one host read).  ValueError for a float
    or bool atlas, a shape mismatch, R < 1 and, for tensors the kernels take, R above ops.REGION_MAX."""
    return _run(attribution, atlas, R, False)


def region_stats_torch(attribution, atlas, R=None):
    """region_stats in stock torch ops (bincount, index_add_, scatter_reduce; argmax = the lowest index among the voxels equal
    to the bin's max): any device, dtype and R.  What region_stats itself falls back to for tensors the kernels do not take."""
    return _run(attribution, atlas, R, True)


class RegionAccumulator:
    """The group table: n, mean and std of a per-region value (a share, abs_sum, occlusion's drops, ...) per class and region
    over an evaluation.  The state (num_classes, R+1, 3) float64 = (n, sum x, sum x^2) lives on the device of the first update;
    float32 HIP values update it in ONE launch without a host read (ops.region_group_update: tmf_region_group_update, the
    samples in ascending order, no atomics: two runs give the same bits), anything else by the same sums in torch float64."""

    def __init__(self, R, num_classes=2):
        self.R = _int(R, "R must be an integer >= 1", 1)
        self.num_classes = _int(num_classes, "num_classes must be an integer >= 1", 1)
        self._state = None

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def _state_on(self, device):
        if self._state is None:
            self._state = torch.zeros((self.num_classes, self.R + 1, 3), dtype=torch.float64, device=device)
        elif self._state.device != device:
            if bool((self._state[..., 0] != 0).any()):
                raise RuntimeError(f"RegionAccumulator: update on {device} after updates on {self._state.device}; reset() first")
            self._state = self._state.to(device)
        return self._state

    def update(self, values, labels):
        """values (B, R+1), or (B, R) for the regions 1..R alone (occlusion's drops with an atlas: column 0 stays empty);
        labels (B,) integers, the samples' classes - one outside 0..num_classes-1 is skipped."""
        R = self.R
        if not torch.is_tensor(values) or values.dim() != 2 or values.shape[1] not in (R, R + 1) or values.shape[0] < 1 \
                or not values.dtype.is_floating_point:
            raise ValueError(f"values must be a floating-point tensor (B, {R + 1}) or (B, {R}), got "
                             f"{tuple(values.shape) if torch.is_tensor(values) else values!r}")
        B = values.shape[0]
        if not torch.is_tensor(labels) or tuple(labels.shape) != (B,) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
            raise ValueError(f"labels must be an integer tensor ({B},)")
        state = self._state_on(values.device)
        values = values.detach()
        cls = labels.to(device=values.device, dtype=torch.int64)
        with _on(values):
            ops.region_group_update(state, values.contiguous(), cls)

    def compute(self):
        """One device-to-host copy -> {"n" (C, R+1), "mean", "std" (unbiased, 0 where n < 2)} float64 host tensors and, for two
        classes, "t": Welch's t per region (class 1 against class 0; NaN where a class has n < 2 or both variances are 0)."""
        if self._state is None:
            raise RuntimeError("RegionAccumulator.compute() before any update()")
        host = self._state.cpu()                                       # the one device-to-host copy
        n, sx, sxx = host[..., 0], host[..., 1], host[..., 2]
        safe = n.clamp(min=1)
        mean = torch.where(n > 0, sx / safe, torch.zeros_like(sx))
        var = torch.where(n > 1, (sxx - sx * sx / safe).clamp(min=0) / (n - 1).clamp(min=1), torch.zeros_like(sx))
        out = {"n": n.clone(), "mean": mean, "std": var.sqrt()}
        if self.num_classes == 2:
            se = var[1] / n[1].clamp(min=1) + var[0] / n[0].clamp(min=1)
            ok = (n[0] > 1) & (n[1] > 1) & (se > 0)
            out["t"] = torch.where(ok, (mean[1] - mean[0]) / torch.where(ok, se, torch.ones_like(se)).sqrt(),
                                   torch.full_like(se, math.nan))
        return out

    def state_dict(self):
        return {"R": self.R, "num_classes": self.num_classes,
                "state": None if self._state is None else self._state.detach().cpu().clone()}

    def load_state_dict(self, sd):
        if sd["R"] != self.R or sd["num_classes"] != self.num_classes:
            raise ValueError(f"state of RegionAccumulator({sd['R']}, {sd['num_classes']}) does not fit "
                             f"RegionAccumulator({self.R}, {self.num_classes})")
        st = sd["state"]
        if st is None:
            self._state = None
            return
        if tuple(st.shape) != (self.num_classes, self.R + 1, 3) or st.dtype != torch.float64:
            raise ValueError(f"state must be float64 {(self.num_classes, self.R + 1, 3)}, got {tuple(st.shape)} {st.dtype}")
        dev = st.device if self._state is None else self._state.device
        self._state = st.detach().clone().to(dev)
