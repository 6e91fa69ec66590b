"""Which region of which modality carries a prediction: occlusion sensitivity, the gradient-free member of the explanation family.

    from transmf_ad_amd import occlusion_sensitivity
    occ = occlusion_sensitivity(model.eval(), mri, pet, patch=12)       # or stride=6, atlas=labels, fill="mean", score="prob"
    occ.drops(0)                                                        # (B, nd, nh, nw): MRI windows; (B, R) with an atlas
    occ.volume(1)                                                       # (B, D, H, W): the voxel map of the PET volume
    occ.logits, occ.target, occ.base_score, occ.grid, occ.patch, occ.stride

Semantics (include/tmf_hip.h states the same for the kernels):
  Window grid.  Per axis with extent S, patch p and stride s, 1 <= s <= p: n = ceil(max(S - p, 0) / s) + 1 windows, window i
    covers [i*s, min(i*s + p, S)); the last one may be shorter, S <= p gives one window.  nW = nd*nh*nw, window
    w = (id*nh + ih)*nw + iw.  Every voxel lies in at least one window (s <= p).
  Regions.  Instead of a grid, `atlas` is an integer label volume (D, H, W) with labels 0..R (R = its maximum): label 0 is
    background and never occluded, job r-1 occludes all voxels with label r, nW = R.
  Jobs.  Job j = b*nW + w is sample b with window / region w replaced by fill[b], one scalar per sample and modality: a float
    (default 0.0, the minimum after the pipeline's ScaleIntensity), "mean" (the sample's mean) or a tensor (B,).
  Score.  "logit": logits[b, target_b]; "prob": the softmax probability of that class.  target as saliency.input_gradients
    (None: the argmax of the UNOCCLUDED logits, resolved once).
  Drop.  drop[b, w] = score(unoccluded) - score(job): positive where the region supported the class.
  Voxel map.  Grid: vmap[b, z, y, x] = the mean of drop[b, w] over the windows that contain the voxel (sum in ascending w in
    fp32, one division by the count).  Atlas: drop[b, label - 1], 0 on background.
  Model mode.  The model must be in eval mode (ValueError otherwise: train-mode BatchNorm would mix the windows of a chunk).
    Everything runs under torch.no_grad(); the caller's tensors, the parameters' .grad, the buffers and torch's generator
    stay untouched.

`volumes` selects the volume arguments to occlude (default: all, one after the other; drops(i) / volume(i) take the argument's
index); joint=True occludes the same window in all selected volumes at once and gives one map.  Per occluded volume the jobs
are walked in chunks of `chunk`: ONE launch (tmf_occlude_windows / tmf_occlude_labels, csrc/occlusion.hip) writes the chunk's
occluded volumes into a buffer allocated once, the other volumes' rows are index_selected to the chunk's samples, one
model(...) call runs, and the drops come from the (K, classes) logits by torch ops.  One more launch per map
(tmf_occlusion_volume / _labels) puts the drops back on the voxel grid.

reuse=True: blanking a region of one volume leaves the encoders of the other volumes where they were.  Every networks.sNet
of a package model that ran ONCE in the baseline forward, on a volume argument that this pass does not occlude, keeps its
baseline output (taken by a forward hook on the encoder module, which leaves it on its one-call path); for the pass that
output, indexed to the chunk's samples, is the encoder's sNet.tmf_replay — the encoder launches nothing, its input is a
zero-stride expand — and it is taken off again, also when the model raises.  A model with one volume, a module that is not
this package's model class, or joint=True over all volumes has nothing to reuse.

occlusion_sensitivity_torch is the same function with clone and slice assignment and the voxel map in plain torch ops, on any
device and dtype and any nn.Module (the reference's classes on the CPU in float or double); tmf_replay is not used there."""
import torch

from . import ops
from ._explain import SCORES, _fill, _is_int, _on, _pass_arguments, _Pass

__all__ = ["occlusion_sensitivity", "occlusion_sensitivity_torch", "Occlusion", "SCORES"]


def _triple(v, name):
    t = (v,) * 3 if _is_int(v) else tuple(v) if isinstance(v, (tuple, list)) else None
    if t is None or len(t) != 3 or any(not _is_int(x) or x < 1 for x in t):
        raise ValueError(f"{name} must be a positive int or three of them, got {v!r}")
    return t


class Occlusion:
    """logits (B, classes): the unoccluded forward; target (B,): the class explained; base_score (B,); grid (nd, nh, nw) or None
    with an atlas; patch, stride; volumes: the occluded volume arguments' indices; joint."""

    def __init__(self, logits, target, base_score, grid, patch, stride, volumes, joint, size, drops, maps):
        self.logits, self.target, self.base_score = logits, target, base_score
        self.grid, self.patch, self.stride, self.volumes, self.joint, self.size = grid, patch, stride, volumes, joint, size
        self._drops, self._maps = drops, maps

    def _key(self, volume):
        if self.joint and (volume is None or volume in self.volumes):
            return self.volumes[0]
        if volume is None and len(self.volumes) == 1:
            return self.volumes[0]
        if volume not in self._drops:
            raise KeyError(f"no map for volume {volume!r}: occluded volume arguments {self.volumes}")
        return volume

    def drops(self, volume=None):
        """(B, nd, nh, nw), or (B, R) with an atlas: score(unoccluded) - score(occluded) per window / region of volume argument
        `volume` (0 = the first); may be left out where one map was computed."""
        d = self._drops[self._key(volume)]
        return d if self.grid is None else d.view(d.shape[0], *self.grid)

    def volume(self, volume=None):
        """(B, D, H, W): the voxel map of that volume argument."""
        return self._maps[self._key(volume)]


def _run(model, volumes, patch, stride, atlas, fill, score, target, output, which, joint, chunk, reuse, torch_only):
    vols, B = _pass_arguments("occlusion_sensitivity", "windows", model, volumes, score, chunk)
    which = tuple(range(len(vols))) if which is None else (which,) if isinstance(which, int) else tuple(which)
    if not which or any(not _is_int(i) or not 0 <= i < len(vols) for i in which) or len(set(which)) != len(which):
        raise ValueError(f"volumes must name some of the {len(vols)} volume arguments once each, got {which!r}")
    size = tuple(int(s) for s in vols[which[0]].shape[-3:])
    if any(tuple(vols[i].shape[-3:]) != size or vols[i].numel() != B * size[0] * size[1] * size[2] for i in which):
        raise ValueError("the occluded volumes must be one-channel volumes of one spatial shape")
    patch = _triple(patch, "patch")
    stride = patch if stride is None else _triple(stride, "stride")
    if atlas is None:
        grid = ops.occlusion_grid(size, patch, stride)                # ValueError for stride > patch
        nW = grid[0] * grid[1] * grid[2]
    else:
        if not torch.is_tensor(atlas) or atlas.dtype.is_floating_point or atlas.dtype == torch.bool \
                or tuple(atlas.shape) != size:
            raise ValueError(f"atlas must be an integer label volume of shape {size}")
        grid, nW = None, int(atlas.max())
        if nW < 1:
            raise ValueError("atlas has no label above 0: nothing to occlude")
        atlas = atlas.detach().to(device=vols[which[0]].device, dtype=torch.int32).contiguous()
    fills = {i: _fill(fill, vols[i], B) for i in which}

    def occlude(i, j0, K, out):
        if atlas is None:
            return (ops.occlude_windows_torch if torch_only else ops.occlude_windows)(vols[i], fills[i], patch, stride, j0, K, out=out)
        return (ops.occlude_labels_torch if torch_only else ops.occlude_labels)(vols[i], atlas, fills[i], nW, j0, K, out=out)

    with torch.no_grad(), _on(vols[0]):
        run = _Pass(model, vols, score, target, output, chunk, reuse)
        drops, maps = {}, {}
        for occluded in ([which] if joint else [(i,) for i in which]):
            # the chunk buffers of the kernel path, allocated once per pass (the torch ops allocate as they go)
            buffered = [i for i in occluded if not torch_only and ops.occlusion_ok(vols[i])]
            d = run.base.view(B, 1) - run.scores(occluded, nW, occlude, buffered).view(B, nW)
            vmap = (ops.occlusion_volume_torch if torch_only else ops.occlusion_volume)(d, size, patch, stride, labels=atlas)
            for i in (occluded[:1] if joint else occluded):
                drops[i], maps[i] = d, vmap
    return Occlusion(run.logits, run.target, run.base, grid, patch, stride, which, bool(joint), size, drops, maps)


def occlusion_sensitivity(model, *vols, patch=12, stride=None, atlas=None, fill=0.0, score="logit", target=None, output=0,
                          volumes=None, joint=False, chunk=32, reuse=True):
    """Occlusion sensitivity of `model` (eval mode) on the volumes (B, 1, D, H, W) -> Occlusion.  See the module docstring for
    the window grid, atlas, fill, score, target, `volumes`, joint, chunk and reuse.  ValueError for a model in train mode,
    stride > patch, a bad fill, score, atlas or volume index."""
    return _run(model, vols, patch, stride, atlas, fill, score, target, output, volumes, bool(joint), chunk, bool(reuse), False)


def occlusion_sensitivity_torch(model, *vols, patch=12, stride=None, atlas=None, fill=0.0, score="logit", target=None,
                                output=0, volumes=None, joint=False, chunk=32, reuse=False):
    """occlusion_sensitivity with clone and slice assignment and the voxel map in plain torch ops: any device, dtype and
    nn.Module.  `reuse` is accepted and ignored: tmf_replay is not used here."""
    return _run(model, vols, patch, stride, atlas, fill, score, target, output, volumes, bool(joint), chunk, False, True)
