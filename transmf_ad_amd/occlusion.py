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
import contextlib

import torch
from torch import nn

from . import networks, ops
from .saliency import _check, _logits, _resolve_target

__all__ = ["occlusion_sensitivity", "occlusion_sensitivity_torch", "Occlusion", "SCORES"]

SCORES = ("logit", "prob")


def _triple(v, name):
    t = (v,) * 3 if isinstance(v, int) and not isinstance(v, bool) else tuple(v) if isinstance(v, (tuple, list)) else None
    if t is None or len(t) != 3 or any(not isinstance(x, int) or isinstance(x, bool) or x < 1 for x in t):
        raise ValueError(f"{name} must be a positive int or three of them, got {v!r}")
    return t


def _score(logits, target, score):
    s = logits if score == "logit" else torch.softmax(logits, 1)
    return s.gather(1, target.view(-1, 1))[:, 0]


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


class _Replay:
    """sNet.tmf_replay on the given encoders for one pass; taken off again on exit."""

    def __init__(self, encoders):
        self.encoders = encoders

    def __enter__(self):
        return self

    def set(self, rows):
        for enc, base in self.encoders:
            enc.tmf_replay = base.index_select(0, rows)

    def __exit__(self, *exc):
        for enc, _base in self.encoders:
            enc.tmf_replay = None
        return False


def _baseline(model, vols, output, want_reuse):
    """The unoccluded forward -> (logits, {volume index: [(encoder, channels-last baseline output)]}): every sNet that ran
    exactly once, on one of the volume arguments as it stands."""
    seen, hooks = {}, []
    if want_reuse:
        from . import mymodel
        if isinstance(model, mymodel._FastModeSwitch):
            def hook(mod, args, kwargs, out):
                seen.setdefault(mod, []).append((args[0] if args else next(iter(kwargs.values()), None), out))
            hooks = [m.register_forward_hook(hook, with_kwargs=True) for m in model.modules() if isinstance(m, networks.sNet)]
    try:
        logits = _logits(model, vols, output)
    finally:
        for h in hooks:
            h.remove()
    by_volume = {}
    for enc, runs in seen.items():
        if len(runs) != 1 or not torch.is_tensor(runs[0][0]) or getattr(enc, "tmf_replay", None) is not None:
            continue
        inp, out = runs[0]
        for i, v in enumerate(vols):
            if inp.data_ptr() == v.data_ptr() and inp.shape == v.shape and inp.stride() == v.stride():
                by_volume.setdefault(i, []).append((enc, out.permute(0, 2, 3, 4, 1)))      # back to (B, d, h, w, C)
                break
    return logits, by_volume


def _run(model, volumes, patch, stride, atlas, fill, score, target, output, which, joint, chunk, reuse, torch_only):
    _check(volumes)
    if not isinstance(model, nn.Module):
        raise TypeError(f"occlusion_sensitivity: {type(model).__name__} is not an nn.Module")
    if any(m.training for m in model.modules()):
        raise ValueError("occlusion_sensitivity explains the deployed network: call model.eval() first (train-mode BatchNorm "
                         "would mix the windows of a chunk)")
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    if not isinstance(chunk, int) or isinstance(chunk, bool) or chunk < 1:
        raise ValueError(f"chunk must be a positive integer, got {chunk!r}")
    vols = [v.detach() for v in volumes]
    which = tuple(range(len(vols))) if which is None else (which,) if isinstance(which, int) else tuple(which)
    if not which or any(not isinstance(i, int) or isinstance(i, bool) or not 0 <= i < len(vols) for i in which) \
            or len(set(which)) != len(which):
        raise ValueError(f"volumes must name some of the {len(vols)} volume arguments once each, got {which!r}")
    B = vols[0].shape[0]
    if any(v.dim() < 4 or v.shape[0] != B for v in vols):
        raise ValueError("volumes must be (B, ..., D, H, W) with one batch size")
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
    fills = {}
    for i in which:
        v = vols[i]
        if isinstance(fill, str):
            if fill != "mean":
                raise ValueError(f"fill must be a float, \"mean\" or a tensor ({B},), got {fill!r}")
            fills[i] = v.reshape(B, -1).mean(1)
        elif torch.is_tensor(fill):
            if tuple(fill.shape) != (B,):
                raise ValueError(f"a fill tensor must be ({B},), got {tuple(fill.shape)}")
            fills[i] = fill.detach().to(device=v.device, dtype=v.dtype).contiguous()
        elif isinstance(fill, (int, float)) and not isinstance(fill, bool):
            fills[i] = torch.full((B,), float(fill), device=v.device, dtype=v.dtype)
        else:
            raise ValueError(f"fill must be a float, \"mean\" or a tensor ({B},), got {fill!r}")

    def occlude(i, j0, K, out):
        v = vols[i]
        if torch_only:                                                  # clone and slice assignment, as a user writes it
            jobs = torch.arange(j0, j0 + K, device=v.device)
            x = v.index_select(0, jobs // nW).clone()
            labels = None if atlas is None else atlas.to(v.device)
            for k in range(K):
                b, w = divmod(j0 + k, nW)
                region = ops.occlusion_window(size, patch, stride, w) if atlas is None else (labels == w + 1,)
                x[k][(..., *region)] = fills[i][b]
            return x
        if atlas is None:
            return ops.occlude_windows(v, fills[i], patch, stride, j0, K, out=out)
        return ops.occlude_labels(v, atlas, fills[i], nW, j0, K, out=out)

    # the library launches on the CURRENT device's current stream: make the volumes' device current for the duration
    guard = torch.cuda.device(vols[0].device) if vols[0].is_cuda else contextlib.nullcontext()
    with torch.no_grad(), guard:
        logits, encoders = _baseline(model, vols, output, reuse and not torch_only)
        target = _resolve_target(target, logits)
        base = _score(logits, target, score)
        sides = []
        if logits.is_cuda:
            # the two-encoder models run one encoder on a side stream: order it ahead of the reads of its kept output
            from . import mymodel
            cur = torch.cuda.current_stream(logits.device)
            sides = mymodel.backward_streams(logits.device)
            for s in sides:
                cur.wait_stream(s)
            for encs in encoders.values():
                for _enc, out in encs:
                    out.record_stream(cur)
        drops, maps = {}, {}
        for occluded in ([which] if joint else [(i,) for i in which]):
            kept = [e for i, encs in encoders.items() if i not in occluded for e in encs]
            replayed = {i for i in encoders if i not in occluded}
            # the chunk buffers of the kernel path, allocated once per pass (the torch ops allocate as they go)
            bufs = {i: torch.empty((min(chunk, B * nW),) + tuple(vols[i].shape[1:]), device=vols[i].device, dtype=vols[i].dtype)
                    for i in occluded if not torch_only and ops.occlusion_ok(vols[i])}
            d = torch.empty((B * nW,), device=logits.device, dtype=logits.dtype)
            with _Replay(kept) as replay:
                for j0 in range(0, B * nW, chunk):
                    K = min(chunk, B * nW - j0)
                    rows = torch.arange(j0, j0 + K, device=logits.device) // nW
                    batch = []
                    for i, v in enumerate(vols):
                        if i in occluded:
                            batch.append(occlude(i, j0, K, bufs[i][:K] if i in bufs else None))
                        elif i in replayed:
                            batch.append(v[:1].expand(K, *v.shape[1:]))        # not read: its encoder replays
                        else:
                            batch.append(v.index_select(0, rows.to(v.device)))
                    replay.set(rows)
                    out = _logits(model, batch, output)
                    d[j0:j0 + K] = base.index_select(0, rows) - _score(out, target.index_select(0, rows), score)
            for i in bufs:
                for s in sides:
                    bufs[i].record_stream(s)
            d = d.view(B, nW)
            vmap = (ops.occlusion_volume_torch if torch_only else ops.occlusion_volume)(d, size, patch, stride, labels=atlas)
            for i in (occluded[:1] if joint else occluded):
                drops[i], maps[i] = d, vmap
    return Occlusion(logits, target, base, grid, patch, stride, which, bool(joint), size, drops, maps)


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
