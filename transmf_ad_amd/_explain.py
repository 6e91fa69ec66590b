"""What the explanation modules share - saliency, gradcam, attention_maps, occlusion, faithfulness, region_stats, clusters: the
model-side helpers (logits, target, score, frozen parameters), the argument checks (volumes, fill, attribution), the small
device helpers (device guard, side-stream wait, voxel coordinates, trilinear resampling) and the perturbation pass.  Private to
the package: the explanation modules import from here, never from each other's underscore names.

A new perturbation-based explanation (RISE masks, a SHAP-style sampler) is: its argument checks behind _pass_arguments, a
write(i, j0, K, out) callable that produces the perturbed rows of volume i for jobs j0 .. j0+K-1 (an ops wrapper with a
kernel behind it and its *_torch formula), one _Pass under torch.no_grad() and _on(device), one or more _Pass.scores(...)
calls, and a result object.  See occlusion._run and faithfulness._run."""
import contextlib

import torch
import torch.nn.functional as F
from torch import nn

from . import networks
from .ops import _int, _is_int

SCORES = ("logit", "prob")


def _logits(model, volumes, output):
    out = model(*volumes)
    if isinstance(out, (tuple, list)):
        if not _is_int(output) or not -len(out) <= output < len(out):
            raise ValueError(f"the model returns {len(out)} outputs, output={output!r} does not exist")
        out = out[output]
    elif output != 0:
        raise ValueError(f"the model returns one tensor, output={output} does not exist")
    if out.dim() != 2:
        raise ValueError(f"output {output} of the model is not (batch, classes) logits: shape {tuple(out.shape)}")
    return out


def _resolve_target(target, logits):
    """-> LongTensor (batch,) on the logits' device; None: each sample's argmax class."""
    B, K = logits.shape
    if target is None:
        return logits.detach().argmax(1)
    if isinstance(target, int):
        target = torch.full((B,), target, dtype=torch.long)
    target = torch.as_tensor(target)
    if target.dim() != 1 or target.shape[0] != B or target.dtype.is_floating_point:
        raise ValueError(f"target must be None, an int or {B} class indices, got shape {tuple(target.shape)} {target.dtype}")
    target = target.to(device=logits.device, dtype=torch.long)
    if bool(((target < 0) | (target >= K)).any()):
        raise ValueError(f"target holds a class outside 0..{K - 1}")
    return target


def _score(logits, target, score):
    """(B,): "logit": logits[b, target_b]; "prob": the softmax probability of that class."""
    s = logits if score == "logit" else torch.softmax(logits, 1)
    return s.gather(1, target.view(-1, 1))[:, 0]


class _Frozen:
    """requires_grad off on every parameter for the duration (the library then skips every weight gradient), restored on exit."""

    def __init__(self, model, on):
        self.params = [p for p in model.parameters() if p.requires_grad] if on else []

    def __enter__(self):
        for p in self.params:
            p.requires_grad_(False)

    def __exit__(self, *exc):
        for p in self.params:
            p.requires_grad_(True)
        return False


def _check(volumes):
    if not volumes:
        raise ValueError("at least one volume")
    for v in volumes:
        if not (torch.is_tensor(v) and v.dtype.is_floating_point):
            raise ValueError("volumes must be floating-point tensors")


def _fill(fill, v, B):
    """fill: a float, "mean" (the mean of each sample of v) or a tensor (B,) -> (B,) of v's dtype on v's device."""
    msg = f"fill must be a float, \"mean\" or a tensor ({B},), got {fill!r}"
    if isinstance(fill, str):
        if fill != "mean":
            raise ValueError(msg)
        return v.reshape(B, -1).mean(1)
    if torch.is_tensor(fill):
        if tuple(fill.shape) != (B,):
            raise ValueError(f"a fill tensor must be ({B},), got {tuple(fill.shape)}")
        return fill.detach().to(device=v.device, dtype=v.dtype).contiguous()
    if isinstance(fill, (int, float)) and not isinstance(fill, bool):
        return torch.full((B,), float(fill), device=v.device, dtype=v.dtype)
    raise ValueError(msg)


def _attribution(attribution, shape=None):
    """A one-channel voxel map (B, D, H, W) or (B, 1, D, H, W) -> its detached (B, D, H, W) view; `shape`: the (B, D, H, W) it
    must have."""
    if not torch.is_tensor(attribution) or not attribution.dtype.is_floating_point or attribution.dim() not in (4, 5) \
            or (attribution.dim() == 5 and attribution.shape[1] != 1) or attribution.numel() == 0:
        raise ValueError("attribution must be a floating-point tensor (B, D, H, W) or (B, 1, D, H, W) with voxels, got "
                         f"{tuple(attribution.shape) if torch.is_tensor(attribution) else attribution!r}")
    a = attribution.detach()
    a = a[:, 0] if a.dim() == 5 else a
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError(f"attribution must hold {tuple(shape)} voxels, got {tuple(attribution.shape)}")
    return a


def _on(x):
    """The library launches on the CURRENT device's current stream: a context that makes x's device current (nothing on the CPU)."""
    return torch.cuda.device(x.device) if x.is_cuda else contextlib.nullcontext()


def _join_side_streams(like, tensors):
    """The two-encoder models run one encoder on a side stream (mymodel.backward_streams).  On like's HIP device: the current
    stream waits for them and `tensors`, which they may have produced, are recorded on it -> the side streams; [] on the CPU."""
    if not like.is_cuda:
        return []
    from . import mymodel
    cur = torch.cuda.current_stream(like.device)
    sides = mymodel.backward_streams(like.device)
    for s in sides:
        cur.wait_stream(s)
    for t in tensors:
        if t.is_cuda:
            t.record_stream(cur)
    return sides


def _dhw(i, size):
    """Linear index (an int or a tensor) into a (D, H, W) volume -> its (d, h, w)."""
    _D, H, W = size
    return i // (H * W), i // W % H, i % W


def _peak_voxel(argmax, size):
    """argmax (B,) linear indices, -1 for none -> (B, 3) int64 of (d, h, w), (-1, -1, -1) where there is none."""
    i = argmax.long()
    zyx = torch.stack(_dhw(i, size), 1)
    return torch.where((i >= 0).view(-1, 1), zyx, torch.full_like(zyx, -1))


def _trilinear(x, size, default):
    """x (B, C, d, h, w) resampled to the three extents `size` (None: `default`) by trilinear interpolation, align_corners=False."""
    size = default if size is None else tuple(int(s) for s in size)
    if size is None or len(size) != 3:
        raise ValueError(f"size must be three spatial extents, got {size!r}")
    return F.interpolate(x, size=size, mode="trilinear", align_corners=False)


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
    """The unperturbed forward -> (logits, {volume index: [(encoder, channels-last baseline output)]}): every sNet that ran
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


def _pass_arguments(name, jobs, model, volumes, score, chunk):
    """The checks in front of every pass -> (the detached volumes, B).  name: the public function, jobs: what a chunk holds
    ("windows", "jobs"), both for the messages."""
    _check(volumes)
    if not isinstance(model, nn.Module):
        raise TypeError(f"{name}: {type(model).__name__} is not an nn.Module")
    if any(m.training for m in model.modules()):
        raise ValueError(f"{name} explains the deployed network: call model.eval() first (train-mode BatchNorm would mix the "
                         f"{jobs} of a chunk)")
    if score not in SCORES:
        raise ValueError(f"score must be one of {SCORES}, got {score!r}")
    _int(chunk, "chunk must be a positive integer", 1)
    vols = [v.detach() for v in volumes]
    B = vols[0].shape[0]
    if any(v.dim() < 4 or v.shape[0] != B for v in vols):
        raise ValueError("volumes must be (B, ..., D, H, W) with one batch size")
    return vols, B


class _Pass:
    """The perturbation pass: score the model on perturbed copies of some of its volumes, `chunk` jobs per forward.  Construct
    and use it under torch.no_grad() and _on(vols[0]).  The constructor runs the unperturbed forward ONCE -> logits (B,
    classes), target (B,), base (B,): its score; with `reuse` it keeps the output of every encoder _baseline finds, ordered
    behind the models' side streams.  scores() may then run several times."""

    def __init__(self, model, vols, score, target, output, chunk, reuse):
        self.model, self.vols, self.score, self.output, self.chunk = model, vols, score, output, chunk
        self.logits, self.encoders = _baseline(model, vols, output, reuse)
        self.target = _resolve_target(target, self.logits)
        self.base = _score(self.logits, self.target, score)
        self.sides = _join_side_streams(self.logits, [out for encs in self.encoders.values() for _enc, out in encs])

    def scores(self, perturbed, jobs, write, buffered=()):
        """-> (B * jobs,): the score of job j = b*jobs + w, sample b under perturbation w of the volume arguments `perturbed`.
        Per chunk of K jobs from j0 the batch is: write(i, j0, K, out) -> (K, ...) for volume i in `perturbed` (out: K rows of
        a buffer allocated once per call for i in `buffered`, else None); a zero-stride expand for a volume whose encoders all
        replay their kept output (sNet.tmf_replay, taken off again also when the model raises); the samples' rows otherwise."""
        vols, chunk, dev = self.vols, self.chunk, self.logits.device
        n = vols[0].shape[0] * jobs
        kept = [e for i, encs in self.encoders.items() if i not in perturbed for e in encs]
        replayed = {i for i in self.encoders if i not in perturbed}
        bufs = {i: torch.empty((min(chunk, n),) + tuple(vols[i].shape[1:]), device=vols[i].device, dtype=vols[i].dtype)
                for i in buffered}
        scores = torch.empty((n,), device=dev, dtype=self.logits.dtype)
        with _Replay(kept) as replay:
            for j0 in range(0, n, chunk):
                K = min(chunk, n - j0)
                rows = torch.arange(j0, j0 + K, device=dev) // jobs
                batch = []
                for i, v in enumerate(vols):
                    if i in perturbed:
                        batch.append(write(i, j0, K, bufs[i][:K] if i in bufs else None))
                    elif i in replayed:
                        batch.append(v[:1].expand(K, *v.shape[1:]))        # not read: its encoder replays
                    else:
                        batch.append(v.index_select(0, rows.to(v.device)))
                replay.set(rows)
                out = _logits(self.model, batch, self.output)
                scores[j0:j0 + K] = _score(out, self.target.index_select(0, rows), self.score)
        for buf in bufs.values():
            for s in self.sides:
                buf.record_stream(s)
        return scores
