"""Which explanation to believe for a scan: deletion / insertion curves (Petsiuk et al., RISE, 2018), the quantitative check on
input_gradients, attention_maps, grad_cam and occlusion_sensitivity.

    from transmf_ad_amd import faithfulness_curve
    fc = faithfulness_curve(model.eval(), mri, pet, attribution=a, volume=0, steps=20, mode="deletion")
    fc.scores       # (B, steps+1): the class score with the top 0, n_1, .. n_steps voxels of the attribution blanked
    fc.auc          # (B,): the area under it on the nominal grid k / steps; low is good for deletion, high for insertion
    fc.removed      # (B, steps+1) int32: the voxels really blanked (revealed) at each step, column 0 is 0
    fc.thresholds   # (B, steps)
    fc.logits, fc.target, fc.base_score, fc.steps, fc.mode, fc.volume

Semantics (include/tmf_hip.h states the same for the kernels):
  Attribution.  `attribution` (B, D, H, W) or (B, 1, D, H, W) holds one value per voxel of volume argument `volume` (0 = the
    first): |input gradient|, a Grad-CAM map the caller upsampled, occ.volume(i), ...  Voxels are ordered by a = attribution
    + 0.0 (-0.0 ranks with +0.0), compared as floats in the attribution's own dtype; infinities are ordinary values.  NaN
    raises ValueError: this is ONE host read (a device synchronisation) before the pass.
  Steps.  n_k = ceil(k*V / steps), k = 1..steps (ops.rank_counts); thresholds[b, k-1] = the n_k-th largest a of sample b.
    Step k masks every voxel with a >= that threshold: ties go together, there is no tie-break by index, so
    removed[b, k] >= n_k with equality where the values are distinct, and equal steps repeat (V < steps, plateaus).
  Jobs.  Job j = b*(steps+1) + s, s = 0..steps; s = 0 masks nothing and runs like every other job.  mode "deletion": the
    masked voxels are replaced by f, the others keep the volume.  mode "insertion": the masked voxels show the volume, the
    others f.  f = baseline[b, voxel] where `baseline` (a tensor of the volume's shape, e.g. a blurred copy) is given, else
    fill[b]: a float (default 0.0), "mean" (the sample's mean) or a tensor (B,), as in occlusion_sensitivity.
    baseline="blur": the masked volume smoothed with smooth.BLUR_SIGMA voxels in reflect mode (RISE's insertion baseline),
    the same tensor as baseline=gaussian_smooth(vol, sigma=BLUR_SIGMA); for another sigma pass that tensor.
  Score.  "prob" (default): the softmax probability of class target_b; "logit": logits[b, target_b].  target as
    saliency.input_gradients (None: the argmax of the UNMASKED logits, resolved once).  base_score is that forward's score.
  AUC.  auc = (s_0/2 + s_1 + .. + s_{S-1} + s_S/2) / S by torch ops; `removed` lets a caller integrate over the true
    fractions removed / V where ties make the steps uneven.
  Model mode.  The model must be in eval mode (ValueError otherwise: train-mode BatchNorm would mix the jobs of a chunk).
    Everything runs under torch.no_grad(); the caller's tensors, the parameters' .grad, the buffers and torch's generator stay
    untouched.

The thresholds come from ONE call (ops.rank_thresholds: tmf_rank_thresholds, csrc/faithfulness.hip, a radix select without a
sort).  The jobs are walked in chunks of `chunk`: ONE launch (ops.mask_by_rank: tmf_mask_by_rank) writes the chunk's masked
volumes into a buffer allocated once, one model(...) call runs, the scores come from the (K, classes) logits by torch ops.

reuse=True is the machinery occlusion uses (_explain._baseline, _explain._Replay): every networks.sNet of a package
model that ran once in the unmasked forward, on a volume argument other than `volume`, keeps its output and replays it
through sNet.tmf_replay for the pass, taken off again also when the model raises.

faithfulness_curve_torch is the same function on sort(descending=True), a gather, >= and torch.where, on any device and
dtype and any nn.Module (the reference's classes on the CPU in float or double); tmf_replay is not used there."""
import torch

from . import ops, smooth
from ._explain import _attribution, _fill, _int, _on, _pass_arguments, _Pass

__all__ = ["faithfulness_curve", "faithfulness_curve_torch", "Faithfulness", "MODES"]

MODES = tuple(ops.RANK_MODES)


class Faithfulness:
    """scores (B, steps+1), auc (B,), removed (B, steps+1) int32, thresholds (B, steps); logits (B, classes): the unmasked
    forward; target (B,): the class scored; base_score (B,); steps, mode, volume."""

    def __init__(self, scores, auc, removed, thresholds, logits, target, base_score, steps, mode, volume):
        self.scores, self.auc, self.removed, self.thresholds = scores, auc, removed, thresholds
        self.logits, self.target, self.base_score = logits, target, base_score
        self.steps, self.mode, self.volume = steps, mode, volume


def _run(model, volumes, attribution, volume, steps, mode, fill, baseline, score, target, output, chunk, reuse, torch_only):
    vols, B = _pass_arguments("faithfulness_curve", "jobs", model, volumes, score, chunk)
    if mode not in MODES:
        raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
    S = _int(steps, "steps must be an integer in 1..64", 1, 64)
    v = vols[_int(volume, f"volume must name one of the {len(vols)} volume arguments", 0, len(vols) - 1)]
    size = tuple(int(s) for s in v.shape[-3:])
    V = size[0] * size[1] * size[2]
    if B < 1 or V < 1 or v.numel() != B * V:
        raise ValueError("the masked volume must be a one-channel volume (B, 1, D, H, W) with voxels")
    attr = _attribution(attribution, (B,) + size).to(v.device).contiguous()
    if bool(torch.isnan(attr).any()):                                   # the one host read
        raise ValueError("attribution holds NaN: voxels cannot be ranked")
    base_vol = None
    if isinstance(baseline, str):
        if baseline != "blur":
            raise ValueError(f"baseline must be a tensor of the volume's shape {tuple(v.shape)} or \"blur\", got {baseline!r}")
        base_vol = (smooth.gaussian_smooth_torch if torch_only else smooth.gaussian_smooth)(v, sigma=smooth.BLUR_SIGMA).contiguous()
    elif baseline is not None:
        if not torch.is_tensor(baseline) or tuple(baseline.shape) != tuple(v.shape):
            raise ValueError(f"baseline must be a tensor of the volume's shape {tuple(v.shape)}")
        base_vol = baseline.detach().to(device=v.device, dtype=v.dtype).contiguous()
    fills = _fill(fill, v, B)
    counts = ops.rank_counts(V, S)
    thresholds, mask = (ops.rank_thresholds_torch, ops.mask_by_rank_torch) if torch_only else (ops.rank_thresholds, ops.mask_by_rank)

    with torch.no_grad(), _on(vols[0]):
        run = _Pass(model, vols, score, target, output, chunk, reuse)
        thr, removed = thresholds(attr, counts)
        # the chunk buffer of the kernel path, allocated once per pass (the torch ops allocate as they go)
        buffered = not torch_only and ops.faithfulness_ok(v, attr, thr, base_vol if base_vol is not None else fills)
        masked = lambda _i, j0, K, out: mask(v, attr, thr, fills, mode, j0, K, base=base_vol, out=out)
        scores = run.scores((volume,), S + 1, masked, (volume,) if buffered else ()).view(B, S + 1)
        auc = (scores[:, 0] / 2 + scores[:, 1:S].sum(1) + scores[:, S] / 2) / S
        removed = torch.cat([torch.zeros((B, 1), device=removed.device, dtype=removed.dtype), removed], 1)
    return Faithfulness(scores, auc, removed, thr, run.logits, run.target, run.base, S, mode, volume)


def faithfulness_curve(model, *vols, attribution, volume=0, steps=20, mode="deletion", fill=0.0, baseline=None, score="prob",
                       target=None, output=0, chunk=32, reuse=True):
    """The deletion or insertion curve of `attribution` for volume argument `volume` of `model` (eval mode) -> Faithfulness.
    See the module docstring for the ordering, steps, jobs, fill / baseline, score, target, chunk and reuse.  ValueError for
    a model in train mode, steps outside 1..64, a bad mode, score, volume, fill, baseline or attribution shape, and an
    attribution that holds NaN (one host read before the pass)."""
    return _run(model, vols, attribution, volume, steps, mode, fill, baseline, score, target, output, chunk, bool(reuse), False)


def faithfulness_curve_torch(model, *vols, attribution, volume=0, steps=20, mode="deletion", fill=0.0, baseline=None,
                             score="prob", target=None, output=0, chunk=32, reuse=False):
    """faithfulness_curve on sort(descending=True), a gather, >= and torch.where: any device, dtype and nn.Module.  `reuse` is
    accepted and ignored: tmf_replay is not used here."""
    return _run(model, vols, attribution, volume, steps, mode, fill, baseline, score, target, output, chunk, False, True)
