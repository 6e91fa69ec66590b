"""Where in the input volumes does a prediction come from: input gradients and integrated gradients.

    from transmf_ad_amd import input_gradients, integrated_gradients
    d_mri, d_pet = input_gradients(model, mri, pet)                    # d logit[argmax] / d volume
    a_mri, a_pet = integrated_gradients(model, mri, pet, steps=16)

Model-agnostic: any module of the package, or any nn.Module that returns the logits or a tuple containing them.  The
derivative with respect to the volumes runs on the library's own kernels — the first encoder block's data gradient
(csrc/conv1_dgrad.hip) never writes the conv output, in eval mode (block by block) as in train mode with batch statistics
(the one-call encoder, tmf_snet_train_bwd_input).

The mode of the model is the caller's, and so are its side effects: every forward of a model in train mode updates the BatchNorm
running statistics and num_batches_tracked and draws Dropout masks from torch's generator.  input_gradients runs one forward,
integrated_gradients steps of them (plus one without a graph when it resolves target=None).  Call model.eval() first for an
explanation of the deployed network that leaves its buffers alone."""
import torch

from ._explain import _check, _Frozen, _int, _logits, _resolve_target
from .smooth import BLUR_SIGMA, gaussian_smooth

__all__ = ["input_gradients", "integrated_gradients"]


def _grads(model, volumes, target, output):
    """(gradients of sum_b logits[b, target_b] with respect to fresh leaves holding the volumes' values, the target used)"""
    leaves = [v.detach().requires_grad_(True) for v in volumes]
    with torch.enable_grad():
        logits = _logits(model, leaves, output)
        target = _resolve_target(target, logits)
        score = logits.gather(1, target.view(-1, 1)).sum()
        grads = torch.autograd.grad(score, leaves, allow_unused=True)
    return tuple(torch.zeros_like(v) if g is None else g.detach() for g, v in zip(grads, leaves)), target


def input_gradients(model, *volumes, target=None, output=0, freeze=True):
    """d sum_b logits[b, target_b] / d volume for every volume -> tuple of tensors shaped like the volumes.

    logits is output number `output` of model(*volumes); target None: each sample's argmax class, an int, or one class index
    per sample.  freeze: no parameter gradient is computed (their requires_grad is switched off and restored, also when the model
    raises).  The caller's tensors are not modified and keep no graph; parameters' .grad is not touched.  One forward of the model
    runs: in train mode that updates BatchNorm buffers and consumes Dropout random numbers (see the module docstring)."""
    _check(volumes)
    with _Frozen(model, freeze):
        return _grads(model, volumes, target, output)[0]


def integrated_gradients(model, *volumes, baselines=None, steps=16, target=None, output=0):
    """(volume - baseline) x the mean input gradient along the straight path from baseline to volume: midpoint rule over `steps`
    points alpha_k = (k + 1/2) / steps, accumulated in fp32 on the device in step order.  baselines None: zeros; "blur": every
    volume's own blurred copy, gaussian_smooth(volume, sigma=smooth.BLUR_SIGMA) (the blurred-input baseline).  target None is
    resolved ONCE, at the volume itself (one more forward, without a graph).  In train mode each of these forwards updates the
    BatchNorm buffers and consumes Dropout random numbers (see the module docstring)."""
    _check(volumes)
    _int(steps, "steps must be a positive integer", 1)
    if baselines is None:
        baselines = tuple(torch.zeros_like(v) for v in volumes)
    elif isinstance(baselines, str):
        if baselines != "blur":
            raise ValueError(f"baselines must be None, \"blur\" or one tensor per volume, got {baselines!r}")
        baselines = tuple(gaussian_smooth(v, sigma=BLUR_SIGMA) for v in volumes)
    elif torch.is_tensor(baselines):
        baselines = (baselines,)
    if len(baselines) != len(volumes) or any(b.shape != v.shape for b, v in zip(baselines, volumes)):
        raise ValueError("one baseline per volume, of the volume's shape")
    vols = [v.detach() for v in volumes]
    bases = [b.detach().to(device=v.device, dtype=v.dtype) for b, v in zip(baselines, vols)]
    with _Frozen(model, True):
        if target is None:
            with torch.no_grad():
                target = _resolve_target(None, _logits(model, vols, output))
        acc = [torch.zeros(v.shape, device=v.device, dtype=torch.float32) for v in vols]
        for k in range(steps):
            alpha = (k + 0.5) / steps
            point = [b + alpha * (v - b) for b, v in zip(bases, vols)]
            grads, _ = _grads(model, point, target, output)
            for a, g in zip(acc, grads):
                a += g.float()
    return tuple(((v - b).float() * (a / steps)).to(v.dtype) for v, b, a in zip(vols, bases, acc))
