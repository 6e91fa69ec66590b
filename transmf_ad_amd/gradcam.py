"""Which part of an encoder's feature maps carries a prediction: Grad-CAM and HiResCAM at any block of every sNet.

    from transmf_ad_amd import grad_cam
    cams = grad_cam(model.eval(), mri, pet, layer="conv3")          # or layer=("conv2", "conv3"); method="hirescam"
    cams.encoders                                                   # ("mri_cnn", "pet_cnn"): every sNet under the model
    cams.map("mri_cnn", "conv3")                                    # (B, d, h, w) on the block's own grid
    cams.weights("mri_cnn", "conv3")                                # (B, C): Grad-CAM's channel weights
    cams.volume("pet_cnn", "conv3")                                 # (B, D, H, W): that map resampled to the volumes

With A (B, d, h, w, C) the output of a block and G = d sum_b logits[b, target_b] / d A:
    "gradcam":  w[b, c] = mean over the voxels of G[b, ..., c],  map[b, v] = sum_c w[b, c] A[b, v, c]
    "hirescam": map[b, v] = sum_c G[b, v, c] A[b, v, c]                 (no pooling of the gradient)
relu clamps the map at 0, normalize divides each sample's map by its maximum (a sample whose maximum is <= 0 gives zeros).

Layers carry the reference's module paths under an encoder (networks.sNet.TAP_LAYERS): "conv1", "conv2", "conv3", "conv4" are
the outputs of the four Sequentials (after their pool), "conv2.2", "conv3.2", "conv4.2" the LeakyReLU output of the first block
of a Sequential.  The blocks that end in a pool are fused with it and never store their pre-pool activations, so those are not
offered.

One call runs ONE forward of the model under enable_grad with a tap on every encoder (sNet.tmf_tap, removed again also when the
model raises; the encoders then run block by block, bit-identical to their one-call paths), ONE torch.autograd.grad of the score
with respect to the tapped tensors, and one library call per (encoder, layer): tmf_cam of csrc/cam.hip reads A and G once each.
Taps that are not float32 tensors on a HIP device (bf16 activation storage) or whose channel count tmf_cam does not take go to
the same formula in torch ops after an upcast.  Parameters are frozen for the duration (no weight gradient is computed, their
.grad is not touched, requires_grad is restored); the caller's tensors are not modified and keep no graph.

The mode of the model is the caller's, and so are its side effects: the forward of a model in train mode updates the BatchNorm
running statistics and num_batches_tracked and draws Dropout masks from torch's generator.  Call model.eval() first for an
explanation of the deployed network that leaves its buffers alone.

grad_cam_torch is the same function with the map arithmetic in plain torch ops on whatever device and dtype the tensors have.
It also takes modules that are not this package's — the reference's classes on the CPU, in float or double: every sub-module
with conv1 ... conv4 Sequentials counts as an encoder and is tapped with ordinary forward hooks on those Sequentials and their
[2] children."""
import torch
from torch import nn

from . import networks, ops
from ._explain import _check, _Frozen, _join_side_streams, _logits, _on, _resolve_target, _trilinear

__all__ = ["grad_cam", "grad_cam_torch", "GradCams", "LAYERS", "METHODS"]

LAYERS = tuple(networks.sNet.TAP_LAYERS)
METHODS = ("gradcam", "hirescam")


def cam_torch(act, grad, method="gradcam", relu=True, normalize=True):
    """The map arithmetic in torch ops on channels-last act, grad (B, ..., C) -> (map (B, ...), weights (B, C) or None, peak (B,))."""
    B, C = act.shape[0], act.shape[-1]
    ones = (1,) * (act.dim() - 2)
    if method == "gradcam":
        weights = grad.reshape(B, -1, C).mean(1)
        cam = (act * weights.view(B, *ones, C)).sum(-1)
    else:
        weights = None
        cam = (act * grad).sum(-1)
    if relu:
        cam = cam.relu()
    peak = cam.reshape(B, -1).amax(1)
    if normalize:
        p = peak.view(B, *ones)
        cam = torch.where(p > 0, cam / torch.where(p > 0, p, torch.ones_like(p)), torch.zeros_like(cam))
    return cam, weights, peak


class GradCams:
    """encoders: the tapped encoders' module paths, in module order; layers: the layer names asked for; logits: the forward's
    logits (detached); target: the class explained per sample; size: the volumes' spatial shape; method: "gradcam" | "hirescam"."""

    def __init__(self, encoders, layers, method, logits, target, size, maps, weights, peaks):
        self.encoders, self.layers, self.method = tuple(encoders), tuple(layers), method
        self.logits, self.target, self.size = logits, target, size
        self._maps, self._weights, self._peaks = maps, weights, peaks

    def _key(self, encoder, layer):
        if encoder is None and len(self.encoders) == 1:
            encoder = self.encoders[0]
        if layer is None and len(self.layers) == 1:
            layer = self.layers[0]
        if (encoder, layer) not in self._maps:
            raise KeyError(f"no map for encoder {encoder!r}, layer {layer!r}: encoders {self.encoders}, layers {self.layers}")
        return encoder, layer

    def map(self, encoder=None, layer=None):
        """(B, d, h, w): the map on the block's grid.  encoder / layer may be left out where only one was computed."""
        return self._maps[self._key(encoder, layer)]

    def weights(self, encoder=None, layer=None):
        """(B, C): Grad-CAM's channel weights; None for "hirescam"."""
        return self._weights[self._key(encoder, layer)]

    def peak(self, encoder=None, layer=None):
        """(B,): each sample's maximum of the map before the division by it."""
        return self._peaks[self._key(encoder, layer)]

    def volume(self, encoder=None, layer=None, size=None):
        """The map resampled to `size` (default: the input volumes' shape) by trilinear interpolation, align_corners=False
        -> (B, *size)."""
        return _trilinear(self.map(encoder, layer).unsqueeze(1), size, self.size)[:, 0]


def resolve_layers(layer):
    """layer: one name or a sequence of names -> tuple of names, each in LAYERS and once (ValueError otherwise)."""
    names = (layer,) if isinstance(layer, str) else tuple(layer) if isinstance(layer, (tuple, list)) else None
    if not names or any(not isinstance(n, str) or n not in networks.sNet.TAP_LAYERS for n in names):
        raise ValueError(f"layer must be one of {LAYERS} or a sequence of them, got {layer!r}")
    return tuple(dict.fromkeys(names))


def find_encoders(model, foreign=False):
    """[(module path, module, is the package's sNet)]: every networks.sNet under `model` in module order; with `foreign` and
    none of those, every module that has conv1 ... conv4 Sequentials.  TypeError where there is none."""
    if not isinstance(model, nn.Module):
        raise TypeError(f"grad_cam: {type(model).__name__} is not an nn.Module")
    found = [(name or "encoder", m, True) for name, m in model.named_modules() if isinstance(m, networks.sNet)]
    if not found and foreign:
        found = [(name or "encoder", m, False) for name, m in model.named_modules()
                 if all(isinstance(getattr(m, c, None), nn.Sequential) for c in ("conv1", "conv2", "conv3", "conv4"))]
    if not found:
        raise TypeError(f"grad_cam: {type(model).__name__} has no sNet encoder" +
                        (" and no module with conv1 ... conv4 Sequentials" if foreign else ""))
    return found


class _Taps:
    """The tapped tensors {(encoder, layer): tensor} of one forward: sNet.tmf_tap on the package's encoders (channels-last
    tensors), forward hooks on the others (the modules' own (B, C, d, h, w) outputs: `channels_first` holds their keys);
    everything is taken off again on exit."""

    def __init__(self, encoders, layers):
        self.encoders, self.layers, self.seen, self.undo = encoders, layers, {}, []
        self.channels_first = {(name, l) for name, _e, own in encoders if not own for l in layers}

    def _record(self, key, x):
        if key in self.seen:
            raise RuntimeError(f"grad_cam: encoder {key[0]!r} ran more than once in one forward")
        self.seen[key] = x

    def __enter__(self):
        try:
            for name, enc, own in self.encoders:
                if own:
                    wanted = {enc.TAP_LAYERS[l]: l for l in self.layers}
                    before = getattr(enc, "tmf_tap", None)
                    self.undo.append(lambda enc=enc, before=before: setattr(enc, "tmf_tap", before))
                    enc.tmf_tap = lambda n, x, name=name, wanted=wanted: n in wanted and self._record((name, wanted[n]), x)
                else:
                    for l in self.layers:
                        seq, _, child = l.partition(".")
                        mod = getattr(enc, seq)[int(child)] if child else getattr(enc, seq)
                        h = mod.register_forward_hook(lambda _m, _i, out, key=(name, l): self._record(key, out))
                        self.undo.append(h.remove)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        while self.undo:
            self.undo.pop()()
        return False


def _run(model, volumes, layer, method, target, output, relu, normalize, torch_only):
    _check(volumes)
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}, got {method!r}")
    layers = resolve_layers(layer)
    encoders = find_encoders(model, foreign=torch_only)
    leaves = [v.detach().requires_grad_(True) for v in volumes]          # every tapped tensor then carries a graph
    with _Frozen(model, True), _Taps(encoders, layers) as taps, torch.enable_grad():
        logits = _logits(model, leaves, output)
        target = _resolve_target(target, logits)
        keys = [(name, l) for name, _e, _o in encoders for l in layers]
        missing = [k for k in keys if k not in taps.seen]
        if missing:
            raise RuntimeError(f"grad_cam: the forward never reached {missing}")
        acts = [taps.seen[k] for k in keys]
        score = logits.gather(1, target.view(-1, 1)).sum()
        grads = torch.autograd.grad(score, acts, allow_unused=True)
    acts = [a.detach() for a in acts]
    grads = [torch.zeros_like(a) if g is None else g.detach() for g, a in zip(grads, acts)]
    for i, k in enumerate(keys):
        if k in taps.channels_first:
            acts[i], grads[i] = acts[i].permute(0, 2, 3, 4, 1), grads[i].permute(0, 2, 3, 4, 1)
    # the two-encoder models run one encoder (forward and backward) on a side stream: order it ahead of what follows here
    _join_side_streams(logits, acts + grads)
    maps, weights, peaks = {}, {}, {}
    for key, a, g in zip(keys, acts, grads):
        a, g = a.contiguous(), g.contiguous()
        if not torch_only and ops.cam_ok(a, g):
            with _on(a):
                maps[key], weights[key], peaks[key] = ops.cam(a, g, method, relu, normalize)
        else:
            if a.dtype in (torch.bfloat16, torch.float16):
                a, g = a.float(), g.float()
            maps[key], weights[key], peaks[key] = cam_torch(a, g.to(a.dtype), method, relu, normalize)
    return GradCams([name for name, _e, _o in encoders], layers, method, logits.detach(), target, tuple(volumes[0].shape[-3:]),
                    maps, weights, peaks)


def grad_cam(model, *volumes, layer="conv3", method="gradcam", target=None, output=0, relu=True, normalize=True):
    """Class activation maps of `model` on the volumes (B, 1, D, H, W) at `layer` (one of LAYERS or several of them) of every
    networks.sNet under the model -> GradCams.  logits is output number `output` of model(*volumes); target None: each sample's
    argmax class, an int, or one class index per sample (as saliency.input_gradients).  TypeError for a model without an sNet,
    ValueError for an unknown layer or method.  One forward of the model runs: in train mode that updates BatchNorm buffers
    and consumes Dropout random numbers (see the module docstring)."""
    return _run(model, volumes, layer, method, target, output, bool(relu), bool(normalize), torch_only=False)


def grad_cam_torch(model, *volumes, layer="conv3", method="gradcam", target=None, output=0, relu=True, normalize=True):
    """grad_cam with the map arithmetic in plain torch ops; also for modules of other packages whose encoders have conv1 ...
    conv4 Sequentials (forward hooks on them and on their [2] children)."""
    return _run(model, volumes, layer, method, target, output, bool(relu), bool(normalize), torch_only=True)
