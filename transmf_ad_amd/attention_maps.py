"""What the cross-modal fusion block attends to: the attention maps of every Transformer instance.

    from transmf_ad_amd import attention_maps
    maps = attention_maps(model.eval(), mri, pet)          # model_ad, model_transformer, anything with a CrossTransformer_MOD_AVG
    maps.received[l, 0]                                    # (B, heads, N): how much each PET token is attended to by the MRI stream
    maps.received[l, 1]                                    # ... each MRI token by the PET stream (on the layer's new MRI tokens)
    vol = maps.volume(layer=-1, direction=0)               # (B, D, H, W): that map on the token grid, resampled to the volumes

received[l, s, b, h, j] = (1/N) sum_i P[l, s, b, h, i, j], the mean over the queries of the softmax the reference builds and
drops (networks.py:169-173); probs=True returns P itself.  The model's own forward runs once and yields `logits`; a forward
pre-hook on `fuse_transformer` hands over the tokens it was given, and a second pass over the fusion block (one library call,
tmf_fusion_attn_maps: one launch per op with tmf_xattn_probs after every attention) rebuilds the maps from the attention's
log-sum-exp.  The model must be in eval mode: with Dropout active the second pass would draw other masks than the forward
that produced `logits`.

attention_maps_torch is the same result from the formula in plain torch ops: CPU tensors, dtypes other than float32 and
geometries the one-call entry refuses (ops.fusion_one_call_supported) take it; attention_maps itself routes them there."""
import torch
import torch.nn.functional as F

from . import networks, ops
from ._explain import _trilinear

__all__ = ["attention_maps", "attention_maps_torch", "AttentionMaps", "token_grid"]


def token_grid(size):
    """The token grid (d, h, w) of a volume of spatial `size`: every side halved four times with floor (the four pooled
    blocks of sNet)."""
    return tuple(int(s) // 2 // 2 // 2 // 2 for s in size)


class AttentionMaps:
    """logits: output 0 of the model's forward (None when only tokens were given); received: (depth, 2, B, heads, N);
    probs: (depth, 2, B, heads, N, N) or None; grid: the token grid (d, h, w) or None; size: the volumes' spatial shape."""

    def __init__(self, logits, received, probs, grid, size):
        self.logits, self.received, self.probs, self.grid, self.size = logits, received, probs, grid, size

    def volume(self, layer=-1, direction=0, heads="mean", size=None):
        """received[layer, direction] on the token grid, resampled to `size` (default: the input volumes' shape) by trilinear
        interpolation (align_corners=False) -> (B, *size) for heads="mean" (the mean over the heads) or one head index,
        (B, heads, *size) for heads=None."""
        if self.grid is None:
            raise ValueError("these maps were computed from tokens alone: no token grid to lay them out on")
        r = self.received[layer, direction]                       # (B, heads, N)
        if heads == "mean":
            r = r.mean(1, keepdim=True)
        elif heads is not None:
            r = r[:, int(heads)].unsqueeze(1)
        vol = _trilinear(r.reshape(r.shape[0], r.shape[1], *self.grid), size, self.size)
        return vol if heads is None else vol[:, 0]


def _fusion_of(model):
    ft = model if isinstance(model, (networks.CrossTransformer_MOD_AVG, networks.CrossTransformer)) \
        else getattr(model, "fuse_transformer", None)
    if isinstance(ft, networks.CrossTransformer):
        raise NotImplementedError(
            f"attention_maps: {type(ft).__name__} (two-part contexts) is not wired up at the model level; the kernel entry "
            "(ops.xattn_probs with kv2) takes its contexts")
    if not isinstance(ft, networks.CrossTransformer_MOD_AVG):
        raise TypeError(f"attention_maps: {type(model).__name__} has no CrossTransformer_MOD_AVG as fuse_transformer")
    return ft


def _instance_torch(tr, x, ctx, want_probs):
    """One Transformer(depth=1) instance (networks.py:215-230) in plain torch ops, eval mode -> (y, recv, probs or None)."""
    (pa, pf), = tr.layers
    at, ff = pa.fn, pf.fn
    dim = x.shape[-1]
    q = F.linear(F.layer_norm(x, (dim,), pa.norm.weight, pa.norm.bias, pa.norm.eps), at.to_q.weight)
    k, v = F.linear(ctx, at.to_kv.weight).chunk(2, dim=-1)
    B, N, inner = q.shape
    split = lambda t: t.reshape(B, t.shape[1], at.heads, inner // at.heads).transpose(1, 2)
    P = (torch.einsum("bhid,bhjd->bhij", split(q), split(k)) * at.scale).softmax(dim=-1)
    out = torch.einsum("bhij,bhjd->bhid", P, split(v)).transpose(1, 2).reshape(B, N, inner)
    x1 = F.linear(out, at.to_out[0].weight, at.to_out[0].bias) + x
    hdn = F.gelu(F.linear(F.layer_norm(x1, (dim,), pf.norm.weight, pf.norm.bias, pf.norm.eps), ff.net[0].weight, ff.net[0].bias))
    x2 = F.linear(hdn, ff.net[3].weight, ff.net[3].bias) + x1
    return F.layer_norm(x2, (dim,), tr.norm.weight, tr.norm.bias, tr.norm.eps), P.mean(dim=2), (P if want_probs else None)


def _maps_torch(ft, mri_tok, pet_tok, want_probs):
    """-> (received (depth, 2, B, heads, N), probs (depth, 2, B, heads, N, N) or None) of CrossTransformer_MOD_AVG's forward
    (networks.py:272-276) on these tokens."""
    recv, probs = [], []
    for mri_enc, pet_enc in ft.layers:
        if len(mri_enc.layers) != 1 or len(pet_enc.layers) != 1:
            raise NotImplementedError("attention_maps: Transformer instances of depth 1 only")
        y, r0, p0 = _instance_torch(mri_enc, mri_tok, pet_tok, want_probs)
        mri_tok = y + mri_tok
        y, r1, p1 = _instance_torch(pet_enc, pet_tok, mri_tok, want_probs)
        pet_tok = y + pet_tok
        recv.append(torch.stack([r0, r1]))
        probs.append(torch.stack([p0, p1]) if want_probs else None)
    if not recv:
        raise ValueError("attention_maps: the fusion block has no layers")
    return torch.stack(recv), (torch.stack(probs) if want_probs else None)


def _device_ok(ft, mri_tok, pet_tok):
    """The one-call entry takes these tokens: float32 on a HIP device, the geometry and the module state the one-call
    forward asks for (CrossTransformer_MOD_AVG._one_call_geometry_ok)."""
    return (ops.FUSION_ONE_CALL and mri_tok.is_cuda and mri_tok.dtype == torch.float32 and pet_tok.dtype == torch.float32
            and pet_tok.shape == mri_tok.shape and len(ft.layers) > 0 and ft._one_call_geometry_ok(mri_tok))


def _run(model, mri, pet, want_probs, torch_only):
    ft = _fusion_of(model)
    if model.training or ft.training:
        raise ValueError("attention_maps: the model must be in eval mode (model.eval()): with Dropout active the maps would "
                         "be those of other masks than the forward that produced the logits")
    with torch.no_grad():
        if mri.dim() == 3:                                  # tokens (B, N, dim) for the fusion block itself
            logits, grid, size = None, None, None
            mri_tok, pet_tok = mri, pet
        else:
            size = tuple(mri.shape[-3:])
            grid = token_grid(size)
            seen = []
            hook = ft.register_forward_pre_hook(lambda _m, args: seen.append(args))
            try:
                out = model(mri, pet)
            finally:
                hook.remove()
            logits = out[0] if isinstance(out, (tuple, list)) else out
            if len(seen) != 1:
                raise RuntimeError(f"attention_maps: the model called its fusion block {len(seen)} times in one forward")
            mri_tok, pet_tok = seen[0]
            if grid[0] * grid[1] * grid[2] != mri_tok.shape[1]:
                raise ValueError(f"attention_maps: the token grid {grid} of volumes {size} does not hold the fusion block's "
                                 f"{mri_tok.shape[1]} tokens")
        if not torch_only and _device_ok(ft, mri_tok, pet_tok):
            cfg, params = ft._one_call_args()
            _cls, recv, probs = ops.fusion_attn_maps(mri_tok, pet_tok, cfg, params, want_probs)
            B, N = mri_tok.shape[:2]
            depth, heads = len(ft.layers), cfg[0]
            recv = recv.view(depth, 2, B, heads, N)
            probs = probs.view(depth, 2, B, heads, N, N) if want_probs else None
        else:
            recv, probs = _maps_torch(ft, mri_tok, pet_tok, want_probs)
    return AttentionMaps(logits, recv, probs, grid, size)


def attention_maps(model, mri, pet, probs=False):
    """The attention maps of `model`'s fusion block on the volumes mri, pet (B, 1, D, H, W) -> AttentionMaps(logits, received,
    probs, grid).  Runs under torch.no_grad(); the caller's tensors, the parameters and the buffers are not modified.  Raises
    ValueError for a model in train mode, NotImplementedError for a networks.CrossTransformer (model_transformer_res)."""
    return _run(model, mri, pet, bool(probs), torch_only=False)


def attention_maps_torch(model, mri, pet, probs=False):
    """attention_maps by the formula in plain torch ops, on whatever device and dtype the tensors and parameters have.
    mri, pet: the volumes, or the (B, N, dim) tokens the fusion block receives (`model` may then be the
    CrossTransformer_MOD_AVG itself; logits and grid are None)."""
    return _run(model, mri, pet, bool(probs), torch_only=True)
