"""Which voxels carry a prediction, by random masking: RISE (Petsiuk et al., 2018), the black-box member of the explanation
family at voxel resolution.

    from transmf_ad_amd import rise
    r = rise(model.eval(), mri, pet, masks=2000, cells=8)               # or p=0.5, seed=0, baseline="blur", halves=True
    r.map(0)                                                            # (B, D, H, W): the map of the MRI volume
    r.scores(0)                                                         # (B, N): the score under every mask
    r.split_half(0)                                                     # (B,): do the even and the odd masks agree?
    r.logits, r.target, r.base_score, r.cells, r.cell, r.p, r.seed, r.masks

Semantics (include/tmf_hip.h states the same for the kernels):
  Geometry.  Per axis with extent S and s cells, 1 <= s <= S: cell size c = ceil(S / s), n = s + 2 nodes.  Mask m owns a node
    grid of n_d * n_h * n_w bytes, each 1 with probability p, and a shift t with 0 <= t_a < c_a; its value at a voxel is the
    trilinear interpolation of the eight nodes around (v + t) / c - W first, then H, then D, every operation rounded on its own.
    E[M(v)] = p for every voxel.
  Nodes and shifts.  Philox4x32-10 keyed by `seed`: a pure function of (seed, m, geometry, p), independent of the number of
    masks, of the chunking and of the call.  torch's generator is not touched.
  Jobs.  Job j = b*N + m is sample b under mask m - the masks are shared by the samples -: f + M * (vol - f) with
    f = baseline[b, voxel] where `baseline` (a tensor of the volume's shape, or "blur": the volume smoothed with
    smooth.BLUR_SIGMA voxels) is given, else fill[b] (a float, "mean" or a tensor (B,)).  fill 0 is the paper's M * vol.
  Score.  "prob" (the default, the paper's): the softmax probability of the target class; "logit": its logit.  target as
    saliency.input_gradients (None: the argmax of the unmasked logits, resolved once).
  Map.  map[b, v] = scale * sum_m score[b, m] * M_m(v), an fp32 chain in ascending m.  normalize="expected": scale = 1 / (N p);
    normalize="coverage": the sum divided by coverage[v] = sum_m M_m(v) (one more accumulate call with scores of ones), 0 where
    the coverage is 0.  halves=True also accumulates the even and the odd masks on their own (each with its own N / 2 or
    coverage): split_half is their Pearson correlation per sample - near 1 where N was enough.
  Model mode.  The model must be in eval mode (ValueError otherwise).  Everything runs under torch.no_grad(); the caller's
    tensors, the parameters' .grad, the buffers and torch's generator stay untouched.

`volumes`, joint, chunk and reuse work as in occlusion_sensitivity: per masked volume the jobs are walked in chunks of
`chunk`, ONE launch (tmf_rise_apply, csrc/rise.hip) writes the chunk's masked volumes into a buffer allocated once straight
from the node bytes, the encoders of the untouched volumes replay their kept output, one model(...) call runs.  ONE more
launch per map (tmf_rise_accumulate) rebuilds every mask in registers and adds it up: no full-resolution mask is ever stored.

rise_torch is the same function on the stock-torch twins (ops.rise_apply_torch, ops.rise_accumulate_torch), on any device and
dtype and any nn.Module; tmf_replay is not used there."""
import torch

from . import ops, smooth
from ._explain import SCORES, _fill, _is_int, _on, _pass_arguments, _Pass

__all__ = ["rise", "rise_torch", "Rise", "SCORES"]

NORMALIZE = ("expected", "coverage")


class Rise:
    """logits (B, classes): the unmasked forward; target (B,): the class explained; base_score (B,); cells, cell: per axis the
    cells and the cell size in voxels; p, seed, masks (N); volumes: the masked volume arguments' indices; joint; normalize;
    coverage (D, H, W): sum_m M_m, None unless normalize="coverage"."""

    def __init__(self, logits, target, base_score, size, cells, cell, p, seed, masks, volumes, joint, normalize, nodes, shifts,
                 scores, maps, halves, coverage, torch_only):
        self.logits, self.target, self.base_score = logits, target, base_score
        self.size, self.cells, self.cell, self.p, self.seed, self.masks = size, cells, cell, p, seed, masks
        self.volumes, self.joint, self.normalize, self.coverage = volumes, joint, normalize, coverage
        self.nodes, self.shifts = nodes, shifts
        self._scores, self._maps, self._halves, self._torch_only = scores, maps, halves, torch_only

    def _key(self, volume):
        if self.joint and (volume is None or volume in self.volumes):
            return self.volumes[0]
        if volume is None and len(self.volumes) == 1:
            return self.volumes[0]
        if volume not in self._maps:
            raise KeyError(f"no map for volume {volume!r}: masked volume arguments {self.volumes}")
        return volume

    def map(self, volume=None):
        """(B, D, H, W): the saliency map of volume argument `volume` (0 = the first); may be left out where one map was computed."""
        return self._maps[self._key(volume)]

    def scores(self, volume=None):
        """(B, N): the score of sample b under mask m of that volume argument."""
        return self._scores[self._key(volume)]

    def halves(self, volume=None):
        """(even, odd): the maps of masks 0, 2, ... and 1, 3, ..., each (B, D, H, W); needs halves=True."""
        if self._halves is None:
            raise ValueError("the half maps were not computed: call rise(..., halves=True)")
        return self._halves[self._key(volume)]

    def split_half(self, volume=None):
        """(B,): the Pearson correlation of the two half maps over the voxels; 0 where one of them is constant."""
        even, odd = (h.reshape(h.shape[0], -1).double() for h in self.halves(volume))
        even, odd = even - even.mean(1, keepdim=True), odd - odd.mean(1, keepdim=True)
        den = even.norm(dim=1) * odd.norm(dim=1)
        r = (even * odd).sum(1) / den.clamp_min(torch.finfo(torch.float64).tiny)
        return torch.where(den > 0, r, torch.zeros_like(r)).to(self.logits.dtype)

    def mask(self, m):
        """(D, H, W): mask m on the voxel grid, the values the kernels rebuild."""
        if not _is_int(m) or not 0 <= m < self.masks:
            raise ValueError(f"mask {m!r} outside 0..{self.masks - 1}")
        return ops.rise_mask_values(self.nodes[m:m + 1], self.shifts[m:m + 1], self.size, self.cells)[0]


def _run(model, volumes, masks, cells, p, seed, fill, baseline, score, target, output, which, joint, chunk, reuse, normalize,
         halves, torch_only):
    vols, B = _pass_arguments("rise", "masks", model, volumes, score, chunk)
    which = tuple(range(len(vols))) if which is None else (which,) if isinstance(which, int) else tuple(which)
    if not which or any(not _is_int(i) or not 0 <= i < len(vols) for i in which) or len(set(which)) != len(which):
        raise ValueError(f"volumes must name some of the {len(vols)} volume arguments once each, got {which!r}")
    size = tuple(int(s) for s in vols[which[0]].shape[-3:])
    if any(tuple(vols[i].shape[-3:]) != size or vols[i].numel() != B * size[0] * size[1] * size[2] for i in which):
        raise ValueError("the masked volumes must be one-channel volumes of one spatial shape")
    if normalize not in NORMALIZE:
        raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
    N = masks
    if not _is_int(N) or N < (2 if halves else 1):
        raise ValueError(f"masks must be an integer >= {2 if halves else 1}, got {masks!r}")
    cell, _nodes, _G = ops.rise_geometry(size, cells)                  # ValueError for cells outside 1..S
    cells = tuple(cells) if isinstance(cells, (tuple, list)) else (cells,) * 3
    if not isinstance(p, (int, float)) or isinstance(p, bool) or not 0.0 < float(p) < 1.0:
        raise ValueError(f"p must lie in (0, 1), got {p!r}")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    bases, fills = {}, {}
    for i in which:
        v = vols[i]
        bases[i] = None
        if isinstance(baseline, str):
            if baseline != "blur":
                raise ValueError(f"baseline must be a tensor of the volume's shape {tuple(v.shape)} or \"blur\", got {baseline!r}")
            bases[i] = (smooth.gaussian_smooth_torch if torch_only else smooth.gaussian_smooth)(v, sigma=smooth.BLUR_SIGMA).contiguous()
        elif baseline is not None:
            if not torch.is_tensor(baseline) or tuple(baseline.shape) != tuple(v.shape):
                raise ValueError(f"baseline must be a tensor of the volume's shape {tuple(v.shape)} or \"blur\"")
            bases[i] = baseline.detach().to(device=v.device, dtype=v.dtype).contiguous()
        fills[i] = _fill(fill, v, B)
    apply, accumulate = (ops.rise_apply_torch, ops.rise_accumulate_torch) if torch_only else (ops.rise_apply, ops.rise_accumulate)
    first = vols[which[0]]

    with torch.no_grad(), _on(vols[0]):
        nodes, shifts = (ops.rise_masks_torch if torch_only else ops.rise_masks)(size, cells, p, seed, 0, N, first.device)
        run = _Pass(model, vols, score, target, output, chunk, reuse)
        write = lambda i, j0, K, out: apply(vols[i], nodes, shifts, fills[i], size, cells, j0, K, base=bases[i], out=out)

        def build(scores, m_first, m_step):
            n = len(range(m_first, N, m_step))
            if normalize == "expected":
                return accumulate(scores, nodes, shifts, size, cells, 1.0 / (n * float(p)), m_first, m_step), None
            cover = accumulate(torch.ones((1, N), device=scores.device, dtype=scores.dtype), nodes, shifts, size, cells, 1.0,
                               m_first, m_step)
            total = accumulate(scores, nodes, shifts, size, cells, 1.0, m_first, m_step)
            return torch.where(cover > 0, total / cover, torch.zeros((), device=total.device, dtype=total.dtype)), cover[0]

        scores, maps, half_maps, coverage = {}, {}, {}, None
        for masked in ([which] if joint else [(i,) for i in which]):
            # the chunk buffers of the kernel path, allocated once per pass (the torch ops allocate as they go)
            buffered = [i for i in masked
                        if not torch_only and ops.rise_ok(vols[i], nodes, shifts, bases[i] if bases[i] is not None else fills[i])]
            s = run.scores(masked, N, write, buffered).view(B, N).contiguous()
            sal, cover = build(s, 0, 1)
            coverage = cover if coverage is None else coverage
            both = (build(s, 0, 2)[0], build(s, 1, 2)[0]) if halves else None
            for i in (masked[:1] if joint else masked):
                scores[i], maps[i] = s, sal
                if halves:
                    half_maps[i] = both
    return Rise(run.logits, run.target, run.base, size, cells, cell, float(p), seed, N, which, bool(joint), normalize, nodes,
                shifts, scores, maps, half_maps if halves else None, coverage, torch_only)


def rise(model, *vols, masks=2000, cells=8, p=0.5, seed=0, fill=0.0, baseline=None, score="prob", target=None, output=0,
         volumes=None, joint=False, chunk=32, reuse=True, normalize="expected", halves=False):
    """RISE saliency of `model` (eval mode) on the volumes (B, 1, D, H, W) -> Rise.  See the module docstring for the geometry,
    masks, fill / baseline, score, target, `volumes`, joint, chunk, reuse, normalize and halves.  ValueError for a model in
    train mode, cells outside 1..S, p outside (0, 1), masks < 1 (< 2 with halves), a bad normalize, baseline, fill, score or
    volume index."""
    return _run(model, vols, masks, cells, p, seed, fill, baseline, score, target, output, volumes, bool(joint), chunk,
                bool(reuse), normalize, bool(halves), False)


def rise_torch(model, *vols, masks=2000, cells=8, p=0.5, seed=0, fill=0.0, baseline=None, score="prob", target=None, output=0,
               volumes=None, joint=False, chunk=32, reuse=False, normalize="expected", halves=False):
    """rise on the stock-torch twins: any device, dtype and nn.Module.  `reuse` is accepted and ignored: tmf_replay is not used
    here."""
    return _run(model, vols, masks, cells, p, seed, fill, baseline, score, target, output, volumes, bool(joint), chunk, False,
                normalize, bool(halves), True)
