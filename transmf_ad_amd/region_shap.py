"""Which atlas region of which modality carries a prediction, when regions can stand in for each other: Shapley values over
the atlas regions of the volumes, the game-theoretic member of the explanation family.

    from transmf_ad_amd import region_shap
    sh = region_shap(model.eval(), mri, pet, atlas=labels, samples=2048)      # or seed=0, baseline="blur", joint=False
    sh.values(0)                                                        # (B, R): the shares of the MRI regions
    sh.volume(1)                                                        # (B, D, H, W): the PET shares on the voxel grid
    sh.phi, sh.delta, sh.base_score, sh.empty_score, sh.ok(), sh.r2(), sh.top(10), sh.table(names)

occlusion_sensitivity(atlas=...) removes one region from the otherwise intact pair; a region whose signal is also present in the
other modality or in a neighbour then shows no drop.  Here the players are the regions of all selected volumes together
(joint=True: P = R * len(volumes), volume number q of `volumes` owns players q*R .. q*R+R-1) and every player gets its share
of delta = score(scan) - score(every region replaced): the shares add up to delta exactly and carry the unit of the score.

Semantics (include/tmf_hip.h states the same for the kernels):
  Estimator.  KernelSHAP (Lundberg & Lee 2017) in the paired-sampling form of Covert & Lee (2021): coalition sizes drawn from
    the Shapley kernel, uniform subsets of that size, every second coalition the complement of the one before it
    (paired=True), an unweighted least-squares fit under the constraint sum(phi) = delta.
  Coalitions.  Philox4x32-10 keyed by `seed`: row m is a pure function of (seed, m, P, paired), independent of `samples`, of the
    chunking and of the call.  torch's generator is not touched.
  Jobs.  Job j = b*(N+1) + m is sample b under coalition m; row N is the empty coalition, its score is v(empty).  A voxel whose
    region is not in the coalition takes baseline[b, voxel] where `baseline` (a tensor of the volume's shape, or "blur") is
    given, else fill[b] (a float, "mean" or a tensor (B,)); background (label 0) is never replaced.
  Fit.  A = sum_m z_m z_m^T (exact integers), rhs_b = sum_m z_m (score[b, m] - v_b(empty)), M = A + ridge I = L L^T in fp64,
    phi_b = x_b - x_1 (sum x_b - delta_b) / sum x_1 with X = M^-1 [rhs, 1].  Too few coalitions for P make A singular: ok() is
    then False and every value NaN; ridge > 0 regularises.
  Model mode.  The model must be in eval mode (ValueError otherwise).  Everything runs under torch.no_grad(); the caller's
    tensors, the parameters' .grad, the buffers and torch's generator stay untouched.  No host read happens before the result
    exists besides the atlas maximum and the checks of an explicit `target`; ok() reads `info` when asked.

`volumes`, chunk and reuse work as in occlusion_sensitivity and rise: the jobs are walked in chunks of `chunk`, ONE launch
(tmf_shap_apply, csrc/shap.hip) writes the chunk's volumes into a buffer allocated once, the encoders of untouched volumes
replay their kept output (joint=False), one model(...) call runs.  Then tmf_shap_gram and tmf_shap_solve.

region_shap_torch is the same function on the stock-torch twins (ops.shap_coalitions_torch, shap_apply_torch, shap_gram_torch,
shap_solve_torch), on any device and dtype and any nn.Module; tmf_replay is not used there."""
import math

import torch

from . import ops, smooth
from ._explain import SCORES, _fill, _int, _is_int, _on, _pass_arguments, _Pass

__all__ = ["region_shap", "region_shap_torch", "RegionShap", "SCORES"]


class _Game:
    """One fitted game: the volume arguments whose regions play, coalitions (N, Wd) int32, scores (B, N), empty (B,), delta (B,)
    float64, A (P, P) int32, phi (B, P) float64, info (1,) int32."""

    def __init__(self, volumes, coalitions, scores, empty, delta, A, phi, info):
        self.volumes, self.coalitions, self.scores, self.empty, self.delta = volumes, coalitions, scores, empty, delta
        self.A, self.phi, self.info = A, phi, info


class RegionShap:
    """logits (B, classes): the unperturbed forward; target (B,): the class explained; base_score (B,); R: the regions;
    volumes: the volume arguments whose regions play; joint; seed; samples (N); paired; ridge; size = (D, H, W).
    joint=False with several volumes fits one game per volume: phi then lists them one after the other, and scores,
    empty_score, delta, coalitions, counts, r2() belong to the game of the first volume - of(volume) gives another one's."""

    def __init__(self, logits, target, base_score, R, volumes, joint, seed, samples, paired, ridge, size, atlas, games, torch_only):
        self.logits, self.target, self.base_score, self.R = logits, target, base_score, R
        self.volumes, self.joint, self.seed, self.samples, self.paired, self.ridge = volumes, joint, seed, samples, paired, ridge
        self.size, self.atlas = size, atlas
        self._games, self._torch_only = games, torch_only

    def _game(self, volume):
        """-> (the game volume argument `volume` plays in, its first player there)."""
        if volume is None:
            volume = self.volumes[0]
        for g in self._games:
            if volume in g.volumes:
                return g, g.volumes.index(volume) * self.R
        raise KeyError(f"no values for volume {volume!r}: the regions of volume arguments {self.volumes} played")

    def of(self, volume):
        """The result restricted to the game volume argument `volume` plays in."""
        g, _p0 = self._game(volume)
        return RegionShap(self.logits, self.target, self.base_score, self.R, g.volumes, self.joint, self.seed, self.samples,
                          self.paired, self.ridge, self.size, self.atlas, [g], self._torch_only)

    phi = property(lambda self: torch.cat([g.phi for g in self._games], 1), doc="(B, P) float64: every player's share")
    players = property(lambda self: sum(g.phi.shape[1] for g in self._games), doc="P")
    scores = property(lambda self: self._games[0].scores, doc="(B, N): the score under every sampled coalition")
    empty_score = property(lambda self: self._games[0].empty, doc="(B,): the score with every region replaced")
    delta = property(lambda self: self._games[0].delta, doc="(B,) float64: base_score - empty_score, the sum of the shares")
    coalitions = property(lambda self: self._games[0].coalitions, doc="(N, Wd) int32: the sampled rows")
    counts = property(lambda self: self._games[0].A.diagonal(), doc="(P,) int32: the coalitions each player is in")
    info = property(lambda self: torch.cat([g.info for g in self._games]), doc="per game: 0, or the first failed pivot")

    def values(self, volume=None):
        """(B, R) in the logits' dtype: the shares of the regions 1..R of volume argument `volume` (default: the first)."""
        g, p0 = self._game(volume)
        return g.phi[:, p0:p0 + self.R].to(self.logits.dtype)

    def ok(self):
        """Whether every fit was solved (info == 0); one host read."""
        return bool((self.info == 0).all())

    def r2(self):
        """(B,) float64: the fit's coefficient of determination over the sampled coalitions, 1 - sum (y - z phi)^2 / sum (y -
        mean y)^2 with y = score - empty_score: near 1 where the game is close to additive (the counterpart of Rise.split_half)."""
        g = self._games[0]
        z = ops.shap_unpack(g.coalitions.to(g.phi.device), g.phi.shape[1]).double()
        y = g.scores.double() - g.empty.double().view(-1, 1)
        res = ((y - g.phi @ z.t()) ** 2).sum(1)
        tot = ((y - y.mean(1, keepdim=True)) ** 2).sum(1)
        return 1.0 - res / tot.clamp_min(torch.finfo(torch.float64).tiny)

    def volume(self, volume=None):
        """(B, D, H, W): values(volume) back on the voxel grid, 0 on the background."""
        v = self.values(volume).contiguous()
        return (ops.occlusion_volume_torch if self._torch_only else ops.occlusion_volume)(v, self.size, labels=self.atlas)

    def top(self, k, volume=None):
        """(indices (B, k) int64 in 1..R, values (B, k)): the k regions of that volume with the largest shares, the largest first."""
        v, i = self.values(volume).topk(_int(k, f"k must lie in 1..{self.R}", 1, self.R), dim=1)
        return i + 1, v

    def table(self, names=None):
        """One host copy -> a list of dict rows (sample, volume, region, name, value), sample-major, for printing or pandas.
        names: a sequence of R + 1 names (bin 0, the background, first - RegionStats.table's) or a dict region -> name."""
        if names is not None and not isinstance(names, dict):
            names = list(names)
            if len(names) != self.R + 1:
                raise ValueError(f"names must hold {self.R + 1} names (bin 0 first), got {len(names)}")
        name = lambda r: (names.get(r, str(r)) if isinstance(names, dict) else names[r]) if names is not None else str(r)
        host = torch.stack([self.values(i).double() for i in self.volumes]).cpu()
        return [dict(sample=b, volume=i, region=r + 1, name=name(r + 1), value=float(host[q, b, r]))
                for b in range(host.shape[1]) for q, i in enumerate(self.volumes) for r in range(self.R)]


def _run(model, volumes, atlas, samples, seed, paired, ridge, fill, baseline, score, target, output, which, joint, chunk, reuse,
         torch_only):
    vols, B = _pass_arguments("region_shap", "coalitions", model, volumes, score, chunk)
    which = tuple(range(len(vols))) if which is None else (which,) if isinstance(which, int) else tuple(which)
    if not which or any(not _is_int(i) or not 0 <= i < len(vols) for i in which) or len(set(which)) != len(which):
        raise ValueError(f"volumes must name some of the {len(vols)} volume arguments once each, got {which!r}")
    size = tuple(int(s) for s in vols[which[0]].shape[-3:])
    if any(tuple(vols[i].shape[-3:]) != size or vols[i].numel() != B * size[0] * size[1] * size[2] for i in which):
        raise ValueError("the perturbed volumes must be one-channel volumes of one spatial shape")
    if not torch.is_tensor(atlas) or atlas.dtype.is_floating_point or atlas.dtype == torch.bool or tuple(atlas.shape) != size:
        raise ValueError(f"atlas must be an integer label volume of shape {size}")
    R = int(atlas.max())
    if R < 1:
        raise ValueError("atlas has no label above 0: no region to play")
    games = [which] if joint else [(i,) for i in which]
    if R * len(games[0]) < 2 or R * len(games[0]) > ops.SHAP_MAX_PLAYERS:
        raise ValueError(f"P = {R} regions x {len(games[0])} volumes = {R * len(games[0])} players outside 2..{ops.SHAP_MAX_PLAYERS}")
    N = samples
    if not _is_int(N) or N < 2 or (paired and N % 2):
        raise ValueError(f"samples must be an integer >= 2{', even with paired=True' if paired else ''}, got {samples!r}")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    if not isinstance(ridge, (int, float)) or isinstance(ridge, bool) or not (0.0 <= float(ridge) < math.inf):
        raise ValueError(f"ridge must be a finite number >= 0, got {ridge!r}")
    atlas = atlas.detach().to(device=vols[which[0]].device, dtype=torch.int32).contiguous()
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
    coalitions, apply, gram, solve = (ops.shap_coalitions_torch, ops.shap_apply_torch, ops.shap_gram_torch, ops.shap_solve_torch) \
        if torch_only else (ops.shap_coalitions, ops.shap_apply, ops.shap_gram, ops.shap_solve)
    first = vols[which[0]]

    with torch.no_grad(), _on(vols[0]):
        run = _Pass(model, vols, score, target, output, chunk, reuse)
        fitted = []
        for game in games:
            P = R * len(game)
            coal = coalitions(P, paired, seed, 0, N, first.device)
            rows = torch.cat([coal, torch.zeros((1, coal.shape[1]), device=coal.device, dtype=coal.dtype)])     # + the empty coalition
            write = lambda i, j0, K, out: apply(vols[i], atlas, rows, fills[i], R, game.index(i) * R, P, j0, K, base=bases[i], out=out)
            # the chunk buffers of the kernel path, allocated once per pass (the torch ops allocate as they go)
            buffered = [i for i in game
                        if not torch_only and ops.shap_ok(vols[i], atlas, rows, bases[i] if bases[i] is not None else fills[i])
                        and vols[i].dtype == torch.float32]
            s = run.scores(game, N + 1, write, buffered).view(B, N + 1)
            scores, empty = s[:, :N].contiguous(), s[:, N].contiguous()
            delta = run.base.double() - empty.double()
            c = coal.to(scores.device)
            A, rhs = gram(c, scores, empty, P)
            phi, info = solve(A, rhs, delta, float(ridge))
            fitted.append(_Game(game, coal, scores, empty, delta, A, phi, info))
    return RegionShap(run.logits, run.target, run.base, R, which, bool(joint), seed, N, bool(paired), float(ridge), size, atlas,
                      fitted, torch_only)


def region_shap(model, *vols, atlas, samples=2048, seed=0, paired=True, ridge=0.0, fill=0.0, baseline=None, score="prob",
                target=None, output=0, volumes=None, joint=True, chunk=32, reuse=True):
    """Shapley values of the atlas regions for `model` (eval mode) on the volumes (B, 1, D, H, W) -> RegionShap.  See the module
    docstring for the estimator, atlas, samples, seed, paired, ridge, fill / baseline, score, target, `volumes`, joint, chunk
    and reuse.  ValueError for a model in train mode, a bad atlas, more than ops.SHAP_MAX_PLAYERS players, samples < 2 or odd
    with paired, a bad seed, ridge, baseline, fill, score or volume index."""
    return _run(model, vols, atlas, samples, seed, bool(paired), ridge, fill, baseline, score, target, output, volumes, bool(joint),
                chunk, bool(reuse), False)


def region_shap_torch(model, *vols, atlas, samples=2048, seed=0, paired=True, ridge=0.0, fill=0.0, baseline=None, score="prob",
                      target=None, output=0, volumes=None, joint=True, chunk=32, reuse=False):
    """region_shap on the stock-torch twins: any device, dtype and nn.Module.  `reuse` is accepted and ignored: tmf_replay is
    not used here."""
    return _run(model, vols, atlas, samples, seed, bool(paired), ridge, fill, baseline, score, target, output, volumes, bool(joint),
                chunk, False, True)
