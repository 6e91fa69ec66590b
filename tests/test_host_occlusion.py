"""Occlusion sensitivity without a GPU: the window-grid arithmetic against brute force, the coverage of every voxel, the torch
formulas of transmf_ad_amd.ops against the fp64 / clone-and-assign formulas of tests/_occlusion_inputs.py, the recorded
distances, occlusion_sensitivity_torch on a toy two-input module against a loop written out by hand (a linear model, where a
drop is the window's weight sum times (x - fill)), target resolution, joint, volumes, atlas, the ValueErrors, the sNet.tmf_replay
checks, the committed fixtures' keep rule, and the new entries in the header, the built library, the binding and the documents."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import _occlusion_inputs as oi
from _golden import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"tmf_occlusion_windows": 9, "tmf_occlude_windows": 16, "tmf_occlude_labels": 12, "tmf_occlusion_volume": 13,
           "tmf_occlusion_volume_labels": 9}


# ---------------------------------------------------------------------------------------------------------------------
# the grid
# ---------------------------------------------------------------------------------------------------------------------

def test_grid_arithmetic_against_brute_force():
    """n = ceil(max(S - p, 0) / s) + 1 and [i*s, min(i*s + p, S)) in the package, in the library and by walking the axis; every
    voxel is covered; the covering windows of a coordinate are i_lo = max(0, ceil((z-p+1)/s)) .. i_hi = min(n-1, floor(z/s))."""
    from transmf_ad_amd import _lib, ops
    lib = _lib.load()
    for S in range(1, 14):
        for p in range(1, 16):
            for s in range(1, p + 1):
                wins = oi.axis_windows(S, p, s)
                n = len(wins)
                assert n == -(-max(S - p, 0) // s) + 1 == ops.occlusion_grid((S, 1, 1), (p, 1, 1), (s, 1, 1))[0]
                assert lib.tmf_occlusion_windows(S, 1, 1, p, 1, 1, s, 1, 1) == n
                assert lib.tmf_occlusion_windows(1, 1, S, 1, 1, p, 1, 1, s) == n
                assert wins[-1][1] == S and all(a < b for a, b in wins)
                for i, (a, b) in enumerate(wins):
                    assert (a, b) == (i * s, min(i * s + p, S))
                    sl = ops.occlusion_window((1, S, 1), (1, p, 1), (1, s, 1), i)[1]
                    assert (sl.start, sl.stop) == (a, b)
                for z in range(S):
                    inside = [i for i, (a, b) in enumerate(wins) if a <= z < b]
                    lo = max(0, -(-(z - p + 1) // s))
                    hi = min(n - 1, z // s)
                    assert inside == list(range(lo, hi + 1)) and inside, (S, p, s, z)


@pytest.mark.parametrize("case", oi.OCCLUDE_CASES, ids=oi.case_id)
def test_window_order_and_coverage(case):
    from transmf_ad_amd import _lib, ops
    B, size, patch, stride = oi.geometry(case)
    wins, grid = oi.windows(size, patch, stride)
    assert grid == ops.occlusion_grid(size, patch, stride)
    assert _lib.load().tmf_occlusion_windows(*size, *patch, *stride) == len(wins) == grid[0] * grid[1] * grid[2]
    cover = torch.zeros(size, dtype=torch.int32)
    for w, (z0, z1, y0, y1, x0, x1) in enumerate(wins):
        assert ops.occlusion_window(size, patch, stride, w) == (slice(z0, z1), slice(y0, y1), slice(x0, x1))
        idx = (w // (grid[1] * grid[2]), w // grid[2] % grid[1], w % grid[2])
        assert (z0, y0, x0) == tuple(i * s for i, s in zip(idx, stride))
        cover[z0:z1, y0:y1, x0:x1] += 1
    assert int(cover.min()) >= 1
    assert (int(cover.max()) > 1) == oi.overlapping(case)
    for j0, K in oi.chunkings(B, len(wins)):
        assert K >= 1 and 0 <= j0 and j0 + K <= B * len(wins)
    if B > 1:
        j0, K = oi.chunkings(B, len(wins))[1]
        assert j0 % len(wins) != 0 or len(wins) == 1
        assert j0 // len(wins) != (j0 + K - 1) // len(wins)                  # the chunk crosses into the next sample


def test_cases_cover_what_the_kernels_can_get_wrong():
    vs = [oi.geometry(c)[1] for c in oi.OCCLUDE_CASES]
    nvox = [a * b * c for a, b, c in vs]
    assert any(n % 4 for n in nvox) and any(n % 4 == 0 for n in nvox)                  # both paths
    assert any(n > 256 * 4 * 4 and n % 4 for n in nvox)                                 # scalar path, more than one workgroup
    assert any(all(p > S for p, S in zip(oi.geometry(c)[2], oi.geometry(c)[1])) for c in oi.OCCLUDE_CASES)
    assert any(oi.geometry(c)[1][2] > 256 for c in oi.OCCLUDE_CASES)
    assert sum(oi.overlapping(c) for c in oi.OCCLUDE_CASES) == len(oi.VOLUME_DISTANCE) == 3
    assert {oi.geometry(c)[0] for c in oi.OCCLUDE_CASES} == {1, 2, 3}
    for size, R in oi.ATLAS_CASES:
        lab = oi.atlas_labels(size, R)
        present = set(lab.unique().tolist())
        assert oi.ATLAS_ABSENT not in present and {0, 1, R, R + 3, -1} <= present and lab.dtype == torch.int32


# ---------------------------------------------------------------------------------------------------------------------
# the torch formulas of ops.py (what runs off the kernels' ground) against the formulas of _occlusion_inputs.py
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", oi.OCCLUDE_CASES, ids=oi.case_id)
def test_torch_formulas_against_brute_force(case):
    from transmf_ad_amd import ops
    B, size, patch, stride = oi.geometry(case)
    vol, fill = oi.occlude_inputs(case)
    wins, grid = oi.windows(size, patch, stride)
    nW = len(wins)
    keep = vol.clone()
    for j0, K in oi.chunkings(B, nW):
        want = oi.occlude_ref(vol, fill, patch, stride, j0, K)
        got = ops.occlude_windows(vol, fill, patch, stride, j0, K)
        assert got.shape == (K, 1) + size and torch.equal(got, want)
        assert torch.equal(ops.occlude_windows_torch(vol, fill, patch, stride, j0, K), want)      # the forced form: same formula
        assert int((got != vol[(torch.arange(j0, j0 + K) // nW)]).sum()) > 0
        buf = torch.full((K, 1) + size, 9.0)
        assert ops.occlude_windows(vol, fill, patch, stride, j0, K, out=buf) is buf and torch.equal(buf, want)
        got64 = ops.occlude_windows(vol.double(), fill.double(), patch, stride, j0, K)
        assert got64.dtype == torch.float64 and torch.equal(got64, want.double())
    assert torch.equal(vol, keep)
    drops = oi.drops_for(B, nW)
    ref = oi.volume_ref64(drops, size, patch, stride)
    got = ops.occlusion_volume(drops, size, patch, stride)
    assert torch.equal(got, oi.volume_formula32(drops, size, patch, stride))
    if not oi.overlapping(case):
        gathered = torch.zeros((B,) + size)
        for w, (z0, z1, y0, y1, x0, x1) in enumerate(wins):
            gathered[:, z0:z1, y0:y1, x0:x1] = drops[:, w].view(B, 1, 1, 1)
        assert torch.equal(got, gathered) and torch.equal(got.double(), ref)
    else:
        assert float(oi.row_errors(got, ref).max()) <= oi.volume_tolerance(case) / oi.MARGIN * 2
    got64 = ops.occlusion_volume(drops.double(), size, patch, stride)
    assert float(oi.row_errors(got64, ref).max()) <= 1e-15
    for fn in (ops.occlude_windows, ops.occlude_windows_torch):
        with pytest.raises(ValueError):
            fn(vol, fill, patch, stride, B * nW, 1)
        with pytest.raises(ValueError):
            fn(vol, fill[:0], patch, stride, 0, 1)
    with pytest.raises(ValueError):
        ops.occlusion_volume(drops[:, :-1] if nW > 1 else torch.zeros(B, 2), size, patch, stride)


@pytest.mark.parametrize("case", [c for c in oi.OCCLUDE_CASES if oi.overlapping(c)], ids=oi.case_id)
def test_recorded_distances(case):
    """The table is what this machine measures, within 2x above the floor."""
    now, rec = oi.volume_distance(case), oi.VOLUME_DISTANCE[oi.case_id(case)]
    assert now <= 2 * max(rec, oi.VOLUME_FLOOR) and rec <= 2 * max(now, oi.VOLUME_FLOOR), (now, rec)
    assert oi.volume_tolerance(case) >= oi.MARGIN * oi.VOLUME_FLOOR


@pytest.mark.parametrize("size,R", oi.ATLAS_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_atlas_formulas(size, R):
    from transmf_ad_amd import ops
    vol, lab, fill = oi.atlas_inputs(size, R)
    B = vol.shape[0]
    for j0, K in oi.chunkings(B, R):
        want = oi.occlude_labels_ref(vol, lab, fill, R, j0, K)
        assert torch.equal(ops.occlude_labels(vol, lab, fill, R, j0, K), want)
        assert torch.equal(ops.occlude_labels_torch(vol, lab, fill, R, j0, K), want)
    absent = ops.occlude_labels(vol, lab, fill, R, oi.ATLAS_ABSENT - 1, 1)
    assert torch.equal(absent[0], vol[0])                                   # a region without voxels: the volume itself
    every = torch.stack([ops.occlude_labels(vol, lab, fill, R, r, 1)[0] for r in range(R)])
    outside = (lab < 1) | (lab > R)
    assert torch.equal(every[:, 0, outside], vol[0, 0, outside].expand(R, -1))     # background and strays are never occluded
    drops = oi.drops_for(B, R, seed=1) + 1.0
    got = ops.occlusion_volume(drops, size, labels=lab)
    assert torch.equal(got, oi.volume_labels_ref(drops, lab, R)) and bool((got[:, outside] == 0).all())
    for fn in (ops.occlude_labels, ops.occlude_labels_torch):
        with pytest.raises(ValueError):
            fn(vol, lab.float(), fill, R, 0, 1)
    with pytest.raises(ValueError):
        ops.occlusion_volume(drops, size, labels=lab[:-1])


# ---------------------------------------------------------------------------------------------------------------------
# occlusion_sensitivity_torch on a toy module against a hand-written loop
# ---------------------------------------------------------------------------------------------------------------------

SIZE = (5, 7, 3)


class _Linear2(nn.Module):
    """logits = <A, x> + <C, y> + bias over two one-channel volumes, three classes; returns a tuple as the package's models do."""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        n = SIZE[0] * SIZE[1] * SIZE[2]
        self.a = nn.Parameter(torch.randn((3, n), generator=g, dtype=torch.float64))
        self.c = nn.Parameter(torch.randn((3, n), generator=g, dtype=torch.float64))
        self.bias = nn.Parameter(torch.randn((3,), generator=g, dtype=torch.float64))
        self.calls = 0

    def forward(self, x, y):
        self.calls += 1
        return x.flatten(1) @ self.a.t() + y.flatten(1) @ self.c.t() + self.bias, x.flatten(1).sum(1, keepdim=True)


class _Curved(_Linear2):
    def forward(self, x, y):
        lo, aux = super().forward(x, y)
        return torch.tanh(lo / 20) * 3, aux


def _toy(cls=_Linear2):
    g = torch.Generator().manual_seed(8)
    x = torch.rand((3, 1) + SIZE, generator=g, dtype=torch.float64)
    y = torch.rand((3, 1) + SIZE, generator=g, dtype=torch.float64)
    return cls().eval(), x, y


def _by_hand(net, vols, which, patch, stride, fills, target, score="logit", atlas=None):
    """The user's loop: one clone and one forward per job, all selected volumes occluded together -> drops (B, nW)."""
    B = vols[0].shape[0]
    if atlas is None:
        wins, _g = oi.windows(SIZE, patch, stride)
        masks = []
        for z0, z1, y0, y1, x0, x1 in wins:
            m = torch.zeros(SIZE, dtype=torch.bool)
            m[z0:z1, y0:y1, x0:x1] = True
            masks.append(m)
    else:
        masks = [atlas == r for r in range(1, int(atlas.max()) + 1)]

    def sc(lo, b):
        return (lo if score == "logit" else torch.softmax(lo, 1))[0, target[b]]

    drops = torch.zeros((B, len(masks)), dtype=vols[0].dtype)
    with torch.no_grad():
        for b in range(B):
            base = sc(net(*[v[b:b + 1] for v in vols])[0], b)
            for w, m in enumerate(masks):
                job = [v[b:b + 1].clone() for v in vols]
                for i in which:
                    job[i][0, 0][m] = fills[i][b]
                drops[b, w] = base - sc(net(*job)[0], b)
    return drops


def test_linear_model_drops_are_window_weight_sums():
    """On a linear model a drop is exactly sum over the window of weight[target] * (x - fill): grid with overlap, default
    target = the argmax of the unoccluded logits, zero fill and a per-sample fill tensor, a chunk that straddles samples."""
    from transmf_ad_amd import occlusion_sensitivity_torch
    net, x, y = _toy()
    patch, stride = (2, 3, 2), (2, 3, 1)
    wins, grid = oi.windows(SIZE, patch, stride)
    for fill in (0.0, torch.tensor([0.25, -1.0, 2.0])):
        net.calls = 0
        occ = occlusion_sensitivity_torch(net, x, y, patch=patch, stride=stride, fill=fill, chunk=7)
        B, nW = 3, len(wins)
        assert net.calls == 1 + 2 * -(-B * nW // 7)
        with torch.no_grad():
            logits = net(x, y)[0]
        assert torch.equal(occ.logits, logits) and torch.equal(occ.target, logits.argmax(1))
        assert torch.equal(occ.base_score, logits.gather(1, occ.target.view(-1, 1))[:, 0])
        assert occ.grid == grid and occ.patch == patch and occ.stride == stride and occ.volumes == (0, 1)
        f = torch.full((3,), fill, dtype=torch.float64) if isinstance(fill, float) else fill.double()
        for i, (v, wt) in enumerate(((x, net.a), (y, net.c))):
            want = torch.zeros((B, nW), dtype=torch.float64)
            for b in range(B):
                wv = wt[occ.target[b]].detach().view(SIZE)
                for w, (z0, z1, y0, y1, x0, x1) in enumerate(wins):
                    want[b, w] = (wv[z0:z1, y0:y1, x0:x1] * (v[b, 0, z0:z1, y0:y1, x0:x1] - f[b])).sum()
            got = occ.drops(i)
            assert got.shape == (B,) + grid and got.dtype == torch.float64
            assert float((got.reshape(B, -1) - want).abs().max()) <= 1e-12 * float(want.abs().max())
            assert torch.equal(occ.volume(i), oi.volume_ref64(got.reshape(B, -1), SIZE, patch, stride)) or float(
                oi.row_errors(occ.volume(i), oi.volume_ref64(got.reshape(B, -1), SIZE, patch, stride)).max()) <= 1e-15
            assert occ.volume(i).shape == (B,) + SIZE
    with pytest.raises(KeyError):
        occ.drops(2)


@pytest.mark.parametrize("score", ("logit", "prob"))
def test_against_the_hand_written_loop(score):
    """A model that is not linear: target (int, per sample), volumes, joint, fill="mean", atlas, stride=None, score."""
    from transmf_ad_amd import occlusion_sensitivity, occlusion_sensitivity_torch
    net, x, y = _toy(_Curved)
    vols = [x, y]
    mean = [v.reshape(3, -1).mean(1) for v in vols]
    zero = [torch.zeros(3, dtype=torch.float64)] * 2
    patch = (3, 3, 3)

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-13

    t = torch.tensor([2, 0, 1])
    occ = occlusion_sensitivity_torch(net, x, y, patch=3, target=t, score=score, chunk=4)
    assert occ.stride == patch and torch.equal(occ.target, t)
    for i in (0, 1):
        assert close(occ.drops(i).reshape(3, -1), _by_hand(net, vols, (i,), patch, patch, zero, t, score))
    occ = occlusion_sensitivity_torch(net, x, y, patch=3, target=1, score=score, volumes=(1,), fill="mean")
    assert occ.volumes == (1,) and occ.target.tolist() == [1, 1, 1]
    assert close(occ.drops().reshape(3, -1), _by_hand(net, vols, (1,), patch, patch, mean, [1, 1, 1], score))
    assert torch.equal(occ.drops(), occ.drops(1))
    with pytest.raises(KeyError):
        occ.volume(0)
    occ = occlusion_sensitivity_torch(net, x, y, patch=3, stride=2, target=t, score=score, joint=True, fill="mean", chunk=100)
    want = _by_hand(net, vols, (0, 1), patch, (2, 2, 2), mean, t, score)
    assert close(occ.drops().reshape(3, -1), want) and torch.equal(occ.drops(0), occ.drops(1)) and occ.joint
    assert float(oi.row_errors(occ.volume(), oi.volume_ref64(occ.drops().reshape(3, -1), SIZE, patch, (2, 2, 2))).max()) <= 1e-15
    atlas = oi.atlas_labels(SIZE, 3)
    atlas = torch.where(atlas > 3, torch.zeros_like(atlas), atlas)      # R is the atlas's maximum: keep the stray -1 only
    occ = occlusion_sensitivity_torch(net, x, y, atlas=atlas, target=t, score=score, chunk=2)
    assert occ.grid is None and occ.drops(0).shape == (3, 3) and int(atlas.min()) == -1
    for i in (0, 1):
        assert close(occ.drops(i), _by_hand(net, vols, (i,), None, None, zero, t, score, atlas=atlas))
        assert torch.equal(occ.volume(i), oi.volume_labels_ref(occ.drops(i), atlas, 3))
        assert float(occ.drops(i)[:, oi.ATLAS_ABSENT - 1].abs().max()) == 0            # nothing occluded: no drop
    # off the kernels' ground (the CPU, float64) occlusion_sensitivity computes the same with torch ops, nothing to reuse
    dev = occlusion_sensitivity(net, x, y, patch=3, stride=2, target=t, score=score, chunk=5)
    ref = occlusion_sensitivity_torch(net, x, y, patch=3, stride=2, target=t, score=score, chunk=5)
    for i in (0, 1):
        assert torch.equal(dev.drops(i), ref.drops(i)) and torch.equal(dev.volume(i), ref.volume(i))


def test_value_errors_and_untouched_state():
    from transmf_ad_amd import occlusion_sensitivity, occlusion_sensitivity_torch
    net, x, y = _toy()
    for fn in (occlusion_sensitivity, occlusion_sensitivity_torch):
        with pytest.raises(ValueError, match="eval"):
            fn(net.train(), x, y, patch=3)
        net.eval()
        for bad in (dict(patch=2, stride=3), dict(patch=(2, 2, 2), stride=(1, 3, 1)), dict(patch=0), dict(patch=(2, 2)),
                    dict(patch=2, stride=0), dict(patch=2.5),
                    dict(patch=3, fill=torch.zeros(2)), dict(patch=3, fill=torch.zeros(3, 1)), dict(patch=3, fill="median"),
                    dict(patch=3, fill=None), dict(patch=3, score="margin"), dict(patch=3, volumes=(2,)),
                    dict(patch=3, volumes=(0, 0)), dict(patch=3, volumes=()), dict(patch=3, chunk=0), dict(patch=3, target=3),
                    dict(patch=3, target=torch.tensor([0, 1])), dict(patch=3, output=2),
                    dict(atlas=torch.zeros(SIZE, dtype=torch.int64)), dict(atlas=torch.ones(SIZE)),
                    dict(atlas=torch.ones((5, 7, 4), dtype=torch.int64))):
            with pytest.raises(ValueError):
                fn(net, x, y, **bad)
        with pytest.raises(ValueError):
            fn(net, x.long(), y, patch=3)
        with pytest.raises(TypeError):
            fn(lambda a, b: a, x, y, patch=3)
    keep = (x.clone(), y.clone(), {k: v.clone() for k, v in net.state_dict().items()}, torch.get_rng_state())
    xr = x.clone().requires_grad_(True)
    occ = occlusion_sensitivity_torch(net, xr, y, patch=3, output=0)
    assert torch.equal(x, keep[0]) and torch.equal(y, keep[1]) and torch.equal(torch.get_rng_state(), keep[3])
    assert all(torch.equal(v, keep[2][k]) for k, v in net.state_dict().items())
    assert all(p.grad is None for p in net.parameters()) and xr.grad is None
    assert not occ.drops(0).requires_grad and not occ.logits.requires_grad
    one = occlusion_sensitivity_torch(net, x, y, patch=3, output=1, target=0)          # the other output: (B, 1) "logits"
    assert one.logits.shape == (3, 1) and float(one.drops(1).abs().max()) == 0 and float(one.drops(0).abs().max()) > 0


def test_replay_hook_checks_before_any_launch():
    """sNet.tmf_replay on the CPU: the tensor comes back as it is, without a kernel (there is no device here to launch on); a
    mismatched K, grid or width is a ValueError; None is the default."""
    import transmf_ad_amd as T
    enc = T.sNet(32).eval()
    assert enc.tmf_replay is None
    vol = torch.zeros((3, 1, 32, 48, 16))
    rep = torch.randn((3, 2, 3, 1, 32))
    enc.tmf_replay = rep
    assert enc.forward_channels_last(vol) is rep
    assert torch.equal(enc(vol.expand(3, 1, 32, 48, 16)), rep.permute(0, 4, 1, 2, 3))
    for bad in (torch.randn((2, 2, 3, 1, 32)), torch.randn((3, 2, 3, 2, 32)), torch.randn((3, 2, 3, 1, 16)),
                torch.randn((3, 32, 2, 3, 1)), torch.randn((3, 2, 3, 32)), "x"):
        enc.tmf_replay = bad
        with pytest.raises(ValueError, match="tmf_replay"):
            enc.forward_channels_last(vol)
    enc.tmf_replay = rep
    with pytest.raises(ValueError):
        enc.forward_channels_last(vol[:, 0])                                # the encoder's own shape check comes first


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no launch is reached: these run without a device), fixtures, header, documents
# ---------------------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    """Every entry returns a negative TMF_E_* for what the header says it refuses - before any launch, so no device is needed
    and the (never dereferenced) pointers here are made up."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    p, q = 1 << 20, (1 << 20) + 4096
    ok = (2, 8, 8, 8, 4, 4, 4, 2, 2, 2)                                    # B, D, H, W, patch, stride: nW = 27
    assert lib.tmf_occlusion_windows(*ok[1:]) == 27
    E = lambda rc: rc in (_lib.E_NULL, _lib.E_SHAPE, _lib.E_ALIGN, _lib.E_ARG)
    for args in ((None, p, q), (p, None, q), (p, p, None)):
        assert lib.tmf_occlude_windows(*args, *ok, 0, 1, None) == _lib.E_NULL
    for args in ((None, p, p, q), (p, None, p, q), (p, p, None, q), (p, p, p, None)):
        assert lib.tmf_occlude_labels(*args, 2, 8, 8, 8, 3, 0, 1, None) == _lib.E_NULL
    assert lib.tmf_occlusion_volume(None, q, *ok, None) == _lib.E_NULL == lib.tmf_occlusion_volume(p, None, *ok, None)
    for args in ((None, p, q), (p, None, q), (p, p, None)):
        assert lib.tmf_occlusion_volume_labels(*args, 2, 8, 8, 8, 3, None) == _lib.E_NULL
    geoms = [(2, 8, 8, 8, 4, 4, 4, 0, 2, 2), (2, 8, 8, 8, 4, 4, 4, 2, 5, 2), (2, 8, 8, 8, 4, 4, 4, 2, 2, -1),      # stride
             (2, 8, 8, 8, 0, 4, 4, 1, 2, 2), (2, 8, 8, 8, 4, 4, -3, 2, 2, 1),                                     # patch
             (2, 0, 8, 8, 4, 4, 4, 2, 2, 2), (2, 8, -1, 8, 4, 4, 4, 2, 2, 2), (2, 8, 8, 0, 4, 4, 4, 2, 2, 2),      # extents
             (2, 2048, 2048, 512, 4, 4, 4, 2, 2, 2), (2, 1 << 30, 2, 1, 4, 4, 4, 2, 2, 2),                        # D*H*W >= 2^31
             (2, 46341, 46341, 1, 4, 4, 4, 2, 2, 2)]
    for g in geoms:
        assert E(lib.tmf_occlusion_windows(*g[1:])), g
        assert E(lib.tmf_occlude_windows(p, p, q, *g, 0, 1, None)), g
        assert E(lib.tmf_occlusion_volume(p, q, *g, None)), g
    for g in geoms[5:]:
        assert E(lib.tmf_occlude_labels(p, p, p, q, *g[:4], 3, 0, 1, None)), g
        assert E(lib.tmf_occlusion_volume_labels(p, p, q, *g[:4], 3, None)), g
    for j0, K in ((0, 0), (0, -1), (-1, 1), (54, 1), (50, 5), (0, 55), ((1 << 31) - 1, 1), (0, 1 << 17)):
        assert E(lib.tmf_occlude_windows(p, p, q, *ok, j0, K, None)), (j0, K)
    for j0, K in ((0, 0), (-1, 1), (6, 1), (4, 3)):
        assert E(lib.tmf_occlude_labels(p, p, p, q, 2, 8, 8, 8, 3, j0, K, None)), (j0, K)
    for B in (0, -1):
        assert E(lib.tmf_occlude_windows(p, p, q, B, *ok[1:], 0, 1, None))
        assert E(lib.tmf_occlusion_volume(p, q, B, *ok[1:], None))
        assert E(lib.tmf_occlusion_volume_labels(p, p, q, B, 8, 8, 8, 3, None))
    assert E(lib.tmf_occlude_windows(p, p, q, 1 << 30, 1, 1, 16, 1, 1, 1, 1, 1, 1, 0, 1, None))       # B * nW >= 2^31
    for R in (0, -2):
        assert E(lib.tmf_occlude_labels(p, p, p, q, 2, 8, 8, 8, R, 0, 1, None))
        assert E(lib.tmf_occlusion_volume_labels(p, p, q, 2, 8, 8, 8, R, None))
    assert lib.tmf_occlude_windows(p + 2, p, q, *ok, 0, 1, None) == _lib.E_ALIGN
    assert lib.tmf_occlude_windows(p, p, q + 1, *ok, 0, 1, None) == _lib.E_ALIGN
    assert lib.tmf_occlude_labels(p, p + 2, p, q, 2, 8, 8, 8, 3, 0, 1, None) == _lib.E_ALIGN
    assert lib.tmf_occlusion_volume(p, q + 2, *ok, None) == _lib.E_ALIGN
    assert lib.tmf_occlusion_volume_labels(p, p + 1, q, 2, 8, 8, 8, 3, None) == _lib.E_ALIGN
    assert b"tmf_occlusion_volume_labels" in lib.tmf_last_error_string()


def test_committed_fixtures_keep_rule():
    """occlusion_cnn_tiny / occlusion_ad_tiny: every setting and modality with fp64 and fp32 drops, the fp64 logits of every
    job (the drops are their differences from the base logits), the reference's fp32 run within 1e-3 of its fp64 run."""
    for name in ("cnn_tiny", "ad_tiny"):
        path = os.path.join(GOLDEN_DIR, f"occlusion_{name}.npz")
        assert os.path.getsize(path) < 1 << 20
        z = np.load(path)
        settings = str(z["settings"]).split(",")
        assert settings == ["p8", "p16", "p16s8"]
        B = z["logits"].shape[0]
        assert z["logits"].dtype == np.float64 and np.array_equal(z["target"], z["logits"].argmax(1))
        for s, grid in zip(settings, ((4, 4, 4), (2, 2, 2), (3, 3, 3))):
            for mod in ("mri", "pet"):
                key = f"{s}.{mod}"
                d64, d32, jobs = z[key + ".drops"], z[key + ".drops.f32"], z[key + ".logits"]
                assert d64.shape == d32.shape == (B,) + grid and d64.dtype == np.float64 and d32.dtype == np.float32
                assert jobs.shape == (B, grid[0] * grid[1] * grid[2], 2)
                t = z["target"]
                base = z["logits"][np.arange(B), t]
                assert np.allclose(d64.reshape(B, -1), base[:, None] - jobs[np.arange(B), :, t], rtol=0, atol=1e-15)
                peak = np.abs(d64).reshape(B, -1).max(1)
                assert (peak > 0).all() and np.array_equal(peak, z["max." + key])
                dist = (np.abs(d32.astype(np.float64) - d64).reshape(B, -1).max(1) / peak).max()
                assert dist == float(z["dist." + key]) and dist <= 1e-3, (name, key, dist)


def test_new_names_in_header_library_binding_and_documents():
    from transmf_ad_amd import _lib, build, ops
    import transmf_ad_amd as T
    with open(os.path.join(ROOT, "include", "tmf_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        row = [l for l in f if l.startswith("| **`tmf_occlude_windows`**")]
    assert len(row) == 1
    stated = {name: int(n) for name, n in re.findall(r"`(tmf_occlu\w*)`[^|`]*?\((\d+) arguments?\)", row[0])}
    assert stated == ENTRIES
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert "occlusion.hip" in build.SOURCES
    for fn in ("occlude_windows", "occlude_labels", "occlusion_volume", "occlusion_ok", "occlusion_grid", "occlusion_window"):
        assert callable(getattr(ops, fn)), fn
    assert "occlusion_sensitivity" in T.__all__ and "occlusion_sensitivity_torch" in T.__all__
    assert callable(T.occlusion_sensitivity) and callable(T.occlusion_sensitivity_torch)
    for doc in ("DESIGN.md", "README.md", os.path.join("profiles", "README.md")):
        with open(os.path.join(ROOT, doc)) as f:
            assert "occlusion" in f.read(), doc
    src = open(os.path.join(ROOT, "transmf_ad_amd", "networks.py")).read()
    assert "tmf_replay" in src and "tmf_replay" in T.occlusion.__doc__
