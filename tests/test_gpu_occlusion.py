"""Occlusion sensitivity on the device: the kernels of csrc/occlusion.hip on their own (through _lib.call with raw pointers)
against clone() plus slice assignment and the fp64 voxel map of tests/_occlusion_inputs.py; their refusals; sNet.tmf_replay;
occlusion_sensitivity against the model's own forward on batches the test builds itself (bit for bit), with and without encoder
reuse; against the drops the reference itself gives (tests/golden/occlusion_*.npz); the remaining options.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs
included) must be unchanged, every output element written."""
import copy
import os

import numpy as np
import pytest
import torch

import _occlusion_inputs as oi
from _golden import GOLDEN_DIR, Golden
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _st
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu
F32 = torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through raw pointers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", oi.OCCLUDE_CASES, ids=oi.case_id)
def test_occlude_windows_kernel(case):
    """torch.equal with clone() plus slice assignment for K = 1, a chunk that crosses into the next sample and the short last
    chunk; the 16-byte path where D*H*W % 4 == 0 (the arena's slots are 256-byte aligned), the scalar path otherwise and, on
    the % 4 == 0 cases, once more through an output that starts 4 bytes off."""
    B, size, patch, stride = oi.geometry(case)
    vol, fill = oi.occlude_inputs(case)
    wins, _grid = oi.windows(size, patch, stride)
    nW, V = len(wins), size[0] * size[1] * size[2]
    chunks = oi.chunkings(B, nW)
    outs = {f"out{i}": ((K, 1) + size, F32) for i, (_j0, K) in enumerate(chunks)}
    shifted = V % 4 == 0
    if shifted:
        outs["off"] = ((chunks[1][1] * V + 1,), F32)
    ar = Arena(dict(vol=vol, fill=fill), outs, tail=4096)
    for i, (j0, K) in enumerate(chunks):
        _call("tmf_occlude_windows", ar.ptr("vol"), ar.ptr("fill"), ar.ptr(f"out{i}"), B, *size, *patch, *stride, j0, K, _st())
    written = None
    if shifted:
        j0, K = chunks[1]
        _call("tmf_occlude_windows", ar.ptr("vol"), ar.ptr("fill"), ar.ptr("off") + 4, B, *size, *patch, *stride, j0, K, _st())
        written = {"off": torch.ones(K * V + 1, dtype=torch.bool)}
        written["off"][0] = False
    got = ar.fetch(written=written)
    for i, (j0, K) in enumerate(chunks):
        want = oi.occlude_ref(vol, fill, patch, stride, j0, K)
        assert torch.equal(got[f"out{i}"], want), (j0, K)
        if shifted and i == 1:
            assert torch.equal(got["off"][1:].view(want.shape), want)


@pytest.mark.parametrize("size,R", oi.ATLAS_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_occlude_labels_and_label_map_kernels(size, R):
    """Regions: every chunking, an absent label (the volume itself), strays outside 0..R (never occluded, 0 in the map); the
    map is a lookup: torch.equal, twice."""
    vol, lab, fill = oi.atlas_inputs(size, R)
    B = vol.shape[0]
    chunks = oi.chunkings(B, R) + [(oi.ATLAS_ABSENT - 1, 1)]
    drops = oi.drops_for(B, R, seed=1) + 1.0
    outs = {f"out{i}": ((K, 1) + tuple(size), F32) for i, (_j0, K) in enumerate(chunks)}
    outs["map0"], outs["map1"] = ((B,) + tuple(size), F32), ((B,) + tuple(size), F32)
    ar = Arena(dict(vol=vol, fill=fill, lab=lab, drops=drops), outs, tail=4096)
    for i, (j0, K) in enumerate(chunks):
        _call("tmf_occlude_labels", ar.ptr("vol"), ar.ptr("lab"), ar.ptr("fill"), ar.ptr(f"out{i}"), B, *size, R, j0, K, _st())
    for m in ("map0", "map1"):
        _call("tmf_occlusion_volume_labels", ar.ptr("drops"), ar.ptr("lab"), ar.ptr(m), B, *size, R, _st())
    got = ar.fetch()
    for i, (j0, K) in enumerate(chunks):
        assert torch.equal(got[f"out{i}"], oi.occlude_labels_ref(vol, lab, fill, R, j0, K)), (j0, K)
    assert torch.equal(got[f"out{len(chunks) - 1}"][0], vol[0])
    want = oi.volume_labels_ref(drops, lab, R)
    assert torch.equal(got["map0"], want) and torch.equal(got["map1"], want)
    assert bool((got["map0"][:, (lab < 1) | (lab > R)] == 0).all())


@pytest.mark.parametrize("case", oi.OCCLUDE_CASES, ids=oi.case_id)
def test_occlusion_volume_kernel(case):
    """stride == patch: the gathered drops, torch.equal.  Overlap: per sample row within MARGIN x the recorded distance of the
    fp32 scatter-add formula from fp64.  Two calls give the same bits."""
    B, size, patch, stride = oi.geometry(case)
    wins, _grid = oi.windows(size, patch, stride)
    drops = oi.drops_for(B, len(wins))
    outs = {m: ((B,) + size, F32) for m in ("map0", "map1")}
    ar = Arena(dict(drops=drops), outs, tail=4096)
    for m in outs:
        _call("tmf_occlusion_volume", ar.ptr("drops"), ar.ptr(m), B, *size, *patch, *stride, _st())
    got = ar.fetch()
    assert torch.equal(got["map0"], got["map1"])
    ref = oi.volume_ref64(drops, size, patch, stride)
    if not oi.overlapping(case):
        assert torch.equal(got["map0"].double(), ref)
    else:
        err, tol = float(oi.row_errors(got["map0"], ref).max()), oi.volume_tolerance(case)
        same = torch.equal(got["map0"], oi.volume_formula32(drops, size, patch, stride))
        print(f"{oi.case_id(case)}: err {err:.3e} tol {tol:.3e} err / tol {err / tol:.3f}; the bits of the torch formula: {same}")
        assert err <= tol


def test_entries_refuse_before_any_launch():
    """Bad arguments on real buffers full of a sentinel: a negative code, and every buffer unchanged."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    src = torch.full((2 * 512 + 64,), 7.0, device=DEV)
    dst = torch.full((64 * 512 + 64,), 7.0, device=DEV)
    lab = torch.full((512,), 1, device=DEV, dtype=torch.int32)
    p, q, l = src.data_ptr(), dst.data_ptr(), lab.data_ptr()
    ok = (2, 8, 8, 8, 4, 4, 4, 2, 2, 2)                                    # B, D, H, W, patch, stride: nW = 27
    neg = lambda rc: rc < 0
    for args in ((None, p, q), (p, None, q), (p, p, None)):
        assert neg(lib.tmf_occlude_windows(*args, *ok, 0, 1, None))
    for args in ((None, l, p, q), (p, None, p, q), (p, l, None, q), (p, l, p, None)):
        assert neg(lib.tmf_occlude_labels(*args, 2, 8, 8, 8, 3, 0, 1, None))
    assert neg(lib.tmf_occlusion_volume(None, q, *ok, None)) and neg(lib.tmf_occlusion_volume(p, None, *ok, None))
    for args in ((None, l, q), (p, None, q), (p, l, None)):
        assert neg(lib.tmf_occlusion_volume_labels(*args, 2, 8, 8, 8, 3, None))
    for g in [(2, 8, 8, 8, 4, 4, 4, 0, 2, 2), (2, 8, 8, 8, 4, 4, 4, 2, 5, 2), (2, 8, 8, 8, 0, 4, 4, 1, 2, 2),
              (2, 0, 8, 8, 4, 4, 4, 2, 2, 2), (2, 2048, 2048, 512, 4, 4, 4, 2, 2, 2), (0, 8, 8, 8, 4, 4, 4, 2, 2, 2)]:
        assert neg(lib.tmf_occlude_windows(p, p, q, *g, 0, 1, None)), g
        assert neg(lib.tmf_occlusion_volume(p, q, *g, None)), g
        assert g[0] == 0 or neg(lib.tmf_occlusion_windows(*g[1:])), g
    for j0, K in ((0, 0), (0, -1), (-1, 1), (54, 1), (50, 5), (0, 55)):
        assert neg(lib.tmf_occlude_windows(p, p, q, *ok, j0, K, None)), (j0, K)
    for j0, K in ((0, 0), (-1, 1), (6, 1), (4, 3)):
        assert neg(lib.tmf_occlude_labels(p, l, p, q, 2, 8, 8, 8, 3, j0, K, None)), (j0, K)
    for R in (0, -2):
        assert neg(lib.tmf_occlude_labels(p, l, p, q, 2, 8, 8, 8, R, 0, 1, None))
        assert neg(lib.tmf_occlusion_volume_labels(p, l, q, 2, 8, 8, 8, R, None))
    assert neg(lib.tmf_occlude_windows(p + 2, p, q, *ok, 0, 1, None)) and neg(lib.tmf_occlude_windows(p, p, q + 1, *ok, 0, 1, None))
    assert neg(lib.tmf_occlusion_volume(p, q + 2, *ok, None)) and neg(lib.tmf_occlusion_volume_labels(p, l + 1, q, 2, 8, 8, 8, 3, None))
    assert b"tmf_occlusion_volume_labels" in lib.tmf_last_error_string()
    torch.cuda.synchronize()
    assert bool((src == 7.0).all()) and bool((dst == 7.0).all()) and bool((lab == 1).all())


# ---------------------------------------------------------------------------------------------------------------------
# the ops wrappers and sNet.tmf_replay
# ---------------------------------------------------------------------------------------------------------------------

def _calls(monkeypatch, fn):
    """fn() -> (its result, the library entries it called in order, the ops wrappers it called in order)."""
    from transmf_ad_amd import _lib, ops
    names, wrappers, real = [], [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    for w in ("occlude_windows", "occlude_labels", "occlusion_volume"):
        monkeypatch.setattr(ops, w, (lambda f, w: lambda *a, **k: (wrappers.append(w), f(*a, **k))[1])(getattr(ops, w), w))
    try:
        return fn(), names, wrappers
    finally:
        monkeypatch.undo()


def test_ops_wrappers_route(monkeypatch):
    """Contiguous float32 HIP tensors take the kernels (one launch each), anything else the torch formulas: the same values."""
    from transmf_ad_amd import ops
    case = oi.OCCLUDE_CASES[2]
    B, size, patch, stride = oi.geometry(case)
    vol, fill = oi.occlude_inputs(case)
    wins, _g = oi.windows(size, patch, stride)
    j0, K = oi.chunkings(B, len(wins))[1]
    want = oi.occlude_ref(vol, fill, patch, stride, j0, K)
    v, f = vol.to(DEV), fill.to(DEV)
    assert ops.occlusion_ok(v, f) and not ops.occlusion_ok(vol, fill) and not ops.occlusion_ok(v.double(), f)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlude_windows(v, f, patch, stride, j0, K))
    assert names == ["tmf_occlude_windows"] and torch.equal(got.cpu(), want)
    buf = torch.empty((K + 3, 1) + size, device=DEV)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlude_windows(v, f, patch, stride, j0, K, out=buf[:K]))
    assert names == ["tmf_occlude_windows"] and got.data_ptr() == buf.data_ptr() and torch.equal(got.cpu(), want)
    wide = torch.zeros((B, 1) + size[:2] + (2 * size[2],), device=DEV)
    wide[..., ::2] = v
    for other in (wide[..., ::2], v.double(), v.bfloat16()):
        got, names, _w = _calls(monkeypatch, lambda: ops.occlude_windows(other, f.to(other.dtype), patch, stride, j0, K))
        assert names == [] and got.dtype == other.dtype and got.is_contiguous()
        assert torch.equal(got.cpu(), oi.occlude_ref(other.cpu(), fill.to(other.dtype), patch, stride, j0, K))
    drops = oi.drops_for(B, len(wins))
    ref = oi.volume_ref64(drops, size, patch, stride)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlusion_volume(drops.to(DEV), size, patch, stride))
    assert names == ["tmf_occlusion_volume"] and float(oi.row_errors(got.cpu(), ref).max()) <= oi.volume_tolerance(case)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlusion_volume(drops.to(DEV).double(), size, patch, stride))
    assert names == [] and float(oi.row_errors(got.cpu(), ref).max()) <= 1e-15
    vol, lab, fill = oi.atlas_inputs((16, 16, 16), 17)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlude_labels(vol.to(DEV), lab.to(DEV), fill.to(DEV), 17, 10, 9))
    assert names == ["tmf_occlude_labels"] and torch.equal(got.cpu(), oi.occlude_labels_ref(vol, lab, fill, 17, 10, 9))
    got, names, _w = _calls(monkeypatch, lambda: ops.occlude_labels(vol.to(DEV), lab.to(DEV).long(), fill.to(DEV), 17, 10, 9))
    assert names == [] and torch.equal(got.cpu(), oi.occlude_labels_ref(vol, lab, fill, 17, 10, 9))
    d = oi.drops_for(2, 17, seed=1)
    got, names, _w = _calls(monkeypatch, lambda: ops.occlusion_volume(d.to(DEV), (16, 16, 16), labels=lab.to(DEV)))
    assert names == ["tmf_occlusion_volume_labels"] and torch.equal(got.cpu(), oi.volume_labels_ref(d, lab, 17))


def _randomise_bn(net):
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.data.uniform_(0.5, 1.5)
                m.bias.data.normal_(0, 0.1)


@pytest.mark.parametrize("size", (16, 32))
def test_replay_is_neutral_and_replays(size, monkeypatch):
    """tmf_replay None (and an encoder that never had the attribute): the one-call eval forward, the same bits.  With a tensor:
    that tensor, no library call, the volume not read; a mismatched tensor raises; back at None the forward's bits again."""
    import transmf_ad_amd as T
    torch.manual_seed(11)
    enc = T.sNet(32).to(DEV)
    _randomise_bn(enc)
    enc.eval()
    old = copy.deepcopy(enc)
    del old.__dict__["tmf_replay"]                                       # a module from before the attribute existed
    vol = torch.rand((2, 1, size, size, size), device=DEV)
    with torch.no_grad():
        want, names, _w = _calls(monkeypatch, lambda: enc.forward_channels_last(vol))
        assert names.count("tmf_snet_eval_fwd") == 1 and enc.tmf_replay is None
        assert torch.equal(old.forward_channels_last(vol), want)
        rep = torch.randn((5,) + tuple(want.shape[1:]), device=DEV)
        enc.tmf_replay = rep
        poison = torch.full((1, 1, size, size, size), float("nan"), device=DEV).expand(5, 1, size, size, size)
        got, names, _w = _calls(monkeypatch, lambda: enc.forward_channels_last(poison))
        assert got is rep and names == []
        assert torch.equal(enc(poison), rep.permute(0, 4, 1, 2, 3))
        for bad in (rep[:2], rep[..., :16], rep[:, :, :, :0]):
            enc.tmf_replay = bad
            with pytest.raises(ValueError, match="tmf_replay"):
                enc.forward_channels_last(poison)
        enc.tmf_replay = None
        again, names, _w = _calls(monkeypatch, lambda: enc.forward_channels_last(vol))
    assert names.count("tmf_snet_eval_fwd") == 1 and torch.equal(again, want)


# ---------------------------------------------------------------------------------------------------------------------
# occlusion_sensitivity against the model's own forward
# ---------------------------------------------------------------------------------------------------------------------

def _model(kind):
    import transmf_ad_amd as T
    torch.manual_seed(5)
    if kind == "cnn32":
        net, size = T.model_CNN_ad(dim=32), (16, 16, 16)
    elif kind == "ad128":
        net, size = T.model_ad(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512, dropout=0.), (32, 32, 32)
    else:
        net, size = T.model_single(dim=128), (32, 32, 32)
    _randomise_bn(net)
    mri, pet, _y = P.make_inputs(2, size, seed=77, kind="blobs")
    return net.to(DEV).eval(), torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV), size


def _score(logits, target, score="logit"):
    s = logits if score == "logit" else torch.softmax(logits, 1)
    return s.gather(1, target.view(-1, 1))[:, 0]


def _loop(net, vols, which, masks, fills, target, chunk, score="logit"):
    """The user's loop through the model's own forward: clone() and assignment of `masks[w]` (slices or a bool volume) in the
    volumes `which`, in chunks of `chunk` jobs -> (drops (B, nW), the logits of every job (B, nW, classes), base logits)."""
    B, nW = vols[0].shape[0], len(masks)
    with torch.no_grad():
        base = net(*vols)
        base = base[0] if isinstance(base, tuple) else base
        outs = []
        for j0 in range(0, B * nW, chunk):
            jobs = range(j0, min(j0 + chunk, B * nW))
            rows = torch.tensor([j // nW for j in jobs], device=DEV)
            batch = [v.index_select(0, rows).clone() for v in vols]
            for k, j in enumerate(jobs):
                for i in which:
                    batch[i][k, 0][masks[j % nW]] = fills[i][j // nW]
            out = net(*batch)
            outs.append(out[0] if isinstance(out, tuple) else out)
        jobs = torch.cat(outs)
    rows = torch.arange(B * nW, device=DEV) // nW
    drops = _score(base, target, score).index_select(0, rows) - _score(jobs, target.index_select(0, rows), score)
    return drops.view(B, nW), jobs.view(B, nW, -1), base


def _slices(size, patch, stride):
    wins, grid = oi.windows(size, oi.triple(patch), oi.triple(stride))
    return [(slice(a, b), slice(c, d), slice(e, f)) for a, b, c, d, e, f in wins], grid


def _bits_follow_the_batch(enc, vol, nW, chunk):
    """Whether the eval encoder gives some sample other bits in a chunk's batch than in the batch of the volumes themselves."""
    B = vol.shape[0]
    with torch.no_grad():
        base = enc(vol)
        for j0 in range(0, B * nW, chunk):
            rows = torch.arange(j0, min(j0 + chunk, B * nW), device=DEV) // nW
            if not torch.equal(enc(vol.index_select(0, rows)), base.index_select(0, rows)):
                return True
    return False


@pytest.mark.parametrize("kind", ("cnn32", "ad128"))
def test_occlusion_sensitivity_is_the_models_own_forward(kind, monkeypatch):
    """reuse=False: the drops are, bit for bit, score(model(base)) - score(model(batch)) on batches the test builds itself with
    clone() and slice assignment in the same chunks; one occlude launch per chunk, one voxel-map launch per map.  reuse=True:
    the encoder of the volume that is not occluded runs in the baseline forward only."""
    import transmf_ad_amd as T
    net, mri, pet, size = _model(kind)
    patch, chunk = size[0] // 2, 5
    masks, grid = _slices(size, patch, patch)
    nW, zero = len(masks), [torch.zeros(2, device=DEV)] * 2
    nchunks = -(-2 * nW // chunk)
    keep = {k: v.clone() for k, v in net.state_dict().items()}
    rng = torch.cuda.get_rng_state(0)
    occ, names, wrappers = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, mri, pet, patch=patch, chunk=chunk, reuse=False))
    assert names.count("tmf_occlude_windows") == wrappers.count("occlude_windows") == 2 * nchunks
    assert names.count("tmf_occlusion_volume") == wrappers.count("occlusion_volume") == 2
    assert names.count("tmf_snet_eval_fwd") == 2 + 2 * 2 * nchunks
    target = occ.logits.argmax(1)
    assert torch.equal(occ.target, target) and occ.grid == grid and occ.volumes == (0, 1)
    for i in (0, 1):
        drops, _jobs, base = _loop(net, [mri, pet], (i,), masks, zero, target, chunk)
        assert torch.equal(occ.logits, base) and torch.equal(occ.base_score, _score(base, target))
        assert torch.equal(occ.drops(i).reshape(2, -1), drops), i
        assert float(drops.abs().max()) > 0
        gathered = torch.zeros((2,) + size, device=DEV)
        for w, m in enumerate(masks):
            gathered[(slice(None), *m)] = drops[:, w].view(2, 1, 1, 1)
        assert torch.equal(occ.volume(i), gathered)
    re, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, mri, pet, patch=patch, chunk=chunk, reuse=True))
    assert names.count("tmf_snet_eval_fwd") == 2 + 2 * nchunks and names.count("tmf_occlude_windows") == 2 * nchunks
    assert net.mri_cnn.tmf_replay is None and net.pet_cnn.tmf_replay is None
    for i in (0, 1):
        diff = float((re.drops(i) - occ.drops(i)).abs().max())
        print(f"{kind} volume {i}: max |drops(reuse=True) - drops(reuse=False)| = {diff:.3e} of max |drop| "
              f"{float(occ.drops(i).abs().max()):.3e}")
        # bit for bit where the kept encoder gives a sample the same bits in the baseline batch as in a chunk's batch; where it
        # does not (its kernels' plans follow the batch size), no number is picked here: both runs are held to the reference's
        # drops under the fixture's tolerance in test_occlusion_sensitivity_against_the_reference
        same = torch.equal(re.drops(i), occ.drops(i)) and torch.equal(re.volume(i), occ.volume(i))
        kept_enc, kept_vol = ((net.pet_cnn, pet), (net.mri_cnn, mri))[i]
        assert same or _bits_follow_the_batch(kept_enc, kept_vol, nW, chunk), i
    joint, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, mri, pet, patch=patch, chunk=chunk, joint=True))
    assert names.count("tmf_snet_eval_fwd") == 2 + 2 * nchunks and names.count("tmf_occlusion_volume") == 1      # nothing to reuse
    drops, _jobs, _base = _loop(net, [mri, pet], (0, 1), masks, zero, target, chunk)
    assert torch.equal(joint.drops().reshape(2, -1), drops) and torch.equal(joint.drops(0), joint.drops(1))
    seen = []

    def stop(_mod, _args):                                              # the model raises in the first chunk, the replay being set
        seen.append(net.pet_cnn.tmf_replay is not None)
        if len(seen) == 2:
            raise RuntimeError("stop")
    h = net.mri_cnn.register_forward_pre_hook(stop)
    with pytest.raises(RuntimeError, match="stop"):
        T.occlusion_sensitivity(net, mri, pet, patch=patch, volumes=(0,))
    h.remove()
    assert seen == [False, True] and net.mri_cnn.tmf_replay is None and net.pet_cnn.tmf_replay is None
    with pytest.raises(ValueError, match="eval"):
        T.occlusion_sensitivity(net.train(), mri, pet, patch=patch)
    net.eval()
    assert all(torch.equal(v, keep[k]) for k, v in net.state_dict().items())
    assert torch.equal(torch.cuda.get_rng_state(0), rng) and all(p.grad is None for p in net.parameters())


def test_options_on_the_device(monkeypatch):
    """model_single with one volume (nothing to reuse); an atlas; score="prob"; fill="mean" and a fill tensor; overlap; all bit
    for bit the model's own forward on test-built batches.  A non-contiguous volume and a float64 module take the torch ops."""
    import transmf_ad_amd as T
    net, mri, _pet, size = _model("single")
    target = torch.tensor([1, 0], device=DEV)
    masks, grid = _slices(size, 16, 8)
    mean = [mri.reshape(2, -1).mean(1)]
    occ, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, mri, patch=16, stride=8, fill="mean", score="prob",
                                                                         target=target, chunk=20))
    assert names.count("tmf_occlude_windows") == 3 and names.count("tmf_snet_eval_fwd") == 1 + 3 and occ.grid == grid == (3, 3, 3)
    drops, _jobs, _base = _loop(net, [mri], (0,), masks, mean, target, 20, "prob")
    assert torch.equal(occ.drops().reshape(2, -1), drops) and occ.volumes == (0,)
    ref = oi.volume_ref64(drops.cpu(), size, (16,) * 3, (8,) * 3)             # up to 8 windows per voxel
    D = float(oi.row_errors(oi.volume_formula32(drops.cpu(), size, (16,) * 3, (8,) * 3), ref).max())
    assert float(oi.row_errors(occ.volume().cpu(), ref).max()) <= oi.MARGIN * max(D, oi.VOLUME_FLOOR)
    g = torch.Generator().manual_seed(2)
    atlas = torch.randint(0, 6, size, generator=g)
    atlas[atlas == 4] = 0
    fill = torch.tensor([0.5, -0.25])
    occ, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, mri, atlas=atlas, fill=fill, target=target, chunk=4))
    assert names.count("tmf_occlude_labels") == 3 and names.count("tmf_occlusion_volume_labels") == 1 and occ.grid is None
    lab = atlas.to(DEV)
    drops, _jobs, _base = _loop(net, [mri], (0,), [lab == r for r in range(1, 6)], [fill.to(DEV)], target, 4)
    assert torch.equal(occ.drops(), drops) and float(drops[:, 3].abs().max()) == 0 and float(drops.abs().max()) > 0
    assert torch.equal(occ.volume().cpu(), oi.volume_labels_ref(drops.cpu(), atlas, 5))
    # a non-contiguous volume: no occlude launch, the same bits as its contiguous copy
    wide = torch.zeros((2, 1) + size[:2] + (2 * size[2],), device=DEV)
    wide[..., ::2] = mri
    masks, _grid = _slices(size, 16, 16)
    a, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(net, wide[..., ::2], patch=16, target=target))
    b = T.occlusion_sensitivity(net, mri, patch=16, target=target)
    assert "tmf_occlude_windows" not in names and names.count("tmf_occlusion_volume") == 1
    assert torch.equal(a.drops(), b.drops()) and torch.equal(a.volume(), b.volume())

    class Lin(torch.nn.Module):                                         # a foreign float64 module on the device
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.randn((3, 16 ** 3), dtype=torch.float64))

        def forward(self, x, y):
            return torch.tanh((x - y).flatten(1) @ self.w.t() / 30)

    lin = Lin().to(DEV).eval()
    x, y = torch.rand((2, 1, 16, 16, 16), device=DEV, dtype=torch.float64), torch.rand((2, 1, 16, 16, 16), device=DEV, dtype=torch.float64)
    a, names, _w = _calls(monkeypatch, lambda: T.occlusion_sensitivity(lin, x, y, patch=8, stride=4, chunk=9))
    b = T.occlusion_sensitivity_torch(lin, x, y, patch=8, stride=4, chunk=9)
    assert names == [] and a.drops(0).dtype == torch.float64
    for i in (0, 1):
        assert torch.equal(a.drops(i), b.drops(i)) and torch.equal(a.volume(i), b.volume(i))


# ---------------------------------------------------------------------------------------------------------------------
# against the reference's own drops
# ---------------------------------------------------------------------------------------------------------------------

SETTINGS = {"p8": (8, 8), "p16": (16, 16), "p16s8": (16, 8)}


@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_occlusion_sensitivity_against_the_reference(name):
    """Window order, sign, fill and target as stored.  E = the worst |logits - fp64 logits| of the EXISTING eval forward over the
    base volumes and all occluded jobs the test builds itself; per sample |drop - drop64| <= max(MARGIN x dist x max |drop64|,
    2 E) (a drop is the difference of two logits), and the comparison means something only where 2 E <= 0.05 max |drop64|."""
    import transmf_ad_amd as T
    z = np.load(os.path.join(GOLDEN_DIR, f"occlusion_{name}.npz"))
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    vols = [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)]
    target = torch.from_numpy(z["target"]).to(DEV)
    B, zero = g.batch, [torch.zeros(g.batch, device=DEV)] * 2
    assert str(z["settings"]).split(",") == list(SETTINGS)
    E, loops = 0.0, {}
    for s, (patch, stride) in SETTINGS.items():
        masks, grid = _slices(g.size, patch, stride)
        for m, mod in enumerate(("mri", "pet")):
            drops, jobs, base = _loop(net, vols, (m,), masks, zero, target, 32)
            E = max(E, float((jobs.cpu().double() - torch.from_numpy(z[f"{s}.{mod}.logits"])).abs().max()),
                    float((base.cpu().double() - torch.from_numpy(z["logits"])).abs().max()))
            loops[(s, mod)] = drops
    print(f"{name}: E = {E:.3e}")
    bad = []
    for s, (patch, stride) in SETTINGS.items():
        for reuse in (False, True):
            occ = T.occlusion_sensitivity(net, *vols, patch=patch, stride=stride, target=target, reuse=reuse)
            for m, mod in enumerate(("mri", "pet")):
                key = f"{s}.{mod}"
                want, peak = torch.from_numpy(z[key + ".drops"]), torch.from_numpy(z["max." + key])
                got = occ.drops(m).cpu().double()
                assert got.shape == want.shape
                err = (got - want).abs().reshape(B, -1).amax(1)
                tol = torch.maximum(oi.MARGIN * float(z["dist." + key]) * peak, torch.full_like(peak, 2 * E))
                own = float((occ.drops(m).reshape(B, -1) - loops[(s, mod)]).abs().max())
                print(f"{name} {key} reuse={reuse}: err {err.tolist()} tol {tol.tolist()} max |drop64| {peak.tolist()} "
                      f"2E / max {(2 * E / peak).tolist()}; against the own loop {own:.3e}")
                if not bool((err <= tol).all()):
                    bad.append((key, reuse, "error", (err / tol).max().item()))
                if not bool((2 * E <= 0.05 * peak).all()):
                    bad.append((key, reuse, "2E above 5 % of the drops", (2 * E / peak).max().item()))
    assert not bad, bad
