"""Deletion / insertion curves on the device: the kernels of csrc/faithfulness.hip on their own (through _lib.call with raw
pointers) against a float32 torch.sort and torch.where (tests/_faithfulness_inputs.py), bit for bit; their refusals;
faithfulness_curve against the test's own loop around the model's forward (bit for bit), with and without encoder reuse; against
the curves the reference itself gives (tests/golden/faithfulness_*.npz).

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs
included) must be unchanged, every output element written."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _faithfulness_inputs as fi
from _golden import GOLDEN_DIR, Golden
from _occlusion_inputs import MARGIN
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _query, _st
from test_gpu_model import DEV, build
from test_gpu_occlusion import _model, _score

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32


def _counts(c):
    return (ctypes.c_int * len(c))(*c)


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through raw pointers
# ---------------------------------------------------------------------------------------------------------------------

def _rank_case(B, V, kind, steps_list):
    """thr as bits and removed exactly against the sorted row, for every steps of the list, each twice: equal bits."""
    attr = fi.values(kind, B, V)
    outs, nws = {}, 0
    for S in steps_list:
        for r in (0, 1):
            outs[f"thr{S}.{r}"], outs[f"rem{S}.{r}"] = ((B, S), F32), ((B, S), I32)
        nws = max(nws, _query("tmf_rank_workspace_bytes", B, V, S))
    assert nws > 0
    outs["ws"] = ((nws,), torch.uint8)
    ar = Arena(dict(attr=attr), outs, tail=4096)
    for S in steps_list:
        counts = fi.counts_ref(V, S)
        for r in (0, 1):
            _call("tmf_rank_thresholds", ar.ptr("attr"), _counts(counts), ar.ptr(f"thr{S}.{r}"), ar.ptr(f"rem{S}.{r}"), ar.ptr("ws"),
                  nws, B, V, S, _st())
    got = ar.fetch(may_nan=[k for k in outs if k.startswith("thr")], workspace=("ws",))
    for S in steps_list:
        counts = fi.counts_ref(V, S)
        thr, removed = fi.thresholds_ref(attr, counts)
        for r in (0, 1):
            assert torch.equal(fi.bits(got[f"thr{S}.{r}"]), fi.bits(thr)), (kind, S, r)
            assert torch.equal(got[f"rem{S}.{r}"], removed), (kind, S, r)
        assert bool((removed >= torch.tensor(counts, dtype=I32)).all())
        if kind == "permutation":
            assert torch.equal(removed, torch.tensor(counts, dtype=I32).expand(B, S))
        if kind == "equal":
            assert bool((removed == V).all()) and bool((thr == thr[0, 0]).all())


@pytest.mark.parametrize("kind", fi.VALUE_SETS)
@pytest.mark.parametrize("shape", fi.RANK_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_rank_thresholds_kernel(shape, kind):
    _rank_case(*shape, kind, fi.RANK_STEPS)


@pytest.mark.parametrize("kind", fi.VALUE_SETS)
def test_rank_thresholds_kernel_repeated_counts(kind):
    (B, V), S = fi.REPEATING
    assert len(set(fi.counts_ref(V, S))) == V < S
    _rank_case(B, V, kind, (S,))


@pytest.mark.parametrize("case", fi.MASK_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mask_by_rank_kernel(case):
    """torch.equal with torch.where for both modes, fill and base, K = 1 (s = 0 and s = S), a chunk that crosses into the next
    sample, the short last chunk and all jobs; thresholds with ties and -0.0 in the attribution; the 16-byte path where
    V % 4 == 0 (the arena's slots are 256-byte aligned), the scalar path otherwise and, on the % 4 == 0 case, once more through
    an output that starts 4 bytes off."""
    B, V, S = case
    vol, attr, thr, fill, base = fi.mask_inputs(B, V, S)
    assert V < 4096 or len(set(thr[0].tolist())) < S, "the larger cases have tied thresholds"
    chunks = fi.chunkings(B, S)
    runs = [(mode, f, i) for mode in fi.MODES for f in ("fill", "base") for i in range(len(chunks))]
    outs = {f"{mode}.{f}.{i}": ((chunks[i][1], V), F32) for mode, f, i in runs}
    shifted = V % 4 == 0
    if shifted:
        outs["off"] = ((chunks[2][1] * V + 1,), F32)
    ar = Arena(dict(vol=vol, attr=attr, thr=thr, fill=fill, base=base), outs, tail=4096)
    mode_code = {"deletion": 0, "insertion": 1}
    for mode, f, i in runs:
        j0, K = chunks[i]
        _call("tmf_mask_by_rank", ar.ptr("vol"), ar.ptr("attr"), ar.ptr("thr"), ar.ptr("fill") if f == "fill" else None,
              ar.ptr("base") if f == "base" else None, ar.ptr(f"{mode}.{f}.{i}"), B, V, S, mode_code[mode], j0, K, _st())
    written = None
    if shifted:
        j0, K = chunks[2]
        _call("tmf_mask_by_rank", ar.ptr("vol"), ar.ptr("attr"), ar.ptr("thr"), ar.ptr("fill"), None, ar.ptr("off") + 4, B, V, S, 0,
              j0, K, _st())
        written = {"off": torch.ones(K * V + 1, dtype=torch.bool)}
        written["off"][0] = False
    got = ar.fetch(written=written)
    for mode, f, i in runs:
        j0, K = chunks[i]
        want = fi.mask_ref(vol, attr, thr, fill, mode, j0, K, base=base if f == "base" else None)
        assert torch.equal(got[f"{mode}.{f}.{i}"], want), (mode, f, j0, K)
    j0, K = chunks[0]
    assert torch.equal(got["deletion.fill.0"][0], vol[0]) and bool((got["insertion.fill.0"][0] == fill[0]).all())     # s = 0
    if shifted:
        j0, K = chunks[2]
        assert torch.equal(got["off"][1:].view(K, V), fi.mask_ref(vol, attr, thr, fill, "deletion", j0, K))


def test_entries_refuse_before_any_launch():
    """Bad arguments on real buffers full of a sentinel: a negative code, every buffer unchanged, the entry named."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    B, V, S = 2, 512, 4
    src = torch.full((B * V + 64,), 7.0, device=DEV)
    dst = torch.full((B * (S + 1) * V + 64,), 7.0, device=DEV)
    thr = torch.full((B * 64,), 7.0, device=DEV)
    rem = torch.full((B * 64,), 7, device=DEV, dtype=I32)
    nws = lib.tmf_rank_workspace_bytes(B, V, 64)
    ws = torch.full((nws,), 7, device=DEV, dtype=torch.uint8)
    p, q, t, r, w = (x.data_ptr() for x in (src, dst, thr, rem, ws))
    neg = lambda rc: rc < 0
    ok = _counts(fi.counts_ref(V, S))
    for args in ((None, ok, t, r, w), (p, None, t, r, w), (p, ok, None, r, w), (p, ok, t, None, w), (p, ok, t, r, None)):
        assert neg(lib.tmf_rank_thresholds(*args, nws, B, V, S, None))
    assert neg(lib.tmf_rank_thresholds(p, _counts([1]), t, r, w, nws, B, V, 0, None))
    assert neg(lib.tmf_rank_thresholds(p, _counts(fi.counts_ref(V, 64) + [V]), t, r, w, nws, B, V, 65, None))
    for bad in ([3, 2, 4, 5], [0, 1, 2, 3], [1, 2, 3, V + 1], [-1, 2, 3, 4]):
        assert neg(lib.tmf_rank_thresholds(p, _counts(bad), t, r, w, nws, B, V, S, None)), bad
    for b, v in ((0, V), (-1, V), (B, 0), (B, -5), (B, 1 << 31), (1 << 17, V)):
        assert neg(lib.tmf_rank_thresholds(p, ok, t, r, w, nws, b, v, S, None)), (b, v)
    assert neg(lib.tmf_rank_thresholds(p, ok, t, r, w, lib.tmf_rank_workspace_bytes(B, V, S) - 1, B, V, S, None))
    for args in ((p + 2, ok, t, r, w), (p, ok, t + 1, r, w), (p, ok, t, r + 2, w), (p, ok, t, r, w + 3)):
        assert neg(lib.tmf_rank_thresholds(*args, nws, B, V, S, None))
    assert b"tmf_rank_thresholds" in lib.tmf_last_error_string()
    assert lib.tmf_rank_workspace_bytes(B, V, 0) == 0 == lib.tmf_rank_workspace_bytes(0, V, S) == lib.tmf_rank_workspace_bytes(B, V, 65)
    for args in ((None, p, t, p, None, q), (p, None, t, p, None, q), (p, p, None, p, None, q), (p, p, t, None, None, q),
                 (p, p, t, p, None, None)):
        assert neg(lib.tmf_mask_by_rank(*args, B, V, S, 0, 0, 1, None))
    for s in (0, 65, -1):
        assert neg(lib.tmf_mask_by_rank(p, p, t, p, None, q, B, V, s, 0, 0, 1, None))
    for mode in (-1, 2):
        assert neg(lib.tmf_mask_by_rank(p, p, t, p, None, q, B, V, S, mode, 0, 1, None))
    for j0, K in ((0, 0), (0, -1), (-1, 1), (10, 1), (8, 3), (0, 11), ((1 << 31) - 1, 1), (0, 1 << 17)):
        assert neg(lib.tmf_mask_by_rank(p, p, t, p, None, q, B, V, S, 0, j0, K, None)), (j0, K)
    for b, v in ((0, V), (-1, V), (B, 0), (B, 1 << 31), (1 << 30, V)):
        assert neg(lib.tmf_mask_by_rank(p, p, t, p, None, q, b, v, S, 0, 0, 1, None)), (b, v)
    for args in ((p + 2, p, t, p, None, q), (p, p + 1, t, p, None, q), (p, p, t + 2, p, None, q), (p, p, t, p + 3, None, q),
                 (p, p, t, p, p + 2, q), (p, p, t, p, None, q + 1)):
        assert neg(lib.tmf_mask_by_rank(*args, B, V, S, 0, 0, 1, None))
    assert b"tmf_mask_by_rank" in lib.tmf_last_error_string()
    torch.cuda.synchronize()
    assert bool((src == 7.0).all()) and bool((dst == 7.0).all()) and bool((thr == 7.0).all())
    assert bool((rem == 7).all()) and bool((ws == 7).all())


# ---------------------------------------------------------------------------------------------------------------------
# the ops wrappers
# ---------------------------------------------------------------------------------------------------------------------

def _calls(monkeypatch, fn):
    """fn() -> (its result, the library entries it called in order)."""
    from transmf_ad_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


def test_ops_wrappers_route(monkeypatch):
    """Contiguous float32 HIP tensors take the kernels (one call each), anything else the torch formulas: the same values."""
    from transmf_ad_amd import ops
    B, V, S = fi.MASK_CASES[1]
    vol, attr, thr, fill, base = fi.mask_inputs(B, V, S)
    counts = ops.rank_counts(V, S)
    assert counts == fi.counts_ref(V, S)
    want_thr, want_rem = fi.thresholds_ref(attr, counts)
    v, a, f, bs = (x.to(DEV) for x in (vol.view(B, 1, 16, 16, 16), attr.view(B, 16, 16, 16), fill, base.view(B, 1, 16, 16, 16)))
    assert ops.faithfulness_ok(v, a, f) and not ops.faithfulness_ok(vol) and not ops.faithfulness_ok(v.double())
    (t, r), names = _calls(monkeypatch, lambda: ops.rank_thresholds(a, counts))
    assert names == ["tmf_rank_thresholds"] and torch.equal(fi.bits(t.cpu()), fi.bits(want_thr)) and torch.equal(r.cpu(), want_rem)
    for other in (a.double(), a[:, :, :, ::2]):
        (t2, r2), names = _calls(monkeypatch, lambda: ops.rank_thresholds(other, ops.rank_counts(other[0].numel(), S)))
        assert names == [] and t2.dtype == other.dtype
    (t2, r2), names = _calls(monkeypatch, lambda: ops.rank_thresholds(a.double(), counts))
    assert torch.equal(t2.cpu(), want_thr.double()) and torch.equal(r2.cpu(), want_rem)
    j0, K = fi.chunkings(B, S)[2]
    for mode in fi.MODES:
        for b_ in (None, bs):
            want = fi.mask_ref(vol, attr, thr, fill, mode, j0, K, base=None if b_ is None else base).view(K, 1, 16, 16, 16)
            got, names = _calls(monkeypatch, lambda: ops.mask_by_rank(v, a, t, f, mode, j0, K, base=b_))
            assert names == ["tmf_mask_by_rank"] and torch.equal(got.cpu(), want)
            got, names = _calls(monkeypatch, lambda: ops.mask_by_rank(v.double(), a, t, f, mode, j0, K,
                                                                      base=None if b_ is None else b_.double()))
            assert names == [] and got.dtype == torch.float64 and torch.equal(got.cpu(), want.double())
    buf = torch.empty((K + 3, 1, 16, 16, 16), device=DEV)
    got, names = _calls(monkeypatch, lambda: ops.mask_by_rank(v, a, t, f, "deletion", j0, K, out=buf[:K]))
    assert names == ["tmf_mask_by_rank"] and got.data_ptr() == buf.data_ptr()


# ---------------------------------------------------------------------------------------------------------------------
# faithfulness_curve against the test's own loop
# ---------------------------------------------------------------------------------------------------------------------

def _attribution(size, B, ties):
    a_mri, a_pet, _y = P.make_inputs(B, size, seed=4321, kind="blobs")
    out = [torch.from_numpy(a).float() for a in (a_mri, a_pet)]
    return [(torch.floor(a * 16) / 16 if ties else a).to(DEV) for a in out]


def _golden_model(name):
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    return g, net, [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)]


class _Count:
    """The forwards of each encoder that really ran: a call that returned its tmf_replay is not one."""

    def __init__(self, *mods):
        self.n = [0] * len(mods)
        self.hooks = [m.register_forward_hook(lambda mod, _a, _o, i=i: self.n.__setitem__(i, self.n[i] + (mod.tmf_replay is None)))
                      for i, m in enumerate(mods)]

    def take(self):
        n, self.n = self.n, [0] * len(self.n)
        return n

    def remove(self):
        for h in self.hooks:
            h.remove()


@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_faithfulness_curve_is_the_models_own_forward(name, monkeypatch):
    """32^3, B = 2, each modality and both modes: with reuse on and off the scores are, bit for bit, the scores of the model's
    forward on batches the test builds itself with torch.sort and torch.where in the same chunks; removed and thresholds equal;
    one rank call per curve, one mask launch per chunk; with reuse the untouched modality's encoder runs once."""
    import transmf_ad_amd as T
    g, net, vols = _golden_model(name)
    B, S, chunk = g.batch, 8, 7
    assert tuple(g.size) == (32, 32, 32) and B == 2
    attrs = _attribution(g.size, B, ties=True)
    zero = torch.zeros(B, device=DEV)
    nchunks = -(-B * (S + 1) // chunk)
    encs = (net.mri_cnn, net.pet_cnn)
    keep = {k: v.clone() for k, v in net.state_dict().items()}
    rng = torch.cuda.get_rng_state(0)
    with torch.no_grad():
        base_logits = net(*vols)[0]
    target = base_logits.argmax(1)
    count = _Count(*encs)
    for m in (0, 1):
        for mode in fi.MODES:
            scores, removed, thr, _jobs, logits = fi.curve_loop(net, vols, m, attrs[m], S, mode, zero, None, target, chunk, "logit")
            count.take()
            assert float((scores.amax(1) - scores.amin(1)).min()) > 0
            for reuse in (False, True):
                fc, names = _calls(monkeypatch, lambda: T.faithfulness_curve(net, *vols, attribution=attrs[m], volume=m, steps=S,
                                                                             mode=mode, score="logit", chunk=chunk, reuse=reuse))
                n = count.take()
                print(f"{name} volume {m} {mode} reuse={reuse}: max |scores - own loop| = {float((fc.scores - scores).abs().max()):.3e}"
                      f" of range {float((scores.amax(1) - scores.amin(1)).min()):.3e}; encoder forwards {n}")
                assert names.count("tmf_rank_thresholds") == 1 and names.count("tmf_mask_by_rank") == nchunks
                assert n[m] == 1 + nchunks and n[1 - m] == (1 if reuse else 1 + nchunks), (n, reuse)
                assert torch.equal(fc.logits, logits) and torch.equal(fc.target, target)
                assert torch.equal(fc.base_score, _score(logits, target))
                assert torch.equal(fc.removed, removed) and fc.removed.dtype == I32 and bool((fc.removed[:, 0] == 0).all())
                assert torch.equal(fi.bits(fc.thresholds), fi.bits(thr))
                assert torch.equal(fc.scores, scores), (m, mode, reuse, float((fc.scores - scores).abs().max()))
                assert float((fc.auc.cpu().double() - fi.auc_ref(scores.cpu())).abs().max()) <= 1e-6 * float(scores.abs().max())
                assert (fc.steps, fc.mode, fc.volume) == (S, mode, m)
                assert encs[0].tmf_replay is None and encs[1].tmf_replay is None
    count.remove()
    seen = []

    def stop(_mod, _args):                                              # the model raises in the first chunk, the replay being set
        seen.append(net.pet_cnn.tmf_replay is not None)
        if len(seen) == 2:
            raise RuntimeError("stop")
    h = net.mri_cnn.register_forward_pre_hook(stop)
    with pytest.raises(RuntimeError, match="stop"):
        T.faithfulness_curve(net, *vols, attribution=attrs[0], volume=0, steps=S)
    h.remove()
    assert seen == [False, True] and net.mri_cnn.tmf_replay is None and net.pet_cnn.tmf_replay is None
    with pytest.raises(ValueError, match="eval"):
        T.faithfulness_curve(net.train(), *vols, attribution=attrs[0], steps=S)
    net.eval()
    assert all(torch.equal(v, keep[k]) for k, v in net.state_dict().items())
    assert torch.equal(torch.cuda.get_rng_state(0), rng) and all(p.grad is None for p in net.parameters())


@pytest.mark.parametrize("chunk", (1, 7, 32))
def test_options_on_the_device(chunk, monkeypatch):
    """score="prob" with fill="mean" and an explicit target; a baseline tensor (it overrides fill) with a fill tensor; the
    attribution with a channel axis; all bit for bit the test's own loop, in chunks of 1, 7 and 32.  reuse=False here: at dim 128
    the kept encoder's bits follow its batch size (tests/test_gpu_occlusion.py), so a replayed baseline output of batch 2 is
    not the bits of a chunk of 1; reuse is held to the loop on the tiny models above and to the reference below."""
    import transmf_ad_amd as T
    net, mri, pet, size = _model("ad128")
    B, S = 2, 5
    attrs = _attribution(size, B, ties=False)
    target = torch.tensor([1, 0], device=DEV)
    mean = pet.reshape(B, -1).mean(1)
    scores, removed, thr, _j, _l = fi.curve_loop(net, [mri, pet], 1, attrs[1], S, "insertion", mean, None, target, chunk, "prob")
    fc, names = _calls(monkeypatch, lambda: T.faithfulness_curve(net, mri, pet, attribution=attrs[1][:, 0], volume=1, steps=S,
                                                                 mode="insertion", fill="mean", target=target, chunk=chunk,
                                                                 reuse=False))
    assert names.count("tmf_mask_by_rank") == -(-B * (S + 1) // chunk)
    assert torch.equal(fc.scores, scores) and torch.equal(fc.removed, removed) and torch.equal(fc.target, target)
    assert bool(((fc.scores > 0) & (fc.scores < 1)).all())
    blur = torch.nn.functional.avg_pool3d(mri, 5, stride=1, padding=2)
    fill = torch.tensor([0.5, -0.25], device=DEV)
    scores, removed, thr, _j, _l = fi.curve_loop(net, [mri, pet], 0, attrs[0], S, "deletion", fill, blur, target, chunk, "logit")
    fc = T.faithfulness_curve(net, mri, pet, attribution=attrs[0], volume=0, steps=S, mode="deletion", fill=fill, baseline=blur,
                              score="logit", target=target, chunk=chunk, reuse=False)
    assert torch.equal(fc.scores, scores) and torch.equal(fc.removed, removed)
    other = T.faithfulness_curve(net, mri, pet, attribution=attrs[0], volume=0, steps=S, mode="deletion", fill=fill,
                                 score="logit", target=target, chunk=chunk, reuse=False)
    assert not torch.equal(other.scores[:, 1:S], fc.scores[:, 1:S]) and torch.equal(other.scores[:, 0], fc.scores[:, 0])


# ---------------------------------------------------------------------------------------------------------------------
# against the reference's own curves
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_faithfulness_curve_against_the_reference(name):
    """Per sample D = max |score - score64| <= max(MARGIN x dist x range, E), E = the worst |logits - fp64 logits| of the EXISTING
    eval forward over the unmasked volumes and all jobs the test builds itself, against the stored job logits; the comparison
    means something only where E <= 0.05 range; removed equals the stored values."""
    import transmf_ad_amd as T
    z = np.load(os.path.join(GOLDEN_DIR, f"faithfulness_{name}.npz"))
    g, net, vols = _golden_model(name)
    B, S = g.batch, 8
    target = torch.from_numpy(z["target"]).to(DEV)
    zero = torch.zeros(B, device=DEV)
    settings = str(z["settings"]).split(",")
    assert settings == ["smooth", "ties"]
    E, keys = 0.0, []
    for s in settings:
        attrs = _attribution(g.size, B, ties=s == "ties")
        for mode in fi.MODES:
            for m, mod in enumerate(("mri", "pet")):
                key = f"{s}.{mode}.{mod}"
                _sc, _rm, _th, jobs, base = fi.curve_loop(net, vols, m, attrs[m], S, mode, zero, None, target, 32, "logit")
                E = max(E, float((jobs.cpu().double() - torch.from_numpy(z[key + ".logits"])).abs().max()),
                        float((base.cpu().double() - torch.from_numpy(z["logits"])).abs().max()))
                keys.append((key, attrs[m], mode, m))
    print(f"{name}: E = {E:.3e}")
    bad = []
    for key, attr, mode, m in keys:
        want, span = torch.from_numpy(z[key + ".scores"]), torch.from_numpy(z["range." + key])
        for reuse in (False, True):
            fc = T.faithfulness_curve(net, *vols, attribution=attr, volume=m, steps=S, mode=mode, fill=0.0, score="logit",
                                      target=target, reuse=reuse)
            assert torch.equal(fc.removed.cpu(), torch.from_numpy(z[key + ".removed"])), key
            D = (fc.scores.cpu().double() - want).abs().amax(1)
            tol = torch.maximum(MARGIN * float(z["dist." + key]) * span, torch.full_like(span, E))
            print(f"{name} {key} reuse={reuse}: D {D.tolist()} tol {tol.tolist()} range {span.tolist()} E / range {(E / span).tolist()}")
            if not bool((D <= tol).all()):
                bad.append((key, reuse, "error", (D / tol).max().item()))
            if not bool((E <= 0.05 * span).all()):
                bad.append((key, reuse, "E above 5 % of the range", (E / span).max().item()))
    assert not bad, bad
