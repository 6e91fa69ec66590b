"""Class activation maps on the device: tmf_cam on its own (csrc/cam.hip, through _lib.call with raw pointers) against the
fp64 maps of tests/_gradcam_inputs.py at every case there; its refusals; the encoder tap sNet.tmf_tap against the untapped
encoder, bit for bit; grad_cam against grad_cam_torch on the same package model; grad_cam against the maps the reference itself
gives (tests/golden/gradcam_*.npz).

A map is judged per sample row: |kernel - fp64| <= MARGIN x max(D, CAM_FLOOR) x max |fp64 row|, D the recorded distance of the
fp32 torch formula from fp64 on the same case; a row whose fp64 maximum is 0 must be exact zeros.  Every buffer of the kernel
test lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs must be unchanged, every output element
written and finite, and the inputs are surrounded by NaN."""
import copy
import os

import numpy as np
import pytest
import torch

import _gradcam_inputs as gi
from _golden import GOLDEN_DIR, Golden
from _token_inputs import floor_distance
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _st
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu
CODE = {"gradcam": 0, "hirescam": 1}


# ---------------------------------------------------------------------------------------------------------------------
# tmf_cam through raw pointers
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", gi.CAM_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_cam_kernel_against_fp64(case):
    """Both methods; flags off, RELU, RELU | NORMALIZE with all outputs; then cam alone (weights and peak NULL) with flags off
    and RELU | NORMALIZE, a second full call, and the weights alone: the same bits every time."""
    from transmf_ad_amd import _lib
    B, V, C, _roles = case
    A, G = gi.cam_inputs(case)
    f32 = torch.float32
    outs, calls = {}, []
    nws = 0
    for method in gi.METHODS:
        n = _lib.query("tmf_cam_workspace_bytes", B, V, C, CODE[method])
        assert n > 0 and n % 256 == 0
        nws = max(nws, n)
        for tag, flags, weights, peak in [("f0", 0, True, True), ("f1", gi.RELU, True, True), ("f3", 3, True, True),
                                          ("f0only", 0, False, False), ("f3only", 3, False, False), ("f3again", 3, True, True)]:
            weights = weights and method == "gradcam"
            k = f"{method}.{tag}"
            outs[k + ".cam"] = ((B, V), f32)
            if weights:
                outs[k + ".weights"] = ((B, C), f32)
            if peak:
                outs[k + ".peak"] = ((B,), f32)
            calls.append((method, flags, k, True, weights, peak))
    outs["gradcam.wonly.weights"] = ((B, C), f32)
    calls.append(("gradcam", 0, "gradcam.wonly", False, True, False))
    outs["ws"] = ((nws,), torch.uint8)
    ar = Arena(dict(A=A, G=G), outs, tail=4096)
    for method, flags, k, cam, weights, peak in calls:
        _call("tmf_cam", ar.ptr("A"), ar.ptr("G"), ar.ptr(k + ".cam") if cam else None,
              ar.ptr(k + ".weights") if weights else None, ar.ptr(k + ".peak") if peak else None, ar.ptr("ws"), nws,
              B, V, C, CODE[method], flags, _st())
    got = ar.fetch(workspace=("ws",))
    worst = {}
    for method in gi.METHODS:
        for tag, flags in (("f0", 0), ("f1", gi.RELU), ("f3", 3)):
            k = f"{method}.{tag}"
            ref = gi.cam_ref(A, G, method, flags)
            res = dict(cam=got[k + ".cam"], weights=got.get(k + ".weights"), peak=got[k + ".peak"])
            ratios = gi.cam_ratios(res, ref, case, method, flags)
            print(f"{case[:3]} {k}: " + " ".join(f"{q} {r:.3f}" for q, r in ratios.items()))
            worst[k] = max(ratios.values())
            dead = ref["cam"].abs().max(1).values == 0
            assert bool((res["cam"][dead] == 0).all()) and bool((res["peak"][dead & (ref["peak"] == 0)] == 0).all())
            if flags & gi.NORMALIZE:            # the maximum of a live sample is exactly 1, nothing exceeds it
                top = res["cam"].max(1).values
                assert torch.equal(top[~dead], torch.ones_like(top[~dead])) and bool((res["cam"] >= 0).all())
        for a, b in (("f0only", "f0"), ("f3only", "f3"), ("f3again", "f3")):
            assert torch.equal(got[f"{method}.{a}.cam"], got[f"{method}.{b}.cam"]), (method, a)
        assert torch.equal(got[f"{method}.f3again.peak"], got[f"{method}.f3.peak"])
        assert torch.equal(got[f"{method}.f1.peak"], got[f"{method}.f3.peak"])
    for tag in ("f1", "f3", "f3again", "wonly"):
        assert torch.equal(got[f"gradcam.{tag}.weights"], got["gradcam.f0.weights"]), tag
    assert max(worst.values()) <= 1.0, worst


def test_cam_entry_refuses_before_any_launch():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    t = torch.full((4, 64, 64), 7.0, device=DEV)
    ws = torch.full((1 << 16,), 7.0, device=DEV)
    p, w, n = t.data_ptr(), ws.data_ptr(), ws.numel() * 4
    need = lib.tmf_cam_workspace_bytes(2, 16, 32, 0)
    assert 0 < need <= n
    ok = (2, 16, 32, 0, 3, None)                                        # B, V, C, method, flags, stream
    assert lib.tmf_cam(p, p, None, None, None, w, n, *ok) < 0                           # cam and weights both NULL
    assert lib.tmf_cam(p, p, None, None, p, w, n, *ok) < 0                              # ... peak alone does not count
    assert lib.tmf_cam(None, p, p, p, p, w, n, *ok) < 0 and lib.tmf_cam(p, None, p, p, p, w, n, *ok) < 0
    assert lib.tmf_cam(p, p, p, p, p, None, n, *ok) < 0                                 # no workspace
    assert lib.tmf_cam(p + 4, p, p, p, p, w, n, *ok) < 0                                # alignment of act
    assert lib.tmf_cam(p, p + 8, p, p, p, w, n, *ok) < 0                                # ... of grad
    assert lib.tmf_cam(p, p, p, p, p, w + 4, n, *ok) < 0                                # ... of the workspace
    assert lib.tmf_cam(p, p, p + 2, p, p, w, n, *ok) < 0                                # ... of an output
    for C in (0, 4, 6, 30, 516, 1024, -8):
        assert lib.tmf_cam(p, p, p, p, p, w, n, 2, 16, C, 0, 3, None) < 0, C            # unsupported C
        assert lib.tmf_cam_ok(C) == 0 and lib.tmf_cam_workspace_bytes(2, 16, C, 0) == 0
    assert all(lib.tmf_cam_ok(C) == 1 for C in (8, 12, 16, 32, 64, 128, 256, 508, 512))
    assert lib.tmf_cam(p, p, p, p, p, w, n, 0, 16, 32, 0, 3, None) < 0                  # B
    assert lib.tmf_cam(p, p, p, p, p, w, n, 2, 0, 32, 0, 3, None) < 0                   # V
    assert lib.tmf_cam(p, p, p, p, p, w, need - 1, *ok) < 0                             # workspace too small
    assert lib.tmf_cam(p, p, p, p, p, w, 0, *ok) < 0
    assert lib.tmf_cam(p, p, p, p, p, w, n, 2, 16, 32, 2, 3, None) < 0                  # method
    assert lib.tmf_cam(p, p, p, p, p, w, n, 2, 16, 32, 0, 4, None) < 0                  # flags
    assert lib.tmf_cam(p, p, p, p, p, w, n, 2, 16, 32, 1, 3, None) < 0                  # weights with HiRes
    assert lib.tmf_cam(p, p, None, p, p, w, n, 2, 16, 32, 0, 3, None) < 0               # peak without cam
    assert b"tmf_cam" in lib.tmf_last_error_string()
    torch.cuda.synchronize()
    assert bool((t == 7.0).all()) and bool((ws == 7.0).all())


def test_ops_cam_and_its_routing():
    from transmf_ad_amd import ops
    case = gi.CAM_CASES[9]                                              # (3, 27, 32)
    A, G = gi.cam_inputs(case)
    a, g = A.view(3, 3, 3, 3, 32).to(DEV), G.view(3, 3, 3, 3, 32).to(DEV)
    assert ops.cam_ok(a, g) and not ops.cam_ok(a.cpu(), g.cpu()) and not ops.cam_ok(a.bfloat16(), g.bfloat16())
    assert not ops.cam_ok(a[..., :6].contiguous(), g[..., :6].contiguous())
    for method in gi.METHODS:
        for flags in gi.FLAG_SETS:
            cam, weights, peak = ops.cam(a, g, method, bool(flags & 1), bool(flags & 2))
            assert cam.shape == (3, 3, 3, 3) and peak.shape == (3,) and (weights is None) == (method == "hirescam")
            res = dict(cam=cam.cpu().view(3, 27), weights=None if weights is None else weights.cpu(), peak=peak.cpu())
            ratios = gi.cam_ratios(res, gi.cam_ref(A, G, method, flags), case, method, flags)
            assert max(ratios.values()) <= 1.0, (method, flags, ratios)
    with pytest.raises(ValueError, match="method"):
        ops.cam(a, g, "gradcam++")


# ---------------------------------------------------------------------------------------------------------------------
# the encoder tap
# ---------------------------------------------------------------------------------------------------------------------

def _calls(monkeypatch, fn):
    from transmf_ad_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    try:
        return fn(), names
    finally:
        monkeypatch.undo()


@pytest.mark.parametrize("train", (False, True), ids=("eval", "train"))
@pytest.mark.parametrize("size", (16, 32))
def test_tap_is_neutral(size, train, monkeypatch):
    """With a recording tmf_tap the encoder's output and BatchNorm buffers are the bits of the untapped encoder (which takes a
    one-call path), the tap sees the seven block outputs, and with the attribute back at None the one-call path runs again."""
    import transmf_ad_amd as T
    torch.manual_seed(11)
    base = T.sNet(32).to(DEV)
    for m in base.modules():
        if isinstance(m, torch.nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    base.train(train)
    vol = torch.rand((2, 1, size, size, size), device=DEV)
    one_call = "tmf_snet_train_fwd" if train else "tmf_snet_eval_fwd"
    plain, tapped = copy.deepcopy(base), copy.deepcopy(base)
    assert plain.tmf_tap is None
    with torch.no_grad():
        want, names = _calls(monkeypatch, lambda: plain(vol))
    assert names.count(one_call) == 1
    seen = []
    tapped.tmf_tap = lambda n, x: seen.append((n, x))
    with torch.no_grad():
        got, names = _calls(monkeypatch, lambda: tapped(vol))
    assert one_call not in names
    assert torch.equal(got, want)
    for (k, a), (_k, b) in zip(plain.state_dict().items(), tapped.state_dict().items()):
        assert torch.equal(a, b), k
    s = size
    shapes = [(2, s // 2, s // 2, s // 2, 8), (2, s // 2, s // 2, s // 2, 8), (2, s // 4, s // 4, s // 4, 16),
              (2, s // 4, s // 4, s // 4, 16), (2, s // 8, s // 8, s // 8, 32), (2, s // 8, s // 8, s // 8, 64),
              (2, s // 16, s // 16, s // 16, 32)]
    assert [n for n, _x in seen] == list(range(7)) and [tuple(x.shape) for _n, x in seen] == shapes
    assert all(x.dtype == torch.float32 and x.is_contiguous() for _n, x in seen)
    assert torch.equal(seen[6][1].permute(0, 4, 1, 2, 3), got)
    tapped.tmf_tap = None
    with torch.no_grad():
        again, names = _calls(monkeypatch, lambda: tapped(vol))
    assert names.count(one_call) == 1
    if not train:
        assert torch.equal(again, want)


# ---------------------------------------------------------------------------------------------------------------------
# grad_cam on package models
# ---------------------------------------------------------------------------------------------------------------------

def _judge(cam, weights, A, G, method, flags, tag):
    """One (encoder, layer) of a model against the fp64 formula on the same taps, by the rule of the kernel test with D measured
    here on the CPU (the fp32 torch formula on these taps against fp64) -> worst ratio."""
    B, C = A.shape[0], A.shape[-1]
    A, G = A.reshape(B, -1, C).cpu(), G.reshape(B, -1, C).cpu()
    ref, f32 = gi.cam_ref(A, G, method, flags), gi.cam_formula32(A, G, method, flags)
    worst = 0.0
    for q, got in (("cam", cam), ("weights", weights)):
        if got is None:
            continue
        rel32, dead = gi.row_errors(f32[q], ref[q])
        D = float(rel32[~dead].max()) if bool((~dead).any()) else 0.0
        rel, _d = gi.row_errors(got.cpu().reshape(B, -1), ref[q])
        exact = (got.cpu().reshape(B, -1) == 0).all(1)
        rel = torch.where(dead, torch.where(exact, torch.zeros_like(rel), torch.full_like(rel, float("inf"))), rel)
        r = float(rel.max()) / (gi.MARGIN * max(D, gi.CAM_FLOOR))
        print(f"{tag} {method} flags {flags} {q}: D {D:.2e} err / tol {r:.3f}")
        worst = max(worst, r)
    return worst


def _recording(monkeypatch, fn):
    """fn() with the two map routines wrapped -> (result, [(which routine, act, grad)] in call order = encoders x layers,
    the library entries called)."""
    from transmf_ad_amd import _lib, gradcam, ops
    seen, names = [], []
    real_cam, real_torch, real_call = ops.cam, gradcam.cam_torch, _lib.call
    monkeypatch.setattr(ops, "cam", lambda a, g, *r: (seen.append(("kernel", a, g)), real_cam(a, g, *r))[1])
    monkeypatch.setattr(gradcam, "cam_torch", lambda a, g, *r: (seen.append(("torch", a, g)), real_torch(a, g, *r))[1])
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    try:
        return fn(), seen, names
    finally:
        monkeypatch.undo()


def _model(kind):
    import transmf_ad_amd as T
    torch.manual_seed(5)
    if kind == "cnn32":
        net, size = T.model_CNN_ad(dim=32), (32, 32, 32)
    else:
        net, size = T.model_ad(dim=128, depth=1, heads=4, dim_head=32, mlp_dim=512, dropout=0.), (48, 48, 48)
    for m in net.modules():
        if isinstance(m, (torch.nn.BatchNorm3d, torch.nn.BatchNorm1d)):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    mri, pet, _y = P.make_inputs(2, size, seed=77, kind="blobs")
    return net.to(DEV).eval(), torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV), size


@pytest.mark.parametrize("kind", ("cnn32", "ad128"))
def test_grad_cam_against_grad_cam_torch(kind, monkeypatch):
    """Every layer, both methods: grad_cam (one tmf_cam per encoder and layer) and grad_cam_torch see the same tapped tensors
    bit for bit, and each is within the kernel tolerance of the fp64 formula on them."""
    import transmf_ad_amd as T
    from transmf_ad_amd.gradcam import LAYERS
    net, mri, pet, size = _model(kind)
    before = {n: p.requires_grad for n, p in net.named_parameters()}
    worst = {}
    for method in gi.METHODS:
        for flags in (0, 3):
            kw = dict(layer=LAYERS, method=method, relu=bool(flags & 1), normalize=bool(flags & 2))
            dev, taps, names = _recording(monkeypatch, lambda: T.grad_cam(net, mri, pet, **kw))
            assert names.count("tmf_cam") == 2 * len(LAYERS) == len(taps) and all(t[0] == "kernel" for t in taps)
            assert "tmf_snet_eval_fwd" not in names and "tmf_snet_train_fwd" not in names
            ref, taps_t, names = _recording(monkeypatch, lambda: T.grad_cam_torch(net, mri, pet, **kw))
            assert "tmf_cam" not in names and len(taps_t) == len(taps) and all(t[0] == "torch" for t in taps_t)
            assert dev.encoders == ref.encoders == ("mri_cnn", "pet_cnn") and torch.equal(dev.logits, ref.logits)
            assert torch.equal(dev.target, ref.target) and torch.equal(dev.target, dev.logits.argmax(1))
            keys = [(enc, layer) for enc in dev.encoders for layer in LAYERS]
            for (enc, layer), (_w, A, G), (_wt, At, Gt) in zip(keys, taps, taps_t):
                assert torch.equal(A, At) and torch.equal(G, Gt)
                assert A.shape == G.shape and dev.map(enc, layer).shape == A.shape[:-1] and float(G.abs().max()) > 0
                for who, cams in (("kernel", dev), ("torch", ref)):
                    worst[(who, method, flags, enc, layer)] = _judge(
                        cams.map(enc, layer), cams.weights(enc, layer), A, G, method, flags, f"{kind} {who} {enc}.{layer}")
            assert tuple(dev.volume("pet_cnn", "conv3").shape) == (2,) + size
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}
    # the tapped forward gave the model's own logits: the bits of its forward on volumes that want a gradient (block by block
    # with a graph, as input_gradients runs it); the no_grad forward fuses each eval block into one kernel - other roundings
    own = net(mri.clone().requires_grad_(True), pet.clone().requires_grad_(True))[0].detach()
    assert torch.equal(own, dev.logits)
    with torch.no_grad():
        assert float((net(mri, pet)[0] - dev.logits).abs().max()) <= 1e-5
    assert all(p.grad is None for p in net.parameters())
    assert {n: p.requires_grad for n, p in net.named_parameters()} == before
    assert net.mri_cnn.tmf_tap is None and net.pet_cnn.tmf_tap is None
    assert not mri.requires_grad and mri.grad is None
    with pytest.raises(ValueError):                                     # the encoder refuses two channels: everything is undone
        T.grad_cam(net, torch.cat([mri, mri], 1), pet)
    assert net.mri_cnn.tmf_tap is None and net.pet_cnn.tmf_tap is None
    assert {n: p.requires_grad for n, p in net.named_parameters()} == before


def test_bf16_storage_taps_take_the_torch_formula(monkeypatch):
    """Encoders with bf16 activation storage hand some blocks' outputs over as bf16 tensors: those maps come from the torch
    formula after an upcast (the bits of grad_cam_torch), the float32 taps still from tmf_cam."""
    import transmf_ad_amd as T
    from transmf_ad_amd.gradcam import LAYERS
    net, mri, pet, _size = _model("cnn32")
    net.mri_cnn.set_precision("bf16", "bf16")
    net.pet_cnn.set_precision("bf16", "bf16")
    seen = []
    for enc in (net.mri_cnn, net.pet_cnn):                              # which blocks hand over bf16 tensors
        enc.tmf_tap = lambda n, x: seen.append(x.dtype)
    with torch.no_grad():
        net(mri, pet)
    net.mri_cnn.tmf_tap = net.pet_cnn.tmf_tap = None
    n16 = sum(d == torch.bfloat16 for d in seen)
    assert len(seen) == 2 * len(LAYERS) and 0 < n16 < len(seen) and set(seen) == {torch.bfloat16, torch.float32}
    dev, taps, names = _recording(monkeypatch, lambda: T.grad_cam(net, mri, pet, layer=LAYERS))
    ref, taps_t, _names = _recording(monkeypatch, lambda: T.grad_cam_torch(net, mri, pet, layer=LAYERS))
    assert [t[0] for t in taps].count("torch") == n16 and names.count("tmf_cam") == len(taps) - n16
    keys = [(e, l) for e in dev.encoders for l in LAYERS]
    for (e, l), (which, A, G), (_wt, At, Gt) in zip(keys, taps, taps_t):
        m = dev.map(e, l)
        assert m.dtype == torch.float32 and bool(torch.isfinite(m).all()) and float(m.min()) >= 0 and float(m.max()) <= 1
        assert A.dtype == G.dtype == torch.float32 and torch.equal(A, At) and torch.equal(G, Gt)     # (upcast where bf16)
        if which == "torch":
            assert torch.equal(m, ref.map(e, l)) and torch.equal(dev.weights(e, l), ref.weights(e, l))
        else:
            worst = _judge(m, dev.weights(e, l), A, G, "gradcam", 3, f"bf16 storage {e}.{l}")
            assert worst <= 1.0, (e, l, worst)
    assert net.mri_cnn.tmf_tap is None and all(p.grad is None for p in net.parameters())


def test_grad_cam_in_train_mode_and_on_one_encoder():
    """The mode is the caller's: in train mode the forward moves the BatchNorm buffers exactly as the model's own forward does;
    model_single has one encoder, named by its path."""
    import transmf_ad_amd as T
    torch.manual_seed(9)
    net = T.model_single(dim=128).to(DEV).train()
    twin = copy.deepcopy(net)
    vol = torch.rand((3, 1, 32, 32, 32), device=DEV)
    cams = T.grad_cam(net, vol, layer=("conv2", "conv4"), target=1)
    with torch.no_grad():
        want = twin(vol)
    assert cams.encoders == ("cnn",) and cams.target.tolist() == [1, 1, 1] and torch.equal(cams.logits, want)
    for (k, a), (_k, b) in zip(twin.state_dict().items(), net.state_dict().items()):
        assert torch.equal(a, b), k
    assert cams.map(layer="conv2").shape == (3, 8, 8, 8) and cams.map("cnn", "conv4").shape == (3, 2, 2, 2)
    assert cams.weights(layer="conv4").shape == (3, 128) and net.training and net.cnn.tmf_tap is None
    assert bool(torch.isfinite(cams.map(layer="conv2")).all())


# ---------------------------------------------------------------------------------------------------------------------
# grad_cam against the reference's own maps
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ("cnn_tiny",))
def test_grad_cam_against_the_reference(name):
    """Raw maps (no ReLU, no normalisation: both amplify noise near zero without limit) and Grad-CAM weights at conv2, conv3,
    conv4 of every encoder, per sample within MARGIN x the reference's stored fp32 <-> fp64 distance of the tensor x the fp64
    maximum of the sample."""
    import transmf_ad_amd as T
    z = np.load(os.path.join(GOLDEN_DIR, f"gradcam_{name}.npz"))
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    vols = [torch.from_numpy(mri).to(DEV)] + ([] if g.model == "model_single" else [torch.from_numpy(pet).to(DEV)])
    target = torch.from_numpy(z["target"])
    layers = ("conv2", "conv3", "conv4")
    bad = []
    for method in gi.METHODS:
        cams = T.grad_cam(net, *vols, layer=layers, method=method, target=target, relu=False, normalize=False)
        assert ",".join(cams.encoders) == str(z["encoders"])
        assert float((cams.logits.cpu().double() - torch.from_numpy(z["logits"]).double()).abs().max()) <= 1e-3
        for enc in cams.encoders:
            for layer in layers:
                for q, got in ((method, cams.map(enc, layer)), ("weights", cams.weights(enc, layer))):
                    if got is None:
                        continue
                    key = f"{enc}.{layer}.{q}"
                    want = torch.from_numpy(z[key]).double()
                    assert got.shape == want.shape
                    err = (got.cpu().double() - want).abs().reshape(g.batch, -1).amax(1) / torch.from_numpy(z["max." + key])
                    tol = gi.MARGIN * floor_distance(float(z["dist." + key]))
                    print(f"{name} {key}: err {float(err.max()):.3e} tol {tol:.3e} err / tol {float(err.max()) / tol:.3f}")
                    if not float(err.max()) <= tol:
                        bad.append((key, f"{float(err.max()) / tol:.3g}"))
    assert not bad, bad
