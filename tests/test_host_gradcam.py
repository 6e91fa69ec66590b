"""Class activation maps without a GPU: the fp64 formulas and the tolerance table of tests/_gradcam_inputs.py, grad_cam_torch on
a plain torch module with conv1 ... conv4 Sequentials against autograd written out by hand, layer names and error types, the
committed fixtures' keep rule, and the new names in the header, the ctypes prototypes, INTEGRATION.md and the package."""
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import _gradcam_inputs as gi
from _golden import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the formulas
# ---------------------------------------------------------------------------------------------------------------------

A_HAND = torch.tensor([[[1., 2, 3, 4], [0, -1, 2, 1], [2, 0, -2, 1]],
                       [[1, 1, 1, 1], [2, 0, 0, 2], [0, 3, 0, 0]]])
G_HAND = torch.tensor([[[1., 0, -1, 2], [3, 0, 1, -2], [-1, 3, 0, 0]],
                       [[-3, 0, 3, 0], [0, -6, 0, 0], [-3, 0, 0, -3]]])
# column means of G: sample 0 (1, 1, 0, 0), sample 1 (-2, -2, 1, -1)
HAND = {
    ("gradcam", 0): ([[3, -1, 2], [-4, -6, -6]], [3, -4]),
    ("gradcam", gi.RELU): ([[3, 0, 2], [0, 0, 0]], [3, 0]),
    ("gradcam", gi.RELU | gi.NORMALIZE): ([[1, 0, 2 / 3], [0, 0, 0]], [3, 0]),
    ("gradcam", gi.NORMALIZE): ([[1, -1 / 3, 2 / 3], [0, 0, 0]], [3, -4]),           # a maximum of -4: zeros, not a division
    ("hirescam", 0): ([[6, 0, -2], [0, 0, 0]], [6, 0]),
    ("hirescam", gi.RELU | gi.NORMALIZE): ([[1, 0, 0], [0, 0, 0]], [6, 0]),
}


@pytest.mark.parametrize("method,flags", sorted(HAND))
def test_formulas_on_a_hand_computed_example(method, flags):
    cam, peak = HAND[(method, flags)]
    for fn in (gi.cam_ref, gi.cam_formula32):
        got = fn(A_HAND, G_HAND, method, flags)
        assert torch.allclose(got["cam"].double(), torch.tensor(cam, dtype=torch.float64), rtol=0, atol=1e-6), fn.__name__
        assert torch.allclose(got["peak"].double(), torch.tensor(peak, dtype=torch.float64), rtol=0, atol=1e-6)
        assert torch.isfinite(got["cam"]).all()
        if method == "gradcam":
            want = torch.tensor([[1., 1, 0, 0], [-2, -2, 1, -1]], dtype=torch.float64)
            assert torch.allclose(got["weights"].double(), want, rtol=0, atol=1e-6)
        else:
            assert got["weights"] is None


def test_package_formula_is_the_same_formula():
    from transmf_ad_amd.gradcam import cam_torch
    for method in gi.METHODS:
        for flags in (0, gi.RELU, gi.NORMALIZE, gi.RELU | gi.NORMALIZE):
            want = gi.cam_ref(A_HAND, G_HAND, method, flags)
            cam, weights, peak = cam_torch(A_HAND.double().view(2, 3, 1, 1, 4), G_HAND.double().view(2, 3, 1, 1, 4), method,
                                           bool(flags & gi.RELU), bool(flags & gi.NORMALIZE))
            assert cam.shape == (2, 3, 1, 1) and torch.allclose(cam.view(2, 3), want["cam"], rtol=0, atol=1e-12)
            assert torch.allclose(peak, want["peak"], rtol=0, atol=1e-12)
            assert (weights is None) == (method == "hirescam")


def test_cases_cover_what_the_kernel_can_get_wrong():
    cs = {c[2] for c in gi.CAM_CASES}
    vs = {c[1] for c in gi.CAM_CASES}
    assert {8, 12, 16, 32, 64, 128, 256, 512} <= cs and {1, 7, 27, 216, 1000, 1573} <= vs
    assert {1, 3} <= {c[0] for c in gi.CAM_CASES}
    assert len({c[:3] for c in gi.CAM_CASES}) == len(gi.CAM_CASES) == len(gi.CAM_DISTANCE)
    roles = [r for c in gi.CAM_CASES for r in c[3]]
    assert all(len(c[3]) == c[0] for c in gi.CAM_CASES) and {"mixed", "nonpos", "zerograd"} == set(roles)
    for c in gi.CAM_CASES:
        if c[0] >= 3:
            assert {"mixed", "nonpos", "zerograd"} <= set(c[3])
    A, G = gi.cam_inputs(gi.CAM_CASES[3])
    mixed = gi.CAM_CASES[3][3].index("mixed")
    means = G[mixed].mean(0)
    assert bool((A[mixed] > 0).any() and (A[mixed] < 0).any() and (means > 0).any() and (means < 0).any())


@pytest.mark.parametrize("case", gi.CAM_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_recorded_distances_and_zero_rows(case):
    """The table is what this machine measures (within 2x), no recorded distance comes from a row whose fp64 maximum is 0, and
    those rows are exact zeros in the fp32 formula too - which is why the kernel is held to exact zeros there."""
    now = gi.cam_distances(case)
    rec = gi.CAM_DISTANCE[case[:3]]
    assert set(now) == set(rec)
    for key, d in now.items():
        assert d <= 2 * max(rec[key], gi.CAM_FLOOR) and rec[key] <= 2 * max(d, gi.CAM_FLOOR), (key, d, rec[key])
    A, G = gi.cam_inputs(case)
    for method in gi.METHODS:
        for flags in gi.FLAG_SETS:
            r64, r32 = gi.cam_ref(A, G, method, flags), gi.cam_formula32(A, G, method, flags)
            dead = r64["cam"].abs().max(1).values == 0
            want_dead = torch.tensor([r == "zerograd" or (r == "nonpos" and bool(flags & gi.RELU)) for r in case[3]])
            assert bool(dead[want_dead].all()), (method, flags)      # (and a mixed sample of a few voxels that ReLU clamps whole)
            assert case[1] < 27 or torch.equal(dead, want_dead), (method, flags)
            assert bool((r32["cam"][dead] == 0).all())
            rel, dead2 = gi.row_errors(r32["cam"], r64["cam"])
            assert torch.equal(dead, dead2)
            live = float(rel[~dead].max()) if bool((~dead).any()) else 0.0
            assert live == now[(method, flags, "cam")]                      # the recorded number is the live rows' alone
            ratios = gi.cam_ratios(r32, r64, case, method, flags)
            assert max(ratios.values()) <= 1.0 / gi.MARGIN * 2 + 1e-9, ratios      # the formula itself sits at <= 2 / MARGIN
    bad = gi.cam_ref(A, G, "gradcam", gi.RELU)
    if bool((bad["cam"].abs().max(1).values == 0).any()):                        # a non-zero in a zero row is an error
        b = int((bad["cam"].abs().max(1).values == 0).nonzero()[0])
        wrong = dict(cam=bad["cam"].clone(), weights=None, peak=None)
        wrong["cam"][b, 0] = 1e-30
        assert gi.cam_ratios(wrong, bad, case, "gradcam", gi.RELU)["cam"] == float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# grad_cam_torch on a plain torch module, against autograd by hand
# ---------------------------------------------------------------------------------------------------------------------

def _block(cin, cout, k):
    return [nn.Conv3d(cin, cout, k, padding=k // 2), nn.BatchNorm3d(cout), nn.LeakyReLU()]


class _Enc(nn.Module):
    def __init__(self, dim=8):
        super().__init__()
        q, h = dim // 4, dim // 2
        self.conv1 = nn.Sequential(*_block(1, q, 3), nn.MaxPool3d(2, 2))
        self.conv2 = nn.Sequential(*_block(q, q, 3), *_block(q, h, 3), nn.MaxPool3d(2, 2))
        self.conv3 = nn.Sequential(*_block(h, h, 3), *_block(h, dim, 3), nn.MaxPool3d(2, 2))
        self.conv4 = nn.Sequential(*_block(dim, 2 * dim, 3), *_block(2 * dim, dim, 1), nn.AvgPool3d(2, 2))

    def forward(self, x):
        return self.conv4(self.conv3(self.conv2(self.conv1(x))))


class _Two(nn.Module):
    def __init__(self):
        super().__init__()
        self.mri_cnn, self.pet_cnn = _Enc(), _Enc()
        self.fc = nn.Linear(16, 3)

    def forward(self, mri, pet):
        f = torch.cat([self.mri_cnn(mri).mean((2, 3, 4)), self.pet_cnn(pet).mean((2, 3, 4))], 1)
        return self.fc(f), f                                        # a tuple: output 0 holds the logits


def _plain_model():
    torch.manual_seed(3)
    net = _Two().double().eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm3d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net


def _by_hand(net, mri, pet, target):
    """{(encoder, layer): (A, G)} as (B, C, d, h, w) from a forward written out block by block and one autograd.grad."""
    taps = {}
    feats = []
    for name, enc, vol in (("mri_cnn", net.mri_cnn, mri), ("pet_cnn", net.pet_cnn, pet)):
        x = taps[(name, "conv1")] = enc.conv1(vol)
        x = taps[(name, "conv2.2")] = enc.conv2[:3](x)
        x = taps[(name, "conv2")] = enc.conv2[3:](x)
        x = taps[(name, "conv3.2")] = enc.conv3[:3](x)
        x = taps[(name, "conv3")] = enc.conv3[3:](x)
        x = taps[(name, "conv4.2")] = enc.conv4[:3](x)
        x = taps[(name, "conv4")] = enc.conv4[3:](x)
        feats.append(x.mean((2, 3, 4)))
    logits = net.fc(torch.cat(feats, 1))
    score = sum(logits[b, t] for b, t in enumerate(target))
    keys = list(taps)
    grads = torch.autograd.grad(score, [taps[k] for k in keys])
    return {k: (taps[k].detach(), g) for k, g in zip(keys, grads)}, logits.detach()


def test_grad_cam_torch_on_a_plain_module_against_autograd_by_hand():
    import transmf_ad_amd as T
    from transmf_ad_amd.gradcam import LAYERS
    net = _plain_model()
    g = torch.Generator().manual_seed(5)
    mri, pet = torch.rand((2, 1, 16, 16, 16), generator=g).double(), torch.rand((2, 1, 16, 16, 16), generator=g).double()
    target = [2, 0]
    hand, logits = _by_hand(net, mri, pet, target)
    before = {n: p.requires_grad for n, p in net.named_parameters()}
    for method in ("gradcam", "hirescam"):
        cams = T.grad_cam_torch(net, mri, pet, layer=LAYERS, method=method, target=target, relu=False, normalize=False)
        assert cams.encoders == ("mri_cnn", "pet_cnn") and cams.layers == LAYERS and cams.method == method
        assert torch.equal(cams.logits, logits) and cams.target.tolist() == target
        for (enc, layer), (A, G) in hand.items():
            if method == "gradcam":
                w = G.mean((2, 3, 4))
                want = (w[:, :, None, None, None] * A).sum(1)
                assert torch.allclose(cams.weights(enc, layer), w, rtol=0, atol=1e-15)
            else:
                want = (G * A).sum(1)
                assert cams.weights(enc, layer) is None
            got = cams.map(enc, layer)
            assert got.shape == want.shape and float(want.abs().max()) > 0
            assert torch.allclose(got, want, rtol=0, atol=1e-12 * float(want.abs().max())), (enc, layer)
            assert torch.allclose(cams.peak(enc, layer), want.reshape(2, -1).amax(1), rtol=0, atol=1e-15)
        assert cams.volume("pet_cnn", "conv3").shape == (2, 16, 16, 16)
        assert cams.volume("pet_cnn", "conv3", size=(8, 9, 10)).shape == (2, 8, 9, 10)
    # defaults: ReLU and normalisation, the argmax class, one layer - and nothing left behind
    cams = T.grad_cam_torch(net, mri, pet)
    assert cams.layers == ("conv3",) and torch.equal(cams.target, logits.argmax(1))
    m = cams.map("mri_cnn")
    assert float(m.min()) >= 0 and all(float(x) in (0.0, 1.0) for x in m.reshape(2, -1).amax(1))
    assert all(not mod._forward_hooks for mod in net.modules())
    assert {n: p.requires_grad for n, p in net.named_parameters()} == before
    assert all(p.grad is None for p in net.parameters())
    assert not mri.requires_grad and mri.grad is None


def test_taps_and_freeze_are_undone_when_the_model_raises():
    import transmf_ad_amd as T
    net = _plain_model()
    net.fc = nn.Linear(5, 3).double()                                 # the head no longer fits: the forward raises
    vol = torch.rand(1, 1, 16, 16, 16).double()
    with pytest.raises(RuntimeError):
        T.grad_cam_torch(net, vol, vol)
    assert all(not mod._forward_hooks for mod in net.modules())
    assert all(p.requires_grad for p in net.parameters())
    own = T.model_CNN_ad(dim=32)                                       # a package model on the CPU: its kernels refuse, the taps go
    with pytest.raises(Exception):
        T.grad_cam(own, vol.float(), vol.float())
    assert own.mri_cnn.tmf_tap is None and own.pet_cnn.tmf_tap is None
    assert all(p.requires_grad for p in own.parameters())


def test_layer_names_and_error_types():
    import transmf_ad_amd as T
    from transmf_ad_amd import gradcam
    assert gradcam.LAYERS == ("conv1", "conv2.2", "conv2", "conv3.2", "conv3", "conv4.2", "conv4")
    assert T.sNet.TAP_LAYERS == {"conv1": 0, "conv2.2": 1, "conv2": 2, "conv3.2": 3, "conv3": 4, "conv4.2": 5, "conv4": 6}
    # the table against the plan of the blocks: the Sequential and, for an inner block, the index of its LeakyReLU
    for name, n in T.sNet.TAP_LAYERS.items():
        seq, conv_at, pool = T.sNet._PLAN[n]
        assert name == (seq if pool else f"{seq}.{conv_at + 2}")
    assert gradcam.resolve_layers("conv3") == ("conv3",)
    assert gradcam.resolve_layers(["conv2", "conv3", "conv2"]) == ("conv2", "conv3")
    vol = torch.rand(1, 1, 16, 16, 16)
    own, plain = T.model_CNN_ad(dim=32), _plain_model()
    for fn, net in ((T.grad_cam, own), (T.grad_cam_torch, own), (T.grad_cam_torch, plain)):
        for bad in ("conv5", "conv1.2", "conv2.5", "", (), ("conv3", 4), None, 3):
            with pytest.raises(ValueError, match="layer"):
                fn(net, vol, vol, layer=bad)
        with pytest.raises(ValueError, match="method"):
            fn(net, vol, vol, method="gradcam++")
    for fn in (T.grad_cam, T.grad_cam_torch):
        with pytest.raises(TypeError, match="sNet"):
            fn(nn.Linear(2, 2), vol)
    with pytest.raises(TypeError, match="sNet"):
        T.grad_cam(plain, vol, vol)                                   # forward hooks are grad_cam_torch's
    enc = T.sNet(32)
    assert enc.tmf_tap is None
    assert [n for n, _m, own_ in gradcam.find_encoders(T.model_single(dim=32))] == ["cnn"]
    assert [n for n, _m, own_ in gradcam.find_encoders(T.model_ad(32, 1, 2, 8, 64, 0.))] == ["mri_cnn", "pet_cnn"]


# ---------------------------------------------------------------------------------------------------------------------
# fixtures, header, prototypes, documents
# ---------------------------------------------------------------------------------------------------------------------

def test_committed_fixtures_keep_rule():
    """Every committed gradcam fixture: raw maps of both methods and the weights at conv2, conv3, conv4 of every encoder, the
    reference's fp32 run within 1e-3 of its fp64 run at each of them, small enough to be committed."""
    paths = sorted(p for p in os.listdir(GOLDEN_DIR) if re.fullmatch(r"gradcam_\w+\.npz", p))
    assert "gradcam_cnn_tiny.npz" in paths
    for p in paths:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, p)) < 1 << 20
        z = np.load(os.path.join(GOLDEN_DIR, p))
        encoders = str(z["encoders"]).split(",")
        B = z["logits"].shape[0]
        assert z["target"].shape == (B,) and np.array_equal(z["target"], z["logits"].argmax(1))
        for enc in encoders:
            for layer in ("conv2", "conv3", "conv4"):
                for q in ("gradcam", "hirescam", "weights"):
                    key = f"{enc}.{layer}.{q}"
                    t64, t32 = z[key].astype(np.float64), z[key + ".f32"].astype(np.float64)
                    assert t64.shape == t32.shape and t64.shape[0] == B and np.isfinite(t64).all()
                    peak = np.abs(t64).reshape(B, -1).max(1)
                    assert (peak > 0).all() and np.allclose(peak, z["max." + key], rtol=1e-6)
                    dist = (np.abs(t32 - t64).reshape(B, -1).max(1) / z["max." + key]).max()
                    assert dist <= 1e-3 and float(z["dist." + key]) <= 1e-3, (p, key, dist)
                    assert abs(dist - float(z["dist." + key])) <= 2.0 ** -22          # (t64 is stored rounded to fp32)


def test_new_names_in_header_prototypes_and_documents():
    from transmf_ad_amd import _lib, ops
    import transmf_ad_amd as T
    with open(os.path.join(ROOT, "include", "tmf_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        row = [l for l in f if l.startswith("| **`tmf_cam`**")]
    assert len(row) == 1
    stated = {name: int(n) for name, n in re.findall(r"`(tmf_cam\w*)`[^|`]*?\((\d+) arguments?\)", row[0])}
    assert stated == {"tmf_cam": 13, "tmf_cam_workspace_bytes": 4, "tmf_cam_ok": 1}
    for name, nargs in stated.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert (_lib.CAM_GRAD, _lib.CAM_HIRES, _lib.CAM_RELU, _lib.CAM_NORMALIZE) == (0, 1, gi.RELU, gi.NORMALIZE)
    assert callable(ops.cam) and set(ops.CAM_METHODS) == set(gi.METHODS)
    assert "grad_cam" in T.__all__ and "grad_cam_torch" in T.__all__
    assert callable(T.grad_cam) and callable(T.grad_cam_torch)
    from transmf_ad_amd import build
    assert "cam.hip" in build.SOURCES
