"""FALoss / SupConLoss without a GPU: the package's torch-op formulas against the reference's fp64 results recorded in
tests/golden/loss_*.npz (tests/golden/make_golden_losses.py), the drop-in surface (constructors, attributes, ValueErrors, the
NaN case), the *_kernel_ok answers, the C-ABI bindings and the register / scratch budget of csrc/losses.hip."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import _loss_inputs as LI                      # noqa: E402
from oracle import params as P                 # noqa: E402
from transmf_ad_amd import losses as L         # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(bytes(z["meta"]).decode())


def gprobe(g):
    g = g.detach().double().reshape(-1)
    idx = torch.from_numpy(P.probe_indices(g.numel()))
    return np.concatenate([[g.sum().item(), g.abs().sum().item(), g.abs().max().item()], g[idx].numpy()])


def assert_probe(got, want, rel=1e-12):
    """[sum, sum |.|, max |.|, probes ...]: the sum to `rel` of the sum of magnitudes, everything else to `rel` of itself
    or of the largest entry."""
    assert abs(got[0] - want[0]) <= rel * want[1], (got[0], want[0])
    assert np.all(np.abs(got[1:] - want[1:]) <= rel * np.maximum(np.abs(want[1:]), want[2])), np.abs(got[1:] - want[1:]).max()


@pytest.mark.parametrize("name", list(LI.FA_CASES))
def test_fa_formula_reproduces_reference_fp64(name):
    z, meta = load(name)
    assert (meta["B"], meta["C"], tuple(meta["spatial"])) == LI.FA_CASES[name] and meta["seed"] == LI.FA_SEED
    a, b = LI.fa_inputs(meta["B"], meta["C"], meta["spatial"], meta["seed"])
    x = torch.from_numpy(a).double().requires_grad_(True)
    y = torch.from_numpy(b).double().requires_grad_(True)
    loss = L.FALoss()(x, y)
    loss.backward()
    want = float(z["loss64"])
    assert abs(loss.item() - want) <= 1e-12 * abs(want), (loss.item(), want)
    assert_probe(gprobe(x.grad), z["g1_64"])
    assert_probe(gprobe(y.grad), z["g2_64"])


def _sc_call(name, dtype=torch.float64):
    z, meta = load(name)
    bs, views, d, positives, mode, shape = LI.SC_CASES[name]
    assert (meta["bs"], meta["views"], meta["d"], meta["positives"], meta["contrast_mode"]) == (bs, views, d, positives, mode)
    f, labels, mask = LI.sc_inputs(bs, views, d, positives, shape, meta["seed"])
    x = torch.from_numpy(f).to(dtype).requires_grad_(True)
    loss = L.SupConLoss(contrast_mode=mode)(x, labels=None if labels is None else torch.from_numpy(labels),
                                            mask=None if mask is None else torch.from_numpy(mask))
    loss.backward()
    return z, loss, x


@pytest.mark.parametrize("name", list(LI.SC_CASES))
def test_supcon_formula_reproduces_reference_fp64(name):
    z, loss, x = _sc_call(name)
    want = float(z["loss64"])
    assert abs(loss.item() - want) <= 1e-12 * abs(want), (loss.item(), want)
    assert_probe(gprobe(x.grad), z["g_64"])
    g64 = z["grad64"]
    assert x.grad.shape == g64.shape
    assert np.abs(x.grad.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()


def test_constructors_and_attributes_match_the_reference():
    fa = L.FALoss()
    assert (fa.subsample_factor, fa.reduction) == (8, "mean")
    assert isinstance(fa, torch.nn.modules.loss._Loss)
    fa = L.FALoss(4, None, None, "sum")
    assert (fa.subsample_factor, fa.reduction) == (4, "sum")
    assert L.FALoss(subsample_factor=2, size_average=False, reduce=False, reduction="none").reduction == "none"
    sc = L.SupConLoss()
    assert (sc.temperature, sc.contrast_mode, sc.base_temperature) == (0.07, "all", 0.07)
    sc = L.SupConLoss(0.5, "one", 0.1)
    assert (sc.temperature, sc.contrast_mode, sc.base_temperature) == (0.5, "one", 0.1)
    import transmf_ad_amd
    assert transmf_ad_amd.FALoss is L.FALoss and transmf_ad_amd.SupConLoss is L.SupConLoss


def test_fa_reductions_on_the_torch_path():
    a, b = LI.fa_inputs(2, 32, (2, 3, 2))
    x, y = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    none = L.FALoss(reduction="none")(x, y)
    assert none.shape == (2, 12 * 12)
    d = torch.einsum("bci,bcj->bij", x.flatten(2), x.flatten(2)) - torch.einsum("bci,bcj->bij", y.flatten(2), y.flatten(2))
    assert torch.allclose(none, d.abs().flatten(1), rtol=1e-13, atol=1e-13)
    assert torch.allclose(L.FALoss(reduction="sum")(x, y), d.abs().sum(), rtol=1e-13)
    assert torch.allclose(L.FALoss()(x, y), d.abs().sum() / (2 * 144), rtol=1e-13)


def test_fa_identical_inputs_give_zero_loss_and_zero_gradients():
    a, _ = LI.fa_inputs(2, 64, (5, 6, 5))
    x = torch.from_numpy(a).requires_grad_(True)
    y = torch.from_numpy(a.copy()).requires_grad_(True)
    loss = L.FALoss()(x, y)
    loss.backward()
    assert loss.item() == 0.0
    assert not x.grad.any() and not y.grad.any()


def test_supcon_value_errors():
    sc = L.SupConLoss()
    f = torch.randn(4, 2, 8)
    with pytest.raises(ValueError, match="at least 3 dimensions"):
        sc(torch.randn(4, 8))
    with pytest.raises(ValueError, match="Cannot define both"):
        sc(f, labels=torch.zeros(4), mask=torch.eye(4))
    with pytest.raises(ValueError, match="Num of labels"):
        sc(f, labels=torch.zeros(5))
    with pytest.raises(ValueError, match="Unknown mode"):
        L.SupConLoss(contrast_mode="some")(f)


def test_supcon_anchor_without_positive_is_nan():
    f, _, _ = LI.sc_inputs(4, 1, 8, "labels")          # one view and distinct labels: no anchor has a positive
    loss = L.SupConLoss()(torch.from_numpy(f), labels=torch.arange(4))
    assert torch.isnan(loss)
    f, _, _ = LI.sc_inputs(4, 2, 8, "labels")
    mask = torch.ones(4, 4)
    mask[2] = 0                                          # sample 2 has no positive at all, not even its other view
    assert torch.isnan(L.SupConLoss()(torch.from_numpy(f), mask=mask))


def test_supcon_flattens_more_than_three_dimensions():
    f, labels, _ = LI.sc_inputs(8, 2, 32, "labels")
    lab = torch.from_numpy(labels)
    a = L.SupConLoss()(torch.from_numpy(f), labels=lab)
    b = L.SupConLoss()(torch.from_numpy(f.reshape(8, 2, 4, 8)), labels=lab)
    assert a.item() == b.item()


def test_kernel_ok_answers():
    for B, C, spatial in LI.FA_CASES.values():
        N = int(np.prod(spatial))
        assert L.fa_shape_ok(C, N, "mean") and L.fa_shape_ok(C, N, "sum")
        assert not L.fa_shape_ok(C, N, "none")
    for C in (32, 64, 96, 128, 160, 192, 224, 256):
        assert L.fa_shape_ok(C, 1) and L.fa_shape_ok(C, 150)
    for C in (1, 16, 48, 100, 288, 512):
        assert not L.fa_shape_ok(C, 216)
    assert not L.fa_shape_ok(64, 0)
    for bs, views, d, _p, _m, _s in LI.SC_CASES.values():
        assert L.supcon_shape_ok(bs, views, d)
    assert not L.supcon_shape_ok(65, 2, 128)             # 130 rows
    assert not L.supcon_shape_ok(8, 2, 130) and not L.supcon_shape_ok(8, 2, 2)
    # CPU tensors and other dtypes never take the kernels
    x = torch.zeros(2, 64, 3, 3, 3)
    assert not L.fa_kernel_ok(x, x) and not L.fa_kernel_ok(x.double(), x.double())
    assert not L.supcon_kernel_ok(torch.zeros(8, 2, 128))


def test_new_symbols_are_bound_and_validate_arguments():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    for n in ("tmf_faloss_ok", "tmf_faloss_partial_rows", "tmf_faloss_workspace_bytes", "tmf_faloss_fwd", "tmf_faloss_bwd",
              "tmf_supcon_ok", "tmf_supcon_fwd", "tmf_supcon_bwd"):
        assert n in _lib.PROTOTYPES and hasattr(lib, n)
    assert _lib.query("tmf_faloss_partial_rows", 2, 150) == 2 * 5
    assert _lib.query("tmf_faloss_workspace_bytes", 2, 150) == 2 * 5 * 8
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_faloss_fwd", None, None, None, None, None, None, 0, 1, 64, 8, 0, 0, None)
    with pytest.raises(_lib.TmfError, match="multiple of 32"):
        _lib.call("tmf_faloss_fwd", 16, 16, 16, None, None, 16, 1 << 20, 1, 48, 8, 0, 0, None)
    with pytest.raises(_lib.TmfError, match="workspace"):
        _lib.call("tmf_faloss_fwd", 16, 16, 16, None, None, 16, 8, 2, 64, 150, 0, 0, None)
    with pytest.raises(_lib.TmfError, match="bs\\*views <= 128"):
        _lib.call("tmf_supcon_fwd", 16, None, None, 16, None, 65, 2, 128, 1, 0.07, 0.07, None)
    with pytest.raises(_lib.TmfError, match="exclusive"):
        _lib.call("tmf_supcon_fwd", 16, 16, 16, 16, None, 8, 2, 128, 1, 0.07, 0.07, None)


@pytest.fixture(scope="module")
def loss_kernels():
    from tools import resources as R
    obj = os.path.join(R.CSRC, "losses.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built (python -m transmf_ad_amd.build)")
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    return R.kernels_of(obj)


def test_loss_kernels_have_no_scratch_and_fit_256_registers(loss_kernels):
    fa = [k for k in loss_kernels if "faloss_kernel" in k["name"]]
    assert len(fa) == 16                                 # 8 channel counts x (with | without the gradient)
    sc = [k for k in loss_kernels if "supcon_kernel" in k["name"]]
    assert len(sc) == 2
    for k in loss_kernels:
        assert k.get("scratch", 0) == 0, k
    for k in fa + sc:
        assert k["vgpr"] <= 256, k
