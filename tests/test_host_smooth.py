"""Gaussian smoothing without a device: the numpy reference of tests/_smooth_inputs.py against scipy (once, so that every later
comparison rests on scipy's definition); the library's taps against the double formula; the stock-torch twin in float64 and
float32; the public function's conversions, folding and ValueErrors; baseline="blur" / baselines="blur" against the explicit
tensor, bit for bit; the entry's refusals (no launch is reached) and the new prototypes as the header parser read them."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _smooth_inputs as si

F32, F64 = torch.float32, torch.float64


def test_reference_is_scipys_gaussian_filter():
    ndi = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(5)
    for shape in ((1, 1, 1), (1, 5, 9), (3, 4, 70), (9, 8, 33), (2, 17, 12), (5, 1, 36)):
        x = g.standard_normal(shape) * np.exp(g.standard_normal(shape))
        for sig in si.SIGMAS + ((0.3, 0.0, 1.7),):
            for mode in si.MODES:
                want = ndi.gaussian_filter(x, sig, mode=mode, truncate=si.TRUNCATE)
                got = si.reference(x[None], sig, mode)[0]
                assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), (shape, sig, mode)
    for sigma in (0.4, 1.0, 2.265, 8.0):                   # the taps themselves: scipy's correlate1d of an impulse
        r = si.radius(sigma)
        e = np.zeros(2 * r + 1)
        e[r] = 1.0
        assert np.abs(ndi.gaussian_filter1d(e, sigma, mode="constant", truncate=si.TRUNCATE) - si.taps64(sigma)).max() <= 1e-16


def test_taps_are_the_double_formula_rounded_once():
    from transmf_ad_amd import ops
    assert ops.SMOOTH_MODES == {"reflect": 0, "constant": 1, "nearest": 2} and ops.SMOOTH_MAX_RADIUS == si.MAX_RADIUS
    for sigma in (0.0, 1e-200, 0.1, 0.4, 0.6, 1.0, 2.265, 2.5, 3.0, 4.0, 8.0, 8.124):
        want = si.taps64(sigma)
        t32, t64 = ops.gaussian_taps(sigma, si.TRUNCATE), ops.gaussian_taps(sigma, si.TRUNCATE, F64)
        assert t32.dtype == F32 and t64.dtype == F64 and t32.numel() == t64.numel() == 2 * si.radius(sigma) + 1
        assert np.abs(t64.numpy() - want).max() <= 2.0 ** -52                    # exp() of two libms
        assert bool((np.abs(t32.double().numpy() - want) <= 2.0 ** -24 * want + 2.0 ** -150).all()), sigma   # one float rounding
        assert torch.equal(t32, t64.float()) and bool((t32 > 0).all()) and torch.equal(t32, t32.flip(0))
        assert abs(float(t32.double().sum()) - 1) <= (t32.numel() + 1) * 2.0 ** -24
    # r = (int)(truncate*sigma + 0.5): just below and just above a half-integer of truncate*sigma
    for truncate, half in ((4.0, 2.5), (4.0, 9.5), (3.0, 4.5), (2.5, 31.5)):
        at = half / truncate
        lo, hi = at, at
        while truncate * lo + 0.5 >= half + 0.5:
            lo = np.nextafter(lo, 0.0)
        while truncate * hi + 0.5 < half + 0.5:
            hi = np.nextafter(hi, np.inf)
        assert ops.gaussian_taps(float(lo), truncate).numel() == 2 * int(half) + 1
        assert ops.gaussian_taps(float(hi), truncate).numel() == 2 * int(half + 1) + 1
    assert ops.gaussian_taps(8.124, 4.0).numel() == 65
    for sigma, truncate in ((8.125, 4.0), (100.0, 4.0), (1e300, 4.0), (-1.0, 4.0), (float("nan"), 4.0), (float("inf"), 4.0),
                            (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            ops.gaussian_taps(sigma, truncate)
    with pytest.raises(ValueError) as e:
        ops.gaussian_taps(8.125, 4.0)
    assert "8.125" in str(e.value) and "32" in str(e.value)                       # names the sigma and the limit


@pytest.mark.parametrize("shape", si.SHAPES + (si.LIMIT_CASE[0],), ids=lambda s: "x".join(map(str, s)))
def test_torch_twin(shape):
    """ops.gaussian_smooth_torch on the CPU: float64 within 1e-12 * peak of the reference, float32 within the derived bound;
    every mode, r >= n, n = 1, skipped axes, every map, with and without a mask."""
    from transmf_ad_amd import ops
    B, size = 1, shape[1:]                                  # the twin has no batch-dependent path: one sample of every map
    a = si.all_maps(B, size)
    sigmas = si.SIGMAS if shape != si.LIMIT_CASE[0] else (si.LIMIT_CASE[1],)
    masks = tuple(si.mask(k, size) for k in si.MASKS) if shape in si.MASKED_SHAPES else ()
    worst = 0.0
    for sig in sigmas:
        for mode in si.MODES:
            for m in (None,) + (masks if sig in si.SIGMAS[1:3] else masks[:1]):      # every mask where an axis is skipped and where r >= n
                ref = si.reference(a, sig, mode, m)
                peak = np.abs(a.double().numpy() * (1 if m is None else (m.numpy() != 0))).reshape(a.shape[0], -1).max(1).reshape(-1, 1, 1, 1)
                got64 = ops.gaussian_smooth_torch(a.double(), sig, si.TRUNCATE, mode, m)
                assert got64.dtype == F64 and bool((np.abs(got64.numpy() - ref) <= 1e-12 * peak).all()), (sig, mode)
                got32 = ops.gaussian_smooth_torch(a, sig, si.TRUNCATE, mode, m)
                err, bnd = np.abs(got32.double().numpy() - ref), si.bound(a, sig, m)
                assert got32.dtype == F32 and bool((err <= bnd).all()), (sig, mode, float((err / np.maximum(bnd, 1e-300)).max()))
                worst = max(worst, float((err / np.maximum(bnd, 1e-300)).max()))
                zero = got32[si.rows("zero", B)]
                assert not bool(zero.any())
                if m is not None:
                    assert not bool(got32[:, m == 0].any())
    print(f"{shape}: worst float32 error / bound {worst:.3f}")
    h = ops.gaussian_smooth_torch(a.bfloat16(), si.SIGMAS[0], si.TRUNCATE, "reflect")
    assert h.dtype == torch.bfloat16 and h.shape == a.shape


def test_public_function_conversions_folding_and_errors():
    from transmf_ad_amd import gaussian_smooth, gaussian_smooth_torch, ops, smooth
    assert smooth.BLUR_SIGMA == 4.0 and smooth.MODES == si.MODES
    g = torch.Generator().manual_seed(2)
    x = torch.randn((2, 3, 6, 7, 8), generator=g, dtype=F64)
    flat = x.reshape(6, 6, 7, 8)
    want = torch.from_numpy(si.reference(flat, (1.0, 1.0, 1.0), "reflect")).view(x.shape)
    for fn in (gaussian_smooth, gaussian_smooth_torch):
        got = fn(x, sigma=1.0)
        assert got.shape == x.shape and got.dtype == F64 and float((got - want).abs().max()) <= 1e-12 * float(x.abs().max())
        assert torch.equal(fn(x, sigma=(1.0, 1.0, 1.0)), got) and torch.equal(fn(x, sigma=[1, 1, 1]), got)
        assert torch.equal(fn(x[0, 0], sigma=1.0), got[0, 0])                      # (D, H, W) alone: the batch position is free
    # fwhm / spacing: sigma = fwhm / (2 sqrt(2 ln 2)) / spacing per axis
    k = 2 * math.sqrt(2 * math.log(2))
    assert torch.equal(gaussian_smooth(x, fwhm=8.0, spacing=1.5), gaussian_smooth(x, sigma=8.0 / k / 1.5))
    assert torch.equal(gaussian_smooth(x, fwhm=(6.0, 0.0, 8.0), spacing=(1.0, 2.0, 1.5)),
                       gaussian_smooth(x, sigma=(6.0 / k, 0.0, 8.0 / k / 1.5)))
    assert si.radius(8.0 / k / 1.5) == 9
    for mode in si.MODES:
        got = gaussian_smooth(x, sigma=(0.0, 2.5, 0.6), mode=mode, truncate=3.0)
        ref = si.reference(flat, (0.0, 2.5, 0.6), mode, truncate=3.0)
        assert float((got.view(flat.shape) - torch.from_numpy(ref)).abs().max()) <= 1e-12 * float(x.abs().max())
    # masks: bool, int64 labels and int32 are one mask; the result is the reference's
    lab = si.mask("bricks", (6, 7, 8))
    ref = torch.from_numpy(si.reference(flat, (1.0, 2.0, 1.0), "nearest", lab)).view(x.shape)
    for m in (lab, lab.long(), lab != 0):
        got = gaussian_smooth(x, sigma=(1.0, 2.0, 1.0), mode="nearest", mask=m)
        assert float((got - ref).abs().max()) <= 1e-12 * float(x.abs().max()) and not bool(got[..., lab == 0].any())
    # a non-contiguous float32 input takes the twin and keeps its shape
    xt = x.float().transpose(-1, -2)
    got = gaussian_smooth(xt, sigma=1.0)
    assert got.shape == xt.shape and torch.equal(got, ops.gaussian_smooth_torch(xt.reshape(6, 6, 8, 7), (1.0,) * 3).view(xt.shape))
    bad = [dict(), dict(sigma=1.0, fwhm=2.0), dict(sigma=-1.0), dict(sigma=(1.0, float("nan"), 1.0)), dict(sigma=float("inf")),
           dict(sigma=(1.0, 1.0)), dict(sigma="1"), dict(sigma=True), dict(fwhm=8.0, spacing=0.0), dict(fwhm=8.0, spacing=(1.0, -1.0, 1.0)),
           dict(sigma=8.125), dict(sigma=4.0, truncate=9.0), dict(sigma=1.0, truncate=0.0), dict(sigma=1.0, truncate=float("nan")),
           dict(sigma=1.0, mode="mirror"), dict(sigma=1.0, mode=0), dict(sigma=1.0, mask=torch.ones((6, 7, 9), dtype=torch.int32)),
           dict(sigma=1.0, mask=torch.ones((1, 6, 7, 8), dtype=torch.bool)), dict(sigma=1.0, mask=torch.ones((6, 7, 8)))]
    for kw in bad:
        for fn in (gaussian_smooth, gaussian_smooth_torch):
            with pytest.raises(ValueError):
                fn(x, **kw)
    with pytest.raises(ValueError, match=r"(?s)8\.125.*32|32.*8\.125"):                 # names the sigma and the limit
        gaussian_smooth(x, sigma=(1.0, 8.125, 1.0))
    for xx in (x.long(), x[0, 0, 0], torch.zeros((0, 4, 4, 4)), x.numpy()):
        with pytest.raises(ValueError):
            gaussian_smooth(xx, sigma=1.0)


def test_blur_baseline_of_the_faithfulness_curve_is_the_explicit_tensor():
    from test_host_faithfulness import _Sum, _sum_inputs
    from transmf_ad_amd import faithfulness_curve, faithfulness_curve_torch, gaussian_smooth_torch, smooth
    net = _Sum().eval()
    for dtype in (F64, F32):
        x, y = _sum_inputs(dtype)
        blur = gaussian_smooth_torch(x, sigma=smooth.BLUR_SIGMA)
        assert blur.shape == x.shape and not torch.equal(blur, x)
        for fn in (faithfulness_curve_torch, faithfulness_curve):                     # on the CPU both take the torch formulas
            for mode in ("deletion", "insertion"):
                kw = dict(attribution=x[:, 0], volume=0, steps=6, mode=mode, score="logit", target=0, chunk=5)
                a, b = fn(net, x, y, baseline="blur", **kw), fn(net, x, y, baseline=blur, **kw)
                assert torch.equal(a.scores, b.scores) and torch.equal(a.auc, b.auc) and torch.equal(a.removed, b.removed)
                assert not torch.equal(a.scores, fn(net, x, y, **kw).scores)
        for badv in ("gauss", "mean", 3.0):
            with pytest.raises(ValueError):
                faithfulness_curve_torch(net, x, y, attribution=x[:, 0], baseline=badv)


def test_blur_baselines_of_integrated_gradients_are_the_explicit_tensors():
    from test_host_input_grad import _Stub, _vols
    from transmf_ad_amd import gaussian_smooth_torch, integrated_gradients, smooth
    m = _Stub()
    u, v = _vols()
    base = tuple(gaussian_smooth_torch(t, sigma=smooth.BLUR_SIGMA) for t in (u, v))
    got = integrated_gradients(m, u, v, baselines="blur", steps=3, output=1)
    want = integrated_gradients(m, u, v, baselines=base, steps=3, output=1)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert not torch.equal(got[0], integrated_gradients(m, u, v, steps=3, output=1)[0])
    with pytest.raises(ValueError):
        integrated_gradients(m, u, v, baselines="zeros", output=1)


def test_entry_refuses_before_any_launch():
    """Every refusal of include/tmf_hip.h with pointers that are never dereferenced: the checks run ahead of the launches."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    A, M, O, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000
    big = 1 << 40

    def rc(a=A, mask=None, out=O, sig=(1.0, 1.0, 1.0), truncate=4.0, mode=0, ws=WS, nws=big, shape=(2, 4, 5, 6)):
        return lib.tmf_gaussian_smooth(a, mask, out, *sig, truncate, mode, ws, nws, *shape, None)

    assert rc(a=None) == rc(out=None) == rc(ws=None) == _lib.E_NULL
    for shape in ((0, 4, 5, 6), (65537, 4, 5, 6), (2, 0, 5, 6), (2, 4, 0, 6), (2, 4, 5, 0), (2, -1, 5, 6), (1, 2048, 1024, 1024),
                  (1, 1 << 16, 1 << 16, 1 << 16)):
        assert rc(shape=shape) == _lib.E_SHAPE, shape
        assert lib.tmf_smooth_workspace_bytes(*shape, 0) == 0 and lib.tmf_smooth_workspace_bytes(*shape, 1) == 0
    for mode in (-1, 3):
        assert rc(mode=mode) == _lib.E_ARG
    for sig in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (8.125, 1.0, 1.0), (1.0, 1.0, 1e300)):
        assert rc(sig=sig) == _lib.E_ARG, sig
    for truncate in (0.0, -1.0, float("nan"), float("inf"), 33.0):
        assert rc(truncate=truncate) == _lib.E_ARG, truncate
    assert rc(a=A + 2) == rc(out=O + 2) == rc(mask=M + 1) == rc(ws=WS + 8) == _lib.E_ALIGN
    n = 2 * 4 * 5 * 6 * 4
    for out in (A, A + 4, A + n - 4, A - n + 4):
        assert rc(out=out) == _lib.E_ARG, hex(out)
    need0, need1 = lib.tmf_smooth_workspace_bytes(2, 4, 5, 6, 0), lib.tmf_smooth_workspace_bytes(2, 4, 5, 6, 1)
    assert need0 == n and need1 == n + 4 * 5 * 6 * 4 and need0 % 16 == 0 and need1 % 16 == 0
    assert lib.tmf_smooth_workspace_bytes(1, 3, 3, 3, 0) == 112 and lib.tmf_smooth_workspace_bytes(1, 3, 3, 3, 1) == 224   # 27 -> 28 floats
    assert rc(nws=need0 - 1) == _lib.E_WORKSPACE and rc(mask=M, nws=need1 - 1) == _lib.E_WORKSPACE
    assert b"workspace" in lib.tmf_last_error_string()
    buf = (ctypes.c_float * 65)()
    assert lib.tmf_gaussian_taps(1.0, 4.0, None, 65) == _lib.E_NULL and lib.tmf_gaussian_taps(1.0, 4.0, ctypes.addressof(buf), 8) == _lib.E_ARG
    assert lib.tmf_gaussian_taps(1.0, 4.0, ctypes.addressof(buf), 9) == 4 and buf[9] == 0.0 and buf[4] == max(buf)


def test_prototypes_as_the_header_parser_read_them():
    from transmf_ad_amd import _lib
    from transmf_ad_amd.build import SOURCES
    C = ctypes
    P = _lib.PROTOTYPES
    assert P["tmf_gaussian_taps"] == (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_int])
    assert P["tmf_gaussian_taps_f64"] == (C.c_int, [C.c_double, C.c_double, C.c_void_p, C.c_int])
    assert P["tmf_smooth_workspace_bytes"] == (C.c_size_t, [C.c_int] * 5)
    assert P["tmf_gaussian_smooth"] == (C.c_int, [C.c_void_p] * 3 + [C.c_double] * 4 + [C.c_int, C.c_void_p, C.c_size_t] + [C.c_int] * 4
                                        + [C.c_void_p])
    assert (_lib.SMOOTH_REFLECT, _lib.SMOOTH_CONSTANT, _lib.SMOOTH_NEAREST, _lib.SMOOTH_MAX_RADIUS) == (0, 1, 2, 32)
    assert "smooth.hip" in SOURCES
    import transmf_ad_amd
    for name in ("gaussian_smooth", "gaussian_smooth_torch"):
        assert name in transmf_ad_amd.__all__ and callable(getattr(transmf_ad_amd, name))
