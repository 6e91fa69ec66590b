"""Gaussian smoothing on the device: the kernels of csrc/smooth.hip on their own (through _lib.call with raw pointers) against the
numpy fp64 reference of tests/_smooth_inputs.py within the bound include/tmf_hip.h derives - every shape at which a mechanism
can go wrong, four sigma sets, three border modes, every map, five masks; exact zeros, no negative output from a map without
negative values, zeros outside the mask; equal bits between calls, batches and access paths; every refusal; then
gaussian_smooth against gaussian_smooth_torch and the two places that take a blurred baseline on the tiny 32^3 model.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs, the
mask and the bands around the workspace included) must be unchanged, every output element written."""
import numpy as np
import pytest
import torch

import _smooth_inputs as si
from _golden import Golden
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _query, _st
from test_gpu_model import DEV, build

pytestmark = pytest.mark.gpu
F32, I32 = torch.float32, torch.int32
MODE = {"reflect": 0, "constant": 1, "nearest": 2}


def _smooth(ar, a, out, sig, mode, B, size, nws, mask=None, a_off=0, out_off=0, mask_off=0):
    _call("tmf_gaussian_smooth", ar.ptr(a) + a_off, None if mask is None else ar.ptr(mask) + mask_off, ar.ptr(out) + out_off,
          *sig, si.TRUNCATE, MODE[mode], ar.ptr("ws"), nws, B, *size, _st())


def _check(got, a, sig, mode, B, mask=None, what=""):
    """The bound against the fp64 reference, per element and sample -> the worst error / bound; exact zeros for the zero map,
    no negative output from the maps without negative values, the constant within the bound of the constant, zeros outside."""
    ref, bnd = si.reference(a, sig, mode, mask), si.bound(a, sig, mask)
    err = np.abs(got.double().numpy() - ref)
    ratio = float((err / np.maximum(bnd, 1e-300)).max()) if bnd.max() > 0 else float(err.max() > 0)
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert bool((err <= bnd).all()), (what, ratio)
    assert not bool(got[si.rows("zero", B)].any()), (what, "zero map")
    for k in ("abs_normal", "abs_heavy"):
        assert float(got[si.rows(k, B)].min()) >= 0.0, (what, k)
    if mode != "constant" and mask is None:
        assert bool(((got[si.rows("constant", B)].double() - 3.7).abs().numpy() <= bnd[si.rows("constant", B)]).all()), (what, "constant")
    if mask is not None:
        assert not bool(got[:, mask == 0].any()), (what, "outside the mask")
    return ratio


@pytest.mark.parametrize("case", si.CASES, ids=si.case_id)
def test_smooth_kernel(case):
    """Every map (stacked along the batch) of one shape, sigma set and mode, twice into separate outputs through ONE
    workspace: the bound, the exact properties, and equal bits of the second call."""
    shape, sig, mode = case
    B, size = shape[0], shape[1:]
    a = si.all_maps(B, size)
    n = a.shape[0]
    nws = _query("tmf_smooth_workspace_bytes", n, *size, 0)
    assert nws >= a.numel() * 4 and nws % 16 == 0
    ar = Arena({"a": a}, {"ws": ((nws,), torch.uint8), "out": (tuple(a.shape), F32), "out#2": (tuple(a.shape), F32)}, tail=4096)
    _smooth(ar, "a", "out", sig, mode, n, size, nws)
    _smooth(ar, "a", "out#2", sig, mode, n, size, nws)
    got = ar.fetch(workspace=("ws",))
    _check(got["out"], a, sig, mode, B, what=si.case_id(case))
    assert torch.equal(got["out"].view(I32), got["out#2"].view(I32)), "the second call"


@pytest.mark.parametrize("case", si.MASKED_CASES, ids=si.case_id)
def test_smooth_kernel_masked(case):
    """The same with every mask: G(a*m) / G(m) inside within (2E + 2) * 2^-24 * max|a*m|, exactly 0 outside; the mask and the
    maps unchanged; a second call gives equal bits."""
    shape, sig, mode = case
    B, size = shape[0], shape[1:]
    a = si.all_maps(B, size)
    n = a.shape[0]
    nws = _query("tmf_smooth_workspace_bytes", n, *size, 1)
    V = size[0] * size[1] * size[2]
    assert nws >= (a.numel() + V) * 4 and nws % 16 == 0
    masks = {k: si.mask(k, size) for k in si.MASKS}
    outs = {"ws": ((nws,), torch.uint8)}
    for k in masks:
        outs[k] = (tuple(a.shape), F32)
        outs[k + "#2"] = (tuple(a.shape), F32)
    ar = Arena(dict(a=a, **{"m." + k: m for k, m in masks.items()}), outs, tail=4096)
    for k in masks:
        _smooth(ar, "a", k, sig, mode, n, size, nws, mask="m." + k)
        _smooth(ar, "a", k + "#2", sig, mode, n, size, nws, mask="m." + k)
    got = ar.fetch(workspace=("ws",))
    for k, m in masks.items():
        _check(got[k], a, sig, mode, B, mask=m, what=f"{si.case_id(case)} {k}")
        assert torch.equal(got[k].view(I32), got[k + "#2"].view(I32)), (k, "the second call")


BITS_CASES = (((3, 9, 8, 36), (1.0, 1.0, 1.0)), ((2, 5, 1, 36), (0.0, 2.5, 0.6)), ((3, 17, 12, 33), (3.0, 0.4, 4.0)),
              ((2, 4, 6, 40), (8.0, 8.0, 8.0)), ((2, 40, 72, 100), (2.265, 2.265, 2.265)))


@pytest.mark.parametrize("shape,sig", BITS_CASES, ids=lambda v: "x".join(f"{s:g}" for s in v))
def test_bits_do_not_depend_on_the_batch_or_the_access_path(shape, sig):
    """The last sample of a batch and the same sample alone give equal bits, with and without a mask (alone it is sample 0, whose
    workgroups also make G_hw(m)).  Where W % 4 == 0 the same batch through pointers 4 bytes off (one element per lane instead
    of 16 bytes) gives equal bits again."""
    B, size = shape[0], shape[1:]
    V = size[0] * size[1] * size[2]
    a, m = si.maps("heavy", B, size), si.mask("half", size)
    pad = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])              # the data from the second element on
    nws = _query("tmf_smooth_workspace_bytes", B, *size, 1)
    vec = size[2] % 4 == 0
    for mode in si.MODES:
        ins = {"a": a, "m": m, "last": a[B - 1:].clone(), "a+": pad(a), "m+": pad(m)}
        outs = {"ws": ((nws,), torch.uint8)}
        for tag in ("all", "all.m"):
            outs[tag] = (tuple(a.shape), F32)
            outs[tag.replace("all", "one")] = ((1,) + tuple(size), F32)
            outs[tag.replace("all", "off")] = ((B * V + 1,), F32)
        ar = Arena(ins, outs, tail=4096)
        for tag, mk in (("", None), (".m", "m")):
            _smooth(ar, "a", "all" + tag, sig, mode, B, size, nws, mask=mk)
            _smooth(ar, "last", "one" + tag, sig, mode, 1, size, nws, mask=mk)
            if vec:
                _smooth(ar, "a+", "off" + tag, sig, mode, B, size, nws, mask=mk and "m+", a_off=4, out_off=4, mask_off=4)
        live = torch.ones(B * V + 1, dtype=torch.bool)
        live[0] = False
        if not vec:
            live[:] = False
        got = ar.fetch(workspace=("ws",), written={"off": live, "off.m": live})
        for tag, mk in (("", None), (".m", m)):
            ref, bnd = si.reference(a, sig, mode, mk), si.bound(a, sig, mk)
            assert bool((np.abs(got["all" + tag].double().numpy() - ref) <= bnd).all()), (mode, tag)
            assert torch.equal(got["all" + tag][B - 1:].view(I32), got["one" + tag].view(I32)), (mode, tag, "alone")
            if vec:
                assert torch.equal(got["all" + tag].view(-1).view(I32), got["off" + tag][1:].view(I32)), (mode, tag, "4 bytes off")


def test_workload_volume():
    """B = 2 at 96^3, FWHM 8 mm at 1.5 mm (r = 9): 32-bit index math and grid sizing at the workload's own volume, against scipy
    where it is installed, else the numpy reference."""
    (B, *size), sig = si.WORKLOAD_CASE
    a = si.maps("normal", B, size)
    try:
        from scipy import ndimage
        ref = np.stack([ndimage.gaussian_filter(a[b].double().numpy(), sig, mode="reflect", truncate=si.TRUNCATE) for b in range(B)])
    except ImportError:
        ref = si.reference(a, sig, "reflect")
    nws = _query("tmf_smooth_workspace_bytes", B, *size, 0)
    ar = Arena({"a": a}, {"ws": ((nws,), torch.uint8), "out": (tuple(a.shape), F32)}, tail=4096)
    _smooth(ar, "a", "out", sig, "reflect", B, size, nws)
    got = ar.fetch(workspace=("ws",))["out"]
    err, bnd = np.abs(got.double().numpy() - ref), si.bound(a, sig)
    print(f"96^3: worst error / bound {float((err / bnd).max()):.3f}")
    assert bool((err <= bnd).all())


def test_entries_refuse_and_leave_the_arena_untouched():
    """Every refusal of include/tmf_hip.h with real device pointers: its TMF_E_*, nothing launched - no byte of the arena
    changes, the output slot keeps its fill pattern; tmf_smooth_workspace_bytes is 0 for the refused shapes."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    B, size = 2, (4, 5, 8)
    a, m = si.maps("normal", B, size), si.mask("half", size)
    nws = _query("tmf_smooth_workspace_bytes", B, *size, 1)
    ar = Arena({"a": a, "m": m}, {"ws": ((nws,), torch.uint8), "out": (tuple(a.shape), F32)}, tail=4096)
    A, M, O, WS = ar.ptr("a"), ar.ptr("m"), ar.ptr("out"), ar.ptr("ws")
    st = _st()

    def rc(a=A, mask=M, out=O, sig=(1.0, 1.0, 1.0), truncate=4.0, mode=0, ws=WS, n=nws, shape=(B,) + size):
        return lib.tmf_gaussian_smooth(a, mask, out, *sig, truncate, mode, ws, n, *shape, st)

    assert rc(a=None) == rc(out=None) == rc(ws=None) == _lib.E_NULL
    for shape in ((0,) + size, (65537,) + size, (B, 0, 5, 8), (B, 4, 0, 8), (B, 4, 5, 0), (1, 2048, 1024, 1024)):
        assert rc(shape=shape) == _lib.E_SHAPE, shape
        assert _query("tmf_smooth_workspace_bytes", *shape, 0) == 0 and _query("tmf_smooth_workspace_bytes", *shape, 1) == 0
    assert rc(mode=-1) == rc(mode=3) == _lib.E_ARG
    for sig in ((-1.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, float("inf")), (8.125, 1.0, 1.0)):
        assert rc(sig=sig) == _lib.E_ARG, sig
    for truncate in (0.0, -1.0, float("nan"), float("inf"), 33.0):
        assert rc(truncate=truncate) == _lib.E_ARG, truncate
    assert rc(a=A + 2) == rc(out=O + 2) == rc(mask=M + 2) == rc(ws=WS + 4) == _lib.E_ALIGN
    assert rc(out=A) == rc(out=A + 16) == rc(a=O + a.numel() * 4 - 4) == _lib.E_ARG            # out overlaps a
    assert rc(n=nws - 1) == _lib.E_WORKSPACE and rc(mask=None, n=_query("tmf_smooth_workspace_bytes", B, *size, 0) - 1) == _lib.E_WORKSPACE
    never = torch.zeros(tuple(a.shape), dtype=torch.bool)
    ar.fetch(workspace=("ws",), written={"out": never})
    ws_off, ws_n = ar.slots["ws"][:2]
    assert torch.equal(ar.dev[ws_off:ws_off + ws_n].cpu(), ar.host[ws_off:ws_off + ws_n]), "a refused call wrote the workspace"


@pytest.mark.parametrize("shape", ((2, 9, 8, 36), (3, 17, 12, 33), (1, 40, 72, 100)), ids=lambda s: "x".join(map(str, s)))
def test_gaussian_smooth_against_gaussian_smooth_torch(shape, monkeypatch):
    """The public function: ONE tmf_gaussian_smooth call for contiguous float32 maps, within twice the bound of
    gaussian_smooth_torch on the same device tensors; float64 and non-contiguous maps take the torch ops."""
    from transmf_ad_amd import _lib, gaussian_smooth, gaussian_smooth_torch
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    B, size = shape[0], shape[1:]
    a = si.maps("heavy", B, size)
    dev = a.to(DEV).view(B, 1, *size)
    lab = si.mask("bricks", size)
    for sig, mode, mask in (((1.0, 1.0, 1.0), "reflect", None), ((0.0, 2.5, 0.6), "constant", lab), ((3.0, 0.4, 4.0), "nearest", lab != 0),
                            ((2.265,) * 3, "reflect", lab.to(DEV))):
        del names[:]
        got = gaussian_smooth(dev, sigma=sig, mode=mode, mask=mask)
        assert names == ["tmf_gaussian_smooth"] and got.shape == dev.shape and got.dtype == F32 and got.device == dev.device
        twin = gaussian_smooth_torch(dev, sigma=sig, mode=mode, mask=mask)
        assert names == ["tmf_gaussian_smooth"] and twin.is_cuda
        bnd = torch.from_numpy(si.bound(a, sig, None if mask is None else lab)).view(B, 1, 1, 1, 1).to(DEV)
        assert bool(((got.double() - twin.double()).abs() <= 2 * bnd).all()), (sig, mode)
        ref = si.reference(a, sig, mode, None if mask is None else lab)
        assert bool((np.abs(got.view(B, *size).double().cpu().numpy() - ref) <= bnd.view(B, 1, 1, 1).cpu().numpy()).all())
        del names[:]
        g64 = gaussian_smooth(dev.double(), sigma=sig, mode=mode, mask=mask)
        assert names == [] and g64.dtype == torch.float64
        assert float((g64.view(B, *size).cpu() - torch.from_numpy(ref)).abs().max()) <= 1e-12 * float(a.abs().max())
    wide = torch.zeros((B, 1) + tuple(size[:2]) + (2 * size[2],), device=DEV)
    wide[..., ::2] = dev
    del names[:]
    gs = gaussian_smooth(wide[..., ::2], sigma=1.0)
    assert names == [] and torch.equal(gs, gaussian_smooth_torch(dev, sigma=1.0))


def test_blurred_baseline_and_smoothed_clusters_on_the_tiny_model():
    """faithfulness_curve(baseline="blur") gives the bits of the explicit tensor in `scores`; a smoothed |input gradient|
    (FWHM 8 mm at 1.5 mm) goes through clusters(top=0.05) and reports no more clusters than the unsmoothed map."""
    import transmf_ad_amd as T
    g = Golden("ad_tiny")
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    vols = [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)]
    attr = T.input_gradients(net, *vols)[0].abs()
    blur = T.gaussian_smooth(vols[0], sigma=T.smooth.BLUR_SIGMA)
    assert blur.shape == vols[0].shape and not torch.equal(blur, vols[0])
    for mode in ("deletion", "insertion"):
        a = T.faithfulness_curve(net, *vols, attribution=attr, volume=0, steps=5, mode=mode, baseline="blur")
        b = T.faithfulness_curve(net, *vols, attribution=attr, volume=0, steps=5, mode=mode, baseline=blur)
        assert torch.equal(a.scores.view(I32), b.scores.view(I32)) and torch.equal(a.removed, b.removed)
    smooth = T.gaussian_smooth(attr, fwhm=8.0, spacing=1.5)
    assert smooth.shape == attr.shape and float(smooth.min()) >= 0.0
    raw, cl = T.clusters(attr, top=0.05), T.clusters(smooth, top=0.05)
    assert int(cl.n.min()) >= 1 and bool((cl.n <= raw.n).all()), (cl.n.tolist(), raw.n.tolist())
