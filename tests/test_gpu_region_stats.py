"""Atlas region statistics on the device: the kernels of csrc/region_stats.hip on their own (through _lib.call with raw
pointers) against the numpy fp64 reference of tests/_region_inputs.py - count, max and argmax exactly, the sums within the
bound include/tmf_hip.h states (exactly on integer maps); equal bits between calls, batches and access paths; NULL outputs;
region_stats against region_stats_torch; the group accumulator against a numpy fp64 loop, bit for bit; and the whole chain on
the tiny 32^3 models.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs
and the bands around the workspace included) must be unchanged, every output element written."""
import numpy as np
import pytest
import torch

import _region_inputs as ri
from _golden import Golden
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _query, _st
from test_gpu_model import DEV, build
from test_host_region_stats import _group_ref

pytestmark = pytest.mark.gpu
F32, I32, F64, I64 = torch.float32, torch.int32, torch.float64, torch.int64
FLOATS = ("sum", "abs_sum", "pos_sum", "max")
OUTS = ("sum", "abs_sum", "pos_sum", "max", "argmax")


def _slots(tag, B, R, skip=()):
    s = {f"{tag}.count": ((R + 1,), I32)}
    for n in OUTS:
        s[f"{tag}.{n}"] = ((B, R + 1), I32 if n == "argmax" else F32)
    return s


def _stats(ar, tag, a, lab, B, V, R, nws, null=(), a_off=0, lab_off=0):
    ptr = lambda n: None if n in null else ar.ptr(f"{tag}.{n}")
    _call("tmf_region_stats", ar.ptr(a) + a_off, ar.ptr(lab) + lab_off, ar.ptr(f"{tag}.count"), *(ptr(n) for n in OUTS), ar.ptr("ws"),
          nws, B, V, R, _st())


def _live(tags, lab, R, B):
    """Arena.fetch's `written` for the argmax slots: -1, the value of an empty bin, is also the arena's fill pattern."""
    live = torch.from_numpy(np.bincount(ri.bins_of(lab, R), minlength=R + 1) > 0).expand(B, R + 1)
    return {f"{t}.argmax": live for t in tags}


def _named(got, tag, names=("count",) + OUTS):
    return {n: got[f"{tag}.{n}"] for n in names}


@pytest.mark.parametrize("case", ri.CASES, ids=ri.case_id)
def test_region_stats_kernel(case):
    """Every atlas x every map: count, max, argmax exact; the sums within n_r * peak_b * 2^-shift + 2^-23 * |exact|, exact on
    the integer and the zero maps; each run twice into separate outputs through ONE workspace: equal bits.  Out-of-range labels
    land in bin 0, an empty region gives (0, 0, 0, 0, -inf, -1), zero and constant maps give each bin's lowest index."""
    (B, *size), R = case
    V = size[0] * size[1] * size[2]
    nws = _query("tmf_region_workspace_bytes", B, V, R)
    assert nws > 0
    worst = 0.0
    for ak in ri.ATLASES:
        lab = ri.atlas(ak, size, R)
        ins = {"lab": lab}
        ins.update({mk: ri.maps(mk, B, size) for mk in ri.MAPS})
        outs = {"ws": ((nws,), torch.uint8)}
        for mk in ri.MAPS:
            outs.update(_slots(mk, B, R))
            outs.update(_slots(mk + "#2", B, R))
        ar = Arena(ins, outs, tail=4096)
        for mk in ri.MAPS:
            _stats(ar, mk, mk, "lab", B, V, R, nws)
            _stats(ar, mk + "#2", mk, "lab", B, V, R, nws)
        got = ar.fetch(workspace=("ws",), written=_live([t for mk in ri.MAPS for t in (mk, mk + "#2")], lab, R, B))
        bins = ri.bins_of(lab, R)
        first = np.array([np.flatnonzero(bins == r)[0] if (bins == r).any() else -1 for r in range(R + 1)])
        for mk in ri.MAPS:
            ref = ri.reference(ins[mk], lab, R)
            g = _named(got, mk)
            worst = max(worst, ri.check(g, ref, V, (ak, mk), exact_sums=mk in ("integers", "zero")))
            for n in ("count",) + OUTS:
                assert torch.equal(got[f"{mk}.{n}"].view(I32), got[f"{mk}#2.{n}"].view(I32)), (ak, mk, n, "the second call")
            if mk in ("zero", "constant"):
                assert np.array_equal(g["argmax"].numpy(), np.broadcast_to(first, (B, R + 1))), (ak, mk)
            if mk == "zero":
                live = ref["count"] > 0
                assert not g["sum"].any() and not g["abs_sum"].any() and not g["pos_sum"].any() and not g["max"][:, live].any()
            if mk == "negative":
                assert not g["pos_sum"].any()
            empty = ref["count"] == 0
            if empty.any():
                assert not g["sum"][:, empty].any() and not g["abs_sum"][:, empty].any() and not g["pos_sum"][:, empty].any()
                assert bool((g["max"][:, empty] == float("-inf")).all()) and bool((g["argmax"][:, empty] == -1).all())
        if ak == "empty_last":
            assert int(got["randn.count"][R]) == 0
        if ak == "out_of_range":
            inside = lab[(lab >= 0) & (lab <= R)]
            assert int(got["randn.count"][0]) == V - int((inside > 0).sum())
        if ak in ("single", "background"):
            assert int(got["randn.count"][1 if ak == "single" else 0]) == V
    print(f"{ri.case_id(case)}: worst error / bound of the sums {worst:.3f}")


@pytest.mark.parametrize("case", ri.CASES, ids=ri.case_id)
def test_bits_do_not_depend_on_the_batch_or_the_access_path(case):
    """Row 2 of a batch of 3 and the same sample alone give equal bits (the grid differs).  Where V % 4 == 0 the same batch
    through base pointers 4 bytes off (one element per lane instead of 16 bytes) gives equal bits again; 2 bytes off is refused."""
    from transmf_ad_amd import _lib
    (_b, *size), R = case
    V = size[0] * size[1] * size[2]
    B = 3
    nws = _query("tmf_region_workspace_bytes", B, V, R)
    for ak, mk in (("blocks", "decades"), ("random", "randn"), ("stripes", "signed_zeros")):
        lab, a = ri.atlas(ak, size, R), ri.maps(mk, B, size)
        pad = lambda t: torch.cat([t.reshape(-1)[:1], t.reshape(-1)])       # the data from the second element on
        ins = {"lab": lab, "a": a, "row2": a[2:3].clone(), "lab+": pad(lab), "a+": pad(a)}
        outs = {"ws": ((nws,), torch.uint8)}
        outs.update(_slots("all", B, R))
        outs.update(_slots("one", 1, R))
        outs.update(_slots("off", B, R))
        ar = Arena(ins, outs, tail=4096)
        _stats(ar, "all", "a", "lab", B, V, R, nws)
        _stats(ar, "one", "row2", "lab", 1, V, R, nws)
        _stats(ar, "off", "a+", "lab+", B, V, R, nws, a_off=4, lab_off=4)
        lib = _lib.load()
        ptrs = [ar.ptr(f"off.{n}") for n in ("count",) + OUTS]
        assert lib.tmf_region_stats(ar.ptr("a") + 2, ar.ptr("lab"), *ptrs, ar.ptr("ws"), nws, B, V, R, None) == _lib.E_ALIGN
        assert lib.tmf_region_stats(ar.ptr("a"), ar.ptr("lab") + 2, *ptrs, ar.ptr("ws"), nws, B, V, R, None) == _lib.E_ALIGN
        written = _live(("all", "off"), lab, R, B)
        written.update(_live(("one",), lab, R, 1))
        got = ar.fetch(workspace=("ws",), written=written)
        ri.check(_named(got, "all"), ri.reference(a, lab, R), V, (ak, mk))
        assert torch.equal(got["all.count"], got["one.count"]) and torch.equal(got["all.count"], got["off.count"])
        for n in OUTS:
            assert torch.equal(got[f"all.{n}"][2:3].view(I32), got[f"one.{n}"].view(I32)), (ak, mk, n, "alone")
            assert torch.equal(got[f"all.{n}"].view(I32), got[f"off.{n}"].view(I32)), (ak, mk, n, "4 bytes off")


@pytest.mark.parametrize("case", [c for c in ri.CASES if c[1] in (7, ri.REGION_MAX)], ids=ri.case_id)
def test_null_outputs(case):
    """Each of the five per-sample outputs NULL in turn, and all five: the others keep their bits, the slot of a NULL output
    and every band around the outputs and the workspace stay untouched."""
    (B, *size), R = case
    V = size[0] * size[1] * size[2]
    nws = _query("tmf_region_workspace_bytes", B, V, R)
    lab, a = ri.atlas("blocks", size, R), ri.maps("decades", B, size)
    runs = {"full": ()}
    runs.update({"no_" + n: (n,) for n in OUTS})
    runs["count_only"] = OUTS
    outs = {"ws": ((nws,), torch.uint8)}
    for tag in runs:
        outs.update(_slots(tag, B, R))
    ar = Arena({"lab": lab, "a": a}, outs, tail=4096)
    for tag, null in runs.items():
        _stats(ar, tag, "a", "lab", B, V, R, nws, null=null)
    never = {f"{tag}.{n}": torch.zeros((B, R + 1), dtype=torch.bool) for tag, null in runs.items() for n in null}
    written = _live([t for t, null in runs.items() if "argmax" not in null], lab, R, B)
    written.update(never)
    got = ar.fetch(workspace=("ws",), written=written)
    ri.check(_named(got, "full"), ri.reference(a, lab, R), V, "full")
    for tag, null in runs.items():
        for n in ("count",) + OUTS:
            if n not in null:
                assert torch.equal(got[f"{tag}.{n}"].view(I32), got[f"full.{n}"].view(I32)), (tag, n)


@pytest.mark.parametrize("case", ri.CASES, ids=ri.case_id)
def test_region_stats_against_region_stats_torch(case, monkeypatch):
    """The public function: the kernel for contiguous float32 maps (ONE tmf_region_stats call, no other library call), within
    the header's bound of the fp64 reference, as region_stats_torch on the device is within the stock ops' own; float64, bf16
    and non-contiguous maps take the torch ops and agree with numpy."""
    from transmf_ad_amd import _lib, region_stats, region_stats_torch
    from test_host_region_stats import _float_bound
    (B, *size), R = case
    V = size[0] * size[1] * size[2]
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    fields = lambda rs: dict(count=rs.count, sum=rs.sum, abs_sum=rs.abs_sum, pos_sum=rs.pos_sum, max=rs.max, argmax=rs.argmax)
    for ak, mk in (("blocks", "decades"), ("out_of_range", "randn"), ("empty_last", "integers")):
        lab, a = ri.atlas(ak, size, R), ri.maps(mk, B, size)
        ref = ri.reference(a, lab, R)
        dev = a.to(DEV)
        del names[:]
        rs = region_stats(dev.view(B, 1, *size), lab, R)
        assert names == ["tmf_region_stats"] and rs.sum.device == dev.device and rs.sum.dtype == F32
        ri.check(fields(rs), ref, V, (ak, mk, "kernel"), exact_sums=mk == "integers")
        rt = region_stats_torch(dev, lab.to(DEV), R)
        assert names == ["tmf_region_stats"] and rt.sum.is_cuda
        ri.check(fields(rt), ref, V, (ak, mk, "torch"), exact_sums=mk == "integers", sums_bound=_float_bound(F32))
        assert torch.equal(rs.count, rt.count) and torch.equal(rs.argmax, rt.argmax) and torch.equal(rs.max, rt.max)
        # shares sum to one; the views are torch ops on the small tensors
        if float(rs.abs_sum[:, 1:].sum(1).min()) > 0:
            assert float((rs.share("abs")[:, 1:].sum(1) - 1).abs().max()) <= 1e-6
        del names[:]
        r64 = region_stats(dev.double(), lab, R)
        ri.check(fields(r64), ri.reference(a.double(), lab, R), V, (ak, mk, "f64"), sums_bound=_float_bound(F64))
        wide = torch.zeros((B,) + tuple(size[:2]) + (2 * size[2],), device=DEV)
        wide[..., ::2] = dev
        strided = wide[..., ::2]
        assert V == 1 or not strided.is_contiguous()
        rn = region_stats(strided, lab, R)
        ri.check(fields(rn), ref, V, (ak, mk, "strided"), exact_sums=mk == "integers", sums_bound=_float_bound(F32))
        if V == 1:
            del names[:]                                                # one voxel is contiguous whatever its strides: the kernel
        h = dev.bfloat16()
        rh = region_stats(h, lab, R)
        ri.check(fields(rh), ri.reference(h, lab, R), V, (ak, mk, "bf16"),
                 sums_bound=lambda ref, name: 2.0 ** -8 * np.abs(ref[name]) + _float_bound(F32)(ref, name))
        assert names == [] and r64.sum.dtype == F64 and rh.max.dtype == torch.bfloat16


@pytest.mark.parametrize("C", (1, 2, 16))
def test_group_update_kernel(C):
    """tmf_region_group_update against the numpy fp64 loop, bit for bit, on a state that already holds sums; classes -1 and C
    are skipped; (B, R) values leave bin 0 alone; two updates equal one update of the concatenation."""
    g = torch.Generator().manual_seed(90 + C)
    for R, B in ((1, 1), (7, 37), (116, 300), (ri.REGION_MAX, 5)):
        start = torch.randn((C, R + 1, 3), generator=g, dtype=F64).abs()
        v1, v2 = (0.3 + torch.randn((B, R + 1), generator=g) for _ in range(2))
        y1, y2 = (torch.randint(-1, C + 1, (B,), generator=g) for _ in range(2))
        vr = torch.randn((B, R), generator=g)
        ins = dict(v1=v1, v2=v2, y1=y1, y2=y2, vr=vr, v12=torch.cat([v1, v2]), y12=torch.cat([y1, y2]))
        ar = Arena(ins, {k: ((C, R + 1, 3), F64) for k in ("two", "one", "cols")}, tail=4096)
        for k in ("two", "one", "cols"):
            off, n = ar.slots[k][:2]
            ar.dev[off:off + n] = start.view(-1).view(torch.uint8).to(DEV)
        _call("tmf_region_group_update", ar.ptr("v1"), ar.ptr("y1"), ar.ptr("two"), B, R, C, 0, _st())
        _call("tmf_region_group_update", ar.ptr("v2"), ar.ptr("y2"), ar.ptr("two"), B, R, C, 0, _st())
        _call("tmf_region_group_update", ar.ptr("v12"), ar.ptr("y12"), ar.ptr("one"), 2 * B, R, C, 0, _st())
        _call("tmf_region_group_update", ar.ptr("vr"), ar.ptr("y1"), ar.ptr("cols"), B, R, C, 1, _st())
        got = ar.fetch()
        want = _group_ref(_group_ref(start.numpy().copy(), v1.numpy(), y1.numpy()), v2.numpy(), y2.numpy())
        assert np.array_equal(got["two"].numpy(), want), (R, B)
        assert torch.equal(got["two"], got["one"])
        want = _group_ref(start.numpy().copy(), vr.numpy(), y1.numpy())
        assert np.array_equal(got["cols"].numpy(), want) and torch.equal(got["cols"][:, 0], start[:, 0])


def test_accumulator_on_the_device(monkeypatch):
    """RegionAccumulator on float32 HIP values: one library call per update and nothing else of the library; compute() matches
    numpy.mean, numpy.std(ddof=1) and Welch's t to 1e-12; float64 values take the torch ops into the same state."""
    from transmf_ad_amd import RegionAccumulator, _lib
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    R, g = 9, torch.Generator().manual_seed(12)
    x = (0.3 + torch.rand((48, R + 1), generator=g)).to(F32)
    y = torch.randint(0, 2, (48,), generator=g)
    x[y == 1, 4] += 0.25
    acc = RegionAccumulator(R)
    for at in range(0, 48, 16):
        acc.update(x[at:at + 16].to(DEV), y[at:at + 16].to(DEV))
    assert names == ["tmf_region_group_update"] * 3
    out = acc.compute()
    xs = [x[y == c].double().numpy() for c in (0, 1)]
    for c in (0, 1):
        assert out["n"][c].tolist() == [len(xs[c])] * (R + 1)
        assert np.allclose(out["mean"][c].numpy(), xs[c].mean(0), rtol=1e-12, atol=0)
        assert np.allclose(out["std"][c].numpy(), xs[c].std(0, ddof=1), rtol=1e-12, atol=0)
    t = (xs[1].mean(0) - xs[0].mean(0)) / np.sqrt(xs[1].var(0, ddof=1) / len(xs[1]) + xs[0].var(0, ddof=1) / len(xs[0]))
    assert np.allclose(out["t"].numpy(), t, rtol=1e-12, atol=0)
    before = acc.state_dict()["state"]
    acc.update(x[:4].double().to(DEV), y[:4].to(DEV))
    assert names == ["tmf_region_group_update"] * 3
    want = _group_ref(before.numpy().copy(), x[:4].numpy(), y[:4].numpy())
    assert np.allclose(acc.state_dict()["state"].numpy(), want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", ("cnn_tiny", "ad_tiny"))
def test_end_to_end_on_the_tiny_models(name):
    """grad_cam(...).volume() and input_gradients(...) of the 32^3 fixtures through region_stats: the shares of the regions sum
    to one per sample; occlusion's (B, R) drops with the same atlas go straight into a RegionAccumulator."""
    import transmf_ad_amd as T
    g = Golden(name)
    net = build(g, inject_masks=False).eval()
    mri, pet, y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    vols = [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)]
    R = 7
    atlas = ri.atlas("blocks", g.size, R)
    cams = T.grad_cam(net, *vols, layer="conv3", relu=False, normalize=False)
    maps = {"grad_cam": cams.volume(cams.encoders[0], "conv3"), "input_gradients": T.input_gradients(net, *vols)[0]}
    for what, m in maps.items():
        rs = T.region_stats(m, atlas)
        assert rs.R == R and rs.sum.shape == (g.batch, R + 1) and rs.sum.is_cuda and int(rs.count.sum()) == 32 ** 3
        ref = ri.reference(m.reshape(g.batch, -1), atlas, R)
        ri.check(dict(count=rs.count, sum=rs.sum, abs_sum=rs.abs_sum, pos_sum=rs.pos_sum, max=rs.max, argmax=rs.argmax), ref, 32 ** 3, what)
        for kind in ("abs", "pos"):
            sh = rs.share(kind)
            mass = (rs.abs_sum if kind == "abs" else rs.pos_sum)[:, 1:].sum(1)
            assert bool(torch.isfinite(sh).all()) and float(mass.min()) > 0, (what, kind)
            assert float((sh[:, 1:].sum(1) - 1).abs().max()) <= 1e-6, (what, kind)
        zyx = rs.peak_voxel(1)
        assert bool((atlas.to(DEV)[zyx[:, 0], zyx[:, 1], zyx[:, 2]] == 1).all())
        assert len(rs.table()) == g.batch * (R + 1)
    occ = T.occlusion_sensitivity(net, *vols, atlas=atlas, volumes=(0,))
    drops = occ.drops(0)
    assert tuple(drops.shape) == (g.batch, R)
    label = torch.from_numpy(np.asarray(y)).to(DEV).long().view(-1) % 2
    acc = T.RegionAccumulator(R)
    acc.update(drops, label)
    out = acc.compute()
    assert out["n"][:, 0].tolist() == [0.0, 0.0] and float(out["n"][:, 1:].sum()) == g.batch * R
    for c in (0, 1):
        sel = drops[label == c].double().cpu()
        if len(sel):
            assert torch.allclose(out["mean"][c, 1:], sel.mean(0), rtol=1e-12, atol=1e-300)
