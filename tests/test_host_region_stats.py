"""Atlas region statistics without a device: region_stats_torch (and region_stats, which takes the same torch ops on the CPU)
against the numpy fp64 reference of tests/_region_inputs.py on every atlas and map; the derived views; every ValueError; the
entries' refusals (no launch is reached); the workspace size; the accumulator against numpy and its state_dict; the new names
in the header, the ctypes prototypes, the documents and the package."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _region_inputs as ri

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"tmf_region_workspace_bytes": 3, "tmf_region_stats": 14, "tmf_region_group_update": 8}
HOST_CASES = [((2, 5, 6, 7), 3), ((2, 5, 6, 7), 116), ((1, 1, 1, 1), 1), ((3, 8, 8, 8), 7)]


def _float_bound(dtype):
    """Stock ops add in the tensor's precision in an order of their own: n_r roundings of at most eps * sum |a| each."""
    eps = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}[dtype]
    return lambda ref, name: (ref["count"][None, :] + 1) * eps * ref["abs_sum"]


@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("case", HOST_CASES, ids=ri.case_id)
def test_torch_path_against_numpy(case, dtype):
    from transmf_ad_amd import region_stats, region_stats_torch
    (B, *size), R = case
    V = size[0] * size[1] * size[2]
    for ak in ri.ATLASES:
        lab = ri.atlas(ak, size, R)
        for mk in ri.MAPS:
            a = ri.maps(mk, B, size).to(dtype)
            ref = ri.reference(a, lab, R)
            for fn in (region_stats_torch, region_stats):
                rs = fn(a.view(B, 1, *size) if fn is region_stats else a, lab.long() if mk == "zero" else lab, R)
                assert rs.R == R and rs.size == tuple(size) and rs.sum.dtype == rs.max.dtype == dtype
                assert rs.count.dtype == rs.argmax.dtype == torch.int32 and rs.count.shape == (R + 1,)
                assert rs.sum.shape == rs.abs_sum.shape == rs.pos_sum.shape == rs.max.shape == rs.argmax.shape == (B, R + 1)
                got = dict(count=rs.count, sum=rs.sum, abs_sum=rs.abs_sum, pos_sum=rs.pos_sum, max=rs.max, argmax=rs.argmax)
                ri.check(got, ref, V, (ak, mk), exact_sums=mk in ("integers", "zero"), sums_bound=_float_bound(dtype))
            if ak == "empty_last":
                assert int(rs.count[R]) == 0 and bool((rs.max[:, R] == float("-inf")).all()) and bool((rs.argmax[:, R] == -1).all())
                assert not bool(rs.sum[:, R].any() or rs.abs_sum[:, R].any() or rs.pos_sum[:, R].any())
            if mk in ("zero", "constant"):
                first = torch.tensor([int(np.flatnonzero(ri.bins_of(lab, R) == r)[0]) if int(rs.count[r]) else -1 for r in range(R + 1)])
                assert torch.equal(rs.argmax.long(), first.expand(B, R + 1))
            if mk == "negative":
                assert not bool(rs.pos_sum.any()) and bool((rs.max[:, rs.count > 0] < 0).all())
    # R defaults to the atlas maximum; out-of-range labels land in bin 0
    lab = ri.atlas("out_of_range", size, R)
    inside = lab[(lab >= 0) & (lab <= R)]
    rs = region_stats_torch(ri.maps("randn", B, size), lab, R)
    assert int(rs.count.sum()) == V and int(rs.count[0]) == V - int((inside > 0).sum())
    lab = ri.atlas("random", size, R)
    assert region_stats(ri.maps("randn", B, size), lab).R == int(lab.max())


def test_bf16_and_non_contiguous_take_the_torch_ops():
    from transmf_ad_amd import region_stats
    B, size, R = 2, (5, 6, 7), 7
    lab = ri.atlas("blocks", size, R)
    a = ri.maps("randn", B, size)
    wide = torch.zeros((B,) + size[:2] + (2 * size[2],))
    wide[..., ::2] = a
    rs, rc = region_stats(wide[..., ::2], lab, R), region_stats(a, lab, R)
    for name in ("count", "sum", "abs_sum", "pos_sum", "max", "argmax"):
        assert torch.equal(getattr(rs, name), getattr(rc, name)), name
    h = a.bfloat16()
    rs = region_stats(h, lab, R)
    ref = ri.reference(h, lab, R)
    assert rs.sum.dtype == rs.max.dtype == torch.bfloat16
    got = dict(count=rs.count, sum=rs.sum, abs_sum=rs.abs_sum, pos_sum=rs.pos_sum, max=rs.max, argmax=rs.argmax)
    # added up in float32, rounded once to bf16 (8 significand bits)
    ri.check(got, ref, 210, "bf16", sums_bound=lambda ref, name: 2.0 ** -8 * np.abs(ref[name]) + _float_bound(torch.float32)(ref, name))


def test_derived_views():
    from transmf_ad_amd import RegionStats, region_stats_torch
    size, R = (2, 3, 4), 3
    lab = torch.tensor([0, 1, 1, 2] * 6).view(size)                   # region 3 is empty
    a = torch.zeros((2,) + size, dtype=torch.float64)
    a[0].view(-1)[:] = torch.arange(24.0) - 10                           # sample 1 stays zero: no mass
    rs = region_stats_torch(a, lab)
    assert rs.R == 2
    rs = region_stats_torch(a, lab, R)
    assert isinstance(rs, RegionStats) and rs.count.tolist() == [6, 12, 6, 0]
    x = (torch.arange(24.0) - 10).double()
    sel = [x[lab.view(-1) == r] for r in range(4)]
    assert rs.mean[0].tolist() == [float(s.mean()) if len(s) else 0.0 for s in sel] and rs.mean[1].tolist() == [0.0] * 4
    for kind, f in (("abs", torch.abs), ("pos", lambda t: t.clamp(min=0))):
        mass = [float(f(s).sum()) for s in sel]
        want = [m / (mass[1] + mass[2]) for m in mass]
        assert torch.allclose(rs.share(kind)[0], torch.tensor(want, dtype=torch.float64), rtol=1e-15, atol=0)
        assert rs.share(kind)[1].tolist() == [0.0] * 4 and not bool(torch.isnan(rs.share(kind)).any())
        assert abs(float(rs.share(kind)[0, 1:].sum()) - 1) < 1e-15
    assert rs.max[0].tolist() == [10.0, 12.0, 13.0, float("-inf")] and rs.argmax[0].tolist() == [20, 22, 23, -1]
    assert rs.argmax[1].tolist() == [0, 1, 3, -1]
    assert rs.peak_voxel(1).tolist() == [[1, 2, 2], [0, 0, 1]] and rs.peak_voxel(3).tolist() == [[-1] * 3] * 2
    assert rs.peak_voxel(0).tolist() == [[1, 2, 0], [0, 0, 0]]
    idx, val = rs.top(2)
    assert idx[0].tolist() == [1, 2] and torch.equal(val[0], rs.share("abs")[0, 1:3]) and idx.shape == val.shape == (2, 2)
    idx, val = rs.top(3, by="pos")
    assert idx[0].tolist() == [1, 2, 3] and float(val[0, 2]) == 0.0
    rows = rs.table()
    assert len(rows) == 2 * 4 and [r["region"] for r in rows[:4]] == [0, 1, 2, 3] and [r["sample"] for r in rows] == [0] * 4 + [1] * 4
    assert rows[1] == dict(sample=0, region=1, name="1", count=12, sum=float(sel[1].sum()), abs_sum=float(sel[1].abs().sum()),
                           pos_sum=float(sel[1].clamp(min=0).sum()), mean=float(sel[1].mean()), max=12.0, argmax=22,
                           share_abs=float(rs.share("abs")[0, 1]), share_pos=float(rs.share("pos")[0, 1]))
    assert rows[3]["count"] == 0 and rows[3]["max"] == float("-inf") and rows[3]["argmax"] == -1 and rows[3]["mean"] == 0.0
    names = ["background", "hippocampus", "amygdala", "insula"]
    assert [r["name"] for r in rs.table(names)[:4]] == names
    assert [r["name"] for r in rs.table({1: "hippocampus"})[:4]] == ["0", "hippocampus", "2", "3"]
    for bad in (lambda: rs.table(names[:3]), lambda: rs.share("neg"), lambda: rs.top(0), lambda: rs.top(4), lambda: rs.top(2, by="x"),
                lambda: rs.peak_voxel(4), lambda: rs.peak_voxel(-1), lambda: rs.peak_voxel(1.0)):
        with pytest.raises(ValueError):
            bad()


def test_value_errors():
    from transmf_ad_amd import RegionAccumulator, ops, region_stats, region_stats_torch
    size = (3, 4, 5)
    a, lab = torch.randn((2,) + size), ri.atlas("random", size, 4)
    for fn in (region_stats, region_stats_torch):
        for bad in (dict(atlas=lab.float()), dict(atlas=lab.bool()), dict(atlas=lab[:2]), dict(atlas=lab.view(-1)), dict(atlas=None),
                    dict(R=0), dict(R=-3), dict(R=2.0), dict(R=True), dict(attribution=a.view(2, -1)), dict(attribution=a.long()),
                    dict(attribution=a.view(1, 2, *size)), dict(attribution=None), dict(atlas=torch.zeros(size, dtype=torch.int64))):
            kw = dict(attribution=a, atlas=lab, R=4)
            kw.update(bad)
            if "atlas" in bad and torch.is_tensor(bad["atlas"]) and not bad["atlas"].any() and bad["atlas"].dtype == torch.int64:
                kw["R"] = None                                      # an atlas without a label above 0
            with pytest.raises(ValueError):
                fn(**kw)
    with pytest.raises(ValueError, match="limit"):
        region_stats(a, lab, ops.REGION_MAX + 1)
    assert region_stats_torch(a, lab, ops.REGION_MAX + 1).sum.shape == (2, ops.REGION_MAX + 2)
    for bad in (lambda: RegionAccumulator(0), lambda: RegionAccumulator(3, 0), lambda: RegionAccumulator(2.0), lambda: RegionAccumulator(3, True)):
        with pytest.raises(ValueError):
            bad()
    acc = RegionAccumulator(4)
    y = torch.tensor([0, 1])
    for v, l in ((torch.zeros(2, 3), y), (torch.zeros(2, 6), y), (torch.zeros(5), y), (torch.zeros(2, 5), y[:1]), (torch.zeros(2, 5), y.float()),
                 (torch.zeros(2, 5, dtype=torch.int64), y), (None, y), (torch.zeros(2, 5), None)):
        with pytest.raises(ValueError):
            acc.update(v, l)
    with pytest.raises(RuntimeError):
        acc.compute()


def _group_ref(state, values, cls):
    """The loop the entry replaces, in numpy fp64, in place: values (B, R+1) or (B, R)."""
    C, first = state.shape[0], state.shape[1] - values.shape[1]
    for b in range(values.shape[0]):
        c = int(cls[b])
        if 0 <= c < C:
            x = values[b].astype(np.float64)
            state[c, first:, 0] += 1.0
            state[c, first:, 1] += x
            state[c, first:, 2] += x * x
    return state


@pytest.mark.parametrize("C", (1, 2, 16))
def test_accumulator_against_numpy(C):
    from transmf_ad_amd import RegionAccumulator
    R, g = 7, torch.Generator().manual_seed(40 + C)
    acc, ref = RegionAccumulator(R, num_classes=C), np.zeros((C, R + 1, 3))
    for B, cols, dtype in ((9, R + 1, torch.float32), (1, R + 1, torch.float64), (14, R, torch.float32), (6, R + 1, torch.float32)):
        v = (0.4 + torch.randn((B, cols), generator=g)).to(dtype)
        y = torch.randint(-1, C + 1, (B,), generator=g)                 # -1 and C: skipped
        acc.update(v, y)
        _group_ref(ref, v.numpy(), y.numpy())
    st = acc.state_dict()
    assert st["R"] == R and st["num_classes"] == C and np.allclose(st["state"].numpy(), ref, rtol=1e-15, atol=0)
    assert ref[:, 0, 0].sum() < ref[:, 1, 0].sum()                                # the (B, R) update left column 0 alone
    out = acc.compute()
    n, sx, sxx = ref[..., 0], ref[..., 1], ref[..., 2]
    assert np.array_equal(out["n"].numpy(), n) and set(out) == ({"n", "mean", "std", "t"} if C == 2 else {"n", "mean", "std"})
    with np.errstate(all="ignore"):
        mean = np.where(n > 0, sx / np.maximum(n, 1), 0)
        var = np.where(n > 1, np.maximum(sxx - sx * sx / np.maximum(n, 1), 0) / np.maximum(n - 1, 1), 0)
    assert np.allclose(out["mean"].numpy(), mean, rtol=1e-14, atol=0) and np.allclose(out["std"].numpy(), np.sqrt(var), rtol=1e-13, atol=0)
    # state_dict round trip: a second accumulator resumes and ends with the same bits
    other = RegionAccumulator(R, num_classes=C)
    other.load_state_dict(st)
    v, y = torch.randn((5, R + 1), generator=g), torch.randint(0, C, (5,), generator=g)
    acc.update(v, y)
    other.update(v, y)
    assert torch.equal(acc.state_dict()["state"], other.state_dict()["state"])
    with pytest.raises(ValueError):
        RegionAccumulator(R + 1, num_classes=C).load_state_dict(st)
    acc.reset()
    assert not bool(acc.state_dict()["state"].any())
    fresh = RegionAccumulator(R, num_classes=C)
    fresh.load_state_dict(fresh.state_dict())
    with pytest.raises(RuntimeError):
        fresh.compute()


def test_compute_against_numpy_mean_std_and_welch():
    from transmf_ad_amd import RegionAccumulator
    R, g = 5, torch.Generator().manual_seed(3)
    x = 0.3 + torch.rand((40, R + 1), generator=g, dtype=torch.float64)
    y = torch.randint(0, 2, (40,), generator=g)
    x[y == 1, 2] += 0.25
    acc = RegionAccumulator(R)
    for at in range(0, 40, 8):
        acc.update(x[at:at + 8], y[at:at + 8])
    out = acc.compute()
    xs = [x[y == c].numpy() for c in (0, 1)]
    for c in (0, 1):
        assert out["n"][c].tolist() == [len(xs[c])] * (R + 1)
        assert np.allclose(out["mean"][c].numpy(), xs[c].mean(0), rtol=1e-12, atol=0)
        assert np.allclose(out["std"][c].numpy(), xs[c].std(0, ddof=1), rtol=1e-12, atol=0)
    t = (xs[1].mean(0) - xs[0].mean(0)) / np.sqrt(xs[1].var(0, ddof=1) / len(xs[1]) + xs[0].var(0, ddof=1) / len(xs[0]))
    assert np.allclose(out["t"].numpy(), t, rtol=1e-12, atol=0) and abs(float(out["t"][2])) > 3
    one = RegionAccumulator(R)
    one.update(x[:1], y[:1] * 0)
    o = one.compute()
    assert o["std"].tolist() == [[0.0] * (R + 1)] * 2 and bool(torch.isnan(o["t"]).all()) and o["mean"][1].tolist() == [0.0] * (R + 1)


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no launch is reached: these run without a device), header, documents
# ---------------------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    """Every entry returns the negative TMF_E_* the header states - before any launch, so no device is needed and the (never
    dereferenced) device pointers here are made up."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    a, l, c, s1, s2, s3, mx, am, w = (i << 20 for i in range(1, 10))
    B, V, R = 2, 512, 7
    nws = lib.tmf_region_workspace_bytes(B, V, R)
    stats = lambda *args: lib.tmf_region_stats(*args, None)
    good = (a, l, c, s1, s2, s3, mx, am, w)
    for i in (0, 1, 2, 8):
        args = list(good)
        args[i] = None
        assert stats(*args, nws, B, V, R) == _lib.E_NULL, i
    for b, v in ((0, V), (-1, V), ((1 << 16) + 1, V), (B, 0), (B, -5), (B, 1 << 31)):
        assert stats(*good, 1 << 40, b, v, R) == _lib.E_SHAPE, (b, v)
    for r in (0, -1, _lib.REGION_MAX + 1):
        assert stats(*good, 1 << 40, B, V, r) == _lib.E_ARG, r
    assert stats(*good, nws - 1, B, V, R) == _lib.E_WORKSPACE
    for i in range(9):
        args = list(good)
        args[i] += 2
        assert stats(*args, nws, B, V, R) == _lib.E_ALIGN, i
    args = list(good)
    args[8] += 4                                                       # the workspace: 16 bytes
    assert stats(*args, nws, B, V, R) == _lib.E_ALIGN
    assert b"tmf_region_stats" in lib.tmf_last_error_string()
    v, y, st = 1 << 20, 2 << 20, 3 << 20
    group = lambda *args: lib.tmf_region_group_update(*args, None)
    for args in ((None, y, st), (v, None, st), (v, y, None)):
        assert group(*args, B, R, 2, 0) == _lib.E_NULL
    for b in (0, -1, (1 << 16) + 1):
        assert group(v, y, st, b, R, 2, 0) == _lib.E_SHAPE
    for r, cc, first in ((0, 2, 0), (_lib.REGION_MAX + 1, 2, 0), (R, 0, 0), (R, 17, 0), (R, 2, 2), (R, 2, -1)):
        assert group(v, y, st, B, r, cc, first) == _lib.E_ARG, (r, cc, first)
    for args in ((v + 2, y, st), (v, y + 4, st), (v, y, st + 4)):
        assert group(*args, B, R, 2, 0) == _lib.E_ALIGN
    assert b"tmf_region_group_update" in lib.tmf_last_error_string()


def test_workspace_bytes():
    from transmf_ad_amd import _lib
    lib = _lib.load()
    f = lib.tmf_region_workspace_bytes
    for bad in ((0, 512, 7), (-1, 512, 7), ((1 << 16) + 1, 512, 7), (2, 0, 7), (2, -1, 7), (2, 1 << 31, 7), (2, 512, 0),
                (2, 512, _lib.REGION_MAX + 1)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1) > 0 and f(1, 1, 1) % 16 == 0
    sizes = [[f(B, 96 ** 3, R) for R in (1, 7, 116, _lib.REGION_MAX)] for B in (1, 2, 8, 65536)]
    assert all(a < b for row in sizes for a, b in zip(row, row[1:])) and all(a < b for col in zip(*sizes) for a, b in zip(col, col[1:]))
    assert f(8, 96 ** 3, 116) == f(8, 5, 116) and f(8, 96 ** 3, 116) >= 8 * 117 * 24 + 117 * 4 + 8 * 4       # no term in V
    assert f(8, 96 ** 3, 116) < 1 << 16


def test_new_names_in_header_library_binding_and_documents():
    from transmf_ad_amd import _lib, build, ops
    import transmf_ad_amd as T
    with open(os.path.join(ROOT, "include", "tmf_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        rows = [l for l in f if l.startswith("| **`tmf_region_stats`**") or l.startswith("| **`tmf_region_group_update`**")]
    assert len(rows) == 2
    stated = {name: int(n) for row in rows for name, n in re.findall(r"`(tmf_region\w*)`[^|`]*?\((\d+) arguments?\)", row)}
    assert stated == ENTRIES
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES["tmf_region_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.REGION_MAX, _lib.REGION_MAX_CLASSES) == (ri.REGION_MAX, 16) == (ops.REGION_MAX, ops.REGION_MAX_CLASSES)
    assert "2^-shift" in header and "2^-23" in header                      # the bound the tests assert
    assert "region_stats.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "region_stats.hip"))
    for fn in ("region_ok", "region_stats", "region_stats_torch", "region_group_update"):
        assert callable(getattr(ops, fn)), fn
    for name in ("region_stats", "region_stats_torch", "RegionStats", "RegionAccumulator"):
        assert name in T.__all__ and callable(getattr(T, name)), name
    for doc, words in (("DESIGN.md", ("3.31", "tmf_region_stats", "tmf_region_group_update", "region_stats_mi355x.txt")),
                       ("README.md", ("region_stats", "RegionAccumulator", "tmf_region_stats")),
                       ("INTEGRATION.md", ("tmf_region_stats", "tmf_region_group_update")),
                       (os.path.join("profiles", "README.md"), ("region_stats_mi355x.txt", "region_time.py"))):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert all(w in text for w in words), doc
    assert os.path.exists(os.path.join(ROOT, "profiles", "region_stats_mi355x.txt"))
    assert os.path.exists(os.path.join(ROOT, "tools", "region_time.py"))
