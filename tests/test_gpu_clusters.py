"""Connected clusters on the device: the kernels of csrc/clusters.hip on their own (through _lib.call with raw pointers) against
the numpy reference of tests/_cluster_inputs.py - labels, n_clusters and the five table outputs EQUAL for every shape, mask,
connectivity and mode; equal bits between two calls through one workspace; n_clusters never -1; min_size; K below, at and above
n; NULL outputs; labels from anywhere; the 4-bytes-off `a`; clusters() against clusters_torch; top= with its device-side
threshold; and the whole chain on the tiny 32^3 model.

Every buffer of the kernel tests lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the inputs and the
bands around the workspace included) must be unchanged, every output element written."""
import numpy as np
import pytest
import torch

import _cluster_inputs as ci
from _golden import Golden
from oracle import params as P
from test_gpu_bn_reduce import Arena, _call, _query, _st
from test_gpu_model import DEV, build
from test_host_clusters import FIELDS, same

pytestmark = pytest.mark.gpu
F32, I32, I64 = torch.float32, torch.int32, torch.int64
MODE = {"pos": 0, "neg": 1, "abs": 2}


def _label_slots(tag, shape):
    return {f"{tag}.labels": (tuple(shape), I32), f"{tag}.n": ((shape[0],), I32)}


def _table_slots(tag, B, K):
    """coord_sum is int64 [B][K][3]; the arena knows 2- and 4-byte words, so its slot is declared as int32 [B][K][6]."""
    return {f"{tag}.size": ((B, K), I32), f"{tag}.peak": ((B, K), F32), f"{tag}.argmax": ((B, K), I32),
            f"{tag}.coord_sum": ((B, K, 6), I32), f"{tag}.bbox": ((B, K, 6), I32)}


def _label(ar, tag, a, shape, mode, conn, min_size, nws, a_off=0):
    _call("tmf_cluster_label", ar.ptr(a) + a_off, ar.ptr("thr"), ar.ptr(f"{tag}.labels"), ar.ptr(f"{tag}.n"), ar.ptr("ws"), nws,
          *shape, MODE[mode], conn, min_size, _st())


def _table(ar, tag, a, labels, shape, mode, K, null=(), a_off=0):
    ptr = lambda n: None if n in null else ar.ptr(f"{tag}.{n}")
    _call("tmf_cluster_table", ar.ptr(a) + a_off, ar.ptr(labels), *(ptr(n) for n in FIELDS), *shape, MODE[mode], K, _st())


def _written(tag, ref, null=()):
    """Arena.fetch's `written`: -1, the argmax and the upper box of an empty row, is also the arena's fill pattern; a NULL output
    keeps the pattern everywhere."""
    w = {f"{tag}.argmax": torch.from_numpy(ref["argmax"] != -1), f"{tag}.bbox": torch.from_numpy(ref["bbox"] != -1)}
    for n in null:
        shape = ref[n].shape[:2] + ((6,) if n in ("coord_sum", "bbox") else ())
        w[f"{tag}.{n}"] = torch.zeros(shape, dtype=torch.bool)
    return w


def _check_table(got, tag, ref, what, null=()):
    for n in FIELDS:
        if n in null:
            continue
        g = got[f"{tag}.{n}"]
        g = g.contiguous().view(I64).view(ref[n].shape) if n == "coord_sum" else g
        same(g.numpy(), ref[n], (what, n))


def _thr(B):
    return torch.full((B,), ci.THR, dtype=F32)


@pytest.mark.parametrize("mk", ci.MASKS)
@pytest.mark.parametrize("shape", ci.SHAPES, ids=ci.shape_id)
def test_label_and_table_kernels(shape, mk):
    """Every connectivity x mode of one mask (the value kinds in turn): labels, n_clusters, size, peak, argmax, coord_sum and bbox
    equal the reference; each call is made twice into separate outputs through ONE workspace: equal bits; n_clusters is never
    -1.  The table reads the labels the label entry wrote."""
    B = shape[0]
    nws = _query("tmf_cluster_workspace_bytes", *shape)
    assert nws > 0
    i = ci.MASKS.index(mk)
    runs, ins, outs = [], {"thr": _thr(B)}, {"ws": ((nws,), torch.uint8)}
    for conn in ci.CONNECTIVITIES:
        lab, n = ci.labels_of(mk, shape, conn)
        K = max(1, int(n.max()))
        for j, mode in enumerate(ci.MODES):
            vk = ci.VALUES[(i + j) % len(ci.VALUES)]
            a = ci.values(vk, mk, shape, mode)
            ins[f"{vk}.{mode}"] = torch.from_numpy(a.copy())
            tag = f"{conn}.{mode}"
            runs.append((tag, f"{vk}.{mode}", conn, mode, K, lab, n, ci.reference_table(a, lab, mode, K)))
            for t in (tag, tag + "#2"):
                outs.update(_label_slots(t, shape))
                outs.update(_table_slots(t, B, K))
    ar = Arena(ins, outs, tail=4096)
    for tag, a, conn, mode, K, *_ in runs:
        for t in (tag, tag + "#2"):
            _label(ar, t, a, shape, mode, conn, 1, nws)
            _table(ar, t, a, f"{t}.labels", shape, mode, K)
    written = {}
    for tag, *_rest, ref in runs:
        written.update(_written(tag, ref))
        written.update(_written(tag + "#2", ref))
    got = ar.fetch(workspace=("ws",), may_nan=[f"{t}.peak" for tag, *_ in runs for t in (tag, tag + "#2")], written=written)
    for tag, a, conn, mode, K, lab, n, ref in runs:
        what = (mk, a, conn)
        assert int(got[f"{tag}.n"].min()) >= 0, what
        same(got[f"{tag}.n"].numpy(), n, what)
        same(got[f"{tag}.labels"].numpy(), lab, what)
        _check_table(got, tag, ref, what)
        for name in ("labels", "n") + FIELDS:
            assert torch.equal(got[f"{tag}.{name}"].view(I32), got[f"{tag}#2.{name}"].view(I32)), (what, name, "the second call")


@pytest.mark.parametrize("mk", ("random10", "random31", "comb", "diagonals"))
def test_min_size(mk):
    """min_size 1, 2 and 50: the smaller clusters become background, the others are renumbered consecutively."""
    shape = ci.SHAPES[-1]
    B = shape[0]
    nws = _query("tmf_cluster_workspace_bytes", *shape)
    a = ci.values("randn", mk, shape, "abs")
    cases = [(conn, m) for conn in (6, 26) for m in (1, 2, 50)]
    outs = {"ws": ((nws,), torch.uint8)}
    for conn, m in cases:
        outs.update(_label_slots(f"{conn}.{m}", shape))
    ar = Arena({"thr": _thr(B), "a": torch.from_numpy(a.copy())}, outs, tail=4096)
    for conn, m in cases:
        _label(ar, f"{conn}.{m}", "a", shape, "abs", conn, m, nws)
    got = ar.fetch(workspace=("ws",))
    for conn, m in cases:
        lab, n = ci.labels_of(mk, shape, conn, m)
        same(got[f"{conn}.{m}.n"].numpy(), n, (mk, conn, m))
        same(got[f"{conn}.{m}.labels"].numpy(), lab, (mk, conn, m))


def test_table_rows_null_outputs_and_labels_from_anywhere():
    """K below, at and above n; each of the five outputs NULL in turn, and all five: the others keep their bits, the slot of a
    NULL output and every band stay untouched; labels that no cluster_label wrote - negative, above K, an empty row inside."""
    shape = ci.SHAPES[-1]
    B = shape[0]
    a = ci.values("randn", "random31", shape, "neg")
    lab, n = ci.labels_of("random31", shape, 6)
    top = int(n.max())
    assert int(n.min()) > 8 and int(n.min()) < top
    rng = np.random.default_rng(23)
    wild = rng.integers(-3, 40, shape).astype(np.int32)
    wild[wild == 7] = 0
    runs = [(f"K{K}", "lab", K, ()) for K in (1, int(n.min()) - 3, int(n.min()), top, top + 9)]
    runs += [("no_" + f, "lab", top, (f,)) for f in FIELDS] + [("none", "lab", top, FIELDS), ("wild", "wild", 33, ())]
    outs = {}
    for tag, _l, K, _null in runs:
        outs.update(_table_slots(tag, B, K))
    ar = Arena({"a": torch.from_numpy(a.copy()), "lab": torch.from_numpy(lab.copy()), "wild": torch.from_numpy(wild)}, outs, tail=4096)
    for tag, l, K, null in runs:
        _table(ar, tag, "a", l, shape, "neg", K, null=null)
    refs = {tag: ci.reference_table(a, wild if l == "wild" else lab, "neg", K) for tag, l, K, _null in runs}
    written = {}
    for tag, _l, _K, null in runs:
        written.update(_written(tag, refs[tag], null))
    got = ar.fetch(may_nan=[f"{tag}.peak" for tag, *_ in runs], written=written)
    for tag, _l, _K, null in runs:
        _check_table(got, tag, refs[tag], tag, null)
    assert int(refs["wild"]["size"][0, 6]) == 0 and int(refs["wild"]["argmax"][0, 6]) == -1


def test_a_four_bytes_off():
    """The same batch through a base pointer 4 bytes off a 16-byte boundary gives equal bits; 2 bytes off is refused."""
    from transmf_ad_amd import _lib
    shape = (2, 8, 12, 36)                                            # V % 4 == 0
    B = shape[0]
    nws = _query("tmf_cluster_workspace_bytes", *shape)
    a = torch.from_numpy(ci.values("randn", "random31", shape, "pos").copy())
    lab, n = ci.labels_of("random31", shape, 18)
    K = int(n.max())
    outs = {"ws": ((nws,), torch.uint8)}
    for t in ("on", "off"):
        outs.update(_label_slots(t, shape))
        outs.update(_table_slots(t, B, K))
    ar = Arena({"thr": _thr(B), "a": a, "a+": torch.cat([a.reshape(-1)[:1], a.reshape(-1)])}, outs, tail=4096)
    for t, name, off in (("on", "a", 0), ("off", "a+", 4)):
        _label(ar, t, name, shape, "pos", 18, 1, nws, a_off=off)
        _table(ar, t, name, f"{t}.labels", shape, "pos", K, a_off=off)
    lib = _lib.load()
    assert lib.tmf_cluster_label(ar.ptr("a") + 2, ar.ptr("thr"), ar.ptr("off.labels"), ar.ptr("off.n"), ar.ptr("ws"), nws, *shape, 0, 18, 1,
                                 None) == _lib.E_ALIGN
    ref = ci.reference_table(a.numpy(), lab, "pos", K)
    written = {**_written("on", ref), **_written("off", ref)}
    got = ar.fetch(workspace=("ws",), may_nan=("on.peak", "off.peak"), written=written)
    same(got["on.labels"].numpy(), lab, "on")
    same(got["on.n"].numpy(), n, "on")
    _check_table(got, "on", ref, "on")
    for name in ("labels", "n") + FIELDS:
        assert torch.equal(got[f"on.{name}"].view(I32), got[f"off.{name}"].view(I32)), name


@pytest.mark.parametrize("shape", ci.SHAPES[1:], ids=ci.shape_id)
def test_clusters_against_clusters_torch(shape, monkeypatch):
    """The public function on device tensors: the kernels for contiguous float32 maps (tmf_cluster_label and tmf_cluster_table and
    nothing else of the library; tmf_rank_thresholds in front for top=), identical to clusters_torch on the device and to the
    reference; top= with its device-side threshold equals threshold= with the same number; float64 and non-contiguous maps take
    the torch ops."""
    from transmf_ad_amd import _lib, clusters, clusters_torch
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (names.append(name), real(name, *args))[1])
    B = shape[0]
    for mk, mode, conn, min_size in (("random31", "pos", 6, 1), ("random50", "abs", 26, 1), ("random10", "neg", 18, 2), ("snake", "abs", 6, 1)):
        a = ci.values("zeros_nan", mk, shape, mode)
        lab, n = ci.labels_of(mk, shape, conn, min_size)
        dev = torch.from_numpy(a.copy()).to(DEV)
        del names[:]
        cl = clusters(dev.unsqueeze(1), threshold=ci.THR, mode=mode, connectivity=conn, min_size=min_size)
        assert names == ["tmf_cluster_label", "tmf_cluster_table"] and cl.labels.is_cuda and cl.n.is_cuda
        ct = clusters_torch(dev, threshold=torch.full((B,), ci.THR, device=DEV), mode=mode, connectivity=conn, min_size=min_size)
        assert names == ["tmf_cluster_label", "tmf_cluster_table"]
        what = (mk, mode, conn)
        same(cl.labels.cpu().numpy(), lab, what)
        same(cl.n.cpu().numpy(), n, what)
        ref = ci.reference_table(a, lab, mode, cl.K)
        for f in ("labels", "n") + FIELDS:
            assert getattr(cl, f).dtype == getattr(ct, f).dtype and getattr(cl, f).shape == getattr(ct, f).shape, (what, f)
            same(getattr(cl, f).cpu().numpy(), getattr(ct, f).cpu().numpy(), (what, f))
        for f in FIELDS:
            same(getattr(cl, f).cpu().numpy(), ref[f], (what, f))
        assert len(cl.table()) == int(n.sum())
        few = clusters(dev, threshold=ci.THR, mode=mode, connectivity=conn, min_size=min_size, max_clusters=2)
        assert few.K == min(2, a[0].size) and torch.equal(few.labels, cl.labels) and torch.equal(few.size[:, :cl.K], cl.size[:, :few.K])
        del names[:]
        r64 = clusters(dev.double(), threshold=ci.THR, mode=mode, connectivity=conn, min_size=min_size)
        wide = torch.zeros(tuple(shape[:3]) + (2 * shape[3],), device=DEV)
        wide[..., ::2] = dev
        rn = clusters(wide[..., ::2], threshold=ci.THR, mode=mode, connectivity=conn, min_size=min_size)
        assert names == [] and r64.peak.dtype == torch.float64
        for r in (r64, rn):
            assert torch.equal(r.labels, cl.labels) and torch.equal(r.argmax, cl.argmax) and torch.equal(r.bbox, cl.bbox)
    # top=: the threshold stays on the device
    g = torch.Generator().manual_seed(7)
    x = torch.randn(shape, generator=g)
    V = x[0].numel()
    for mode in ci.MODES:
        for top in (0.01, 0.05, 1.0):
            count = int(np.ceil(top * V))
            thr = torch.stack([ci_score(v, mode).reshape(-1).sort(descending=True).values[count - 1] for v in x])
            del names[:]
            ct = clusters(x.to(DEV), top=top, mode=mode, connectivity=18)
            assert names == ["tmf_rank_thresholds", "tmf_cluster_label", "tmf_cluster_table"]
            cn = clusters(x.to(DEV), threshold=thr.to(DEV), mode=mode, connectivity=18)
            lab, n = ci.reference_clusters(x.numpy(), thr.numpy(), mode, 18)
            same(ct.labels.cpu().numpy(), lab, (mode, top))
            same(ct.n.cpu().numpy(), n, (mode, top))
            for f in ("labels", "n") + FIELDS:
                same(getattr(ct, f).cpu().numpy(), getattr(cn, f).cpu().numpy(), (mode, top, f))


def ci_score(v, mode):
    return v if mode == "pos" else -v if mode == "neg" else v.abs()


def test_end_to_end_on_the_tiny_model():
    """input_gradients of the 32^3 fixture -> clusters(top=0.05) -> cl.stats(map): the voxel counts of the bins equal cl.size;
    occlusion_sensitivity with the label volume as its atlas returns one drop per cluster."""
    import transmf_ad_amd as T
    g = Golden("ad_tiny")
    net = build(g, inject_masks=False).eval()
    mri, pet, _y = P.make_inputs(g.batch, g.size, seed=1234, kind="blobs")
    vols = [torch.from_numpy(mri).to(DEV), torch.from_numpy(pet).to(DEV)]
    m = T.input_gradients(net, *vols)[0]
    cl = T.clusters(m, top=0.05, mode="abs", connectivity=26, min_size=4)
    n = cl.n.cpu()
    assert int(n.min()) >= 1 and cl.K == int(n.max()) and cl.labels.shape == (g.batch, 32, 32, 32)
    flat = m.reshape(g.batch, -1)
    lab, want_n = ci.reference_clusters(m.reshape(g.batch, 32, 32, 32).cpu().numpy(),
                                        np.array([np.sort(np.abs(r))[::-1][int(np.ceil(0.05 * 32 ** 3)) - 1] for r in flat.cpu().numpy()]),
                                        "abs", 26, 4)
    same(cl.labels.cpu().numpy(), lab, "labels")
    same(n.numpy(), want_n, "n")
    stats = cl.stats(m)
    for b, rs in enumerate(stats):
        assert rs.R == min(cl.K, T.ops.REGION_MAX) and torch.equal(rs.count[1:], cl.size[b, :rs.R])
        k = int(n[b])
        assert torch.equal(rs.abs_sum[0, 1:k + 1] > 0, torch.ones(k, dtype=torch.bool, device=DEV))
    zyx = cl.peak_voxel(1)
    assert bool((cl.labels[torch.arange(g.batch), zyx[:, 0], zyx[:, 1], zyx[:, 2]] == 1).all())
    occ = T.occlusion_sensitivity(net, *vols, atlas=cl.labels[0], volumes=(0,))
    assert tuple(occ.drops(0).shape) == (g.batch, int(n[0]))
