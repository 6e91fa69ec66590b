"""Connected clusters without a device: the numpy reference of tests/_cluster_inputs.py against scipy.ndimage.label; clusters_torch
(and clusters, which takes the same torch ops on the CPU) against that reference on every shape, mask, connectivity and mode -
labels, n and the table, compared with ==; top= against a numpy sort; min_size; max_clusters; the derived views; cl.stats against
region_stats_torch; every ValueError; the entries' refusals (no launch is reached); the new names in the header, the ctypes
prototypes, the documents and the package."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _cluster_inputs as ci

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"tmf_cluster_workspace_bytes": 4, "tmf_cluster_label": 14, "tmf_cluster_table": 14}
FIELDS = ("size", "peak", "argmax", "coord_sum", "bbox")


def same(got, want, what):
    """Equal element by element; NaN equals NaN (the peak of an empty row), -0.0 does not equal +0.0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == "f":
        bits = {4: np.int32, 8: np.int64}[got.dtype.itemsize]
        both_nan = np.isnan(got) & np.isnan(want)
        assert np.array_equal(np.where(both_nan, 0, got.view(bits)), np.where(both_nan, 0, want.view(bits))), what
    else:
        assert np.array_equal(got, want), what


def check_table(cl, ref, what):
    for name in FIELDS:
        same(getattr(cl, name).cpu().numpy(), ref[name], (what, name))


@pytest.mark.parametrize("shape", ci.SHAPES, ids=ci.shape_id)
def test_reference_against_scipy(shape):
    ndimage = pytest.importorskip("scipy.ndimage")
    for mk in ci.MASKS:
        for conn, rank in ((6, 1), (18, 2), (26, 3)):
            lab, n = ci.labels_of(mk, shape, conn)
            for b, m in enumerate(ci.mask(mk, shape)):
                want, k = ndimage.label(m, ndimage.generate_binary_structure(3, rank))
                assert k == n[b] and np.array_equal(want, lab[b]), (mk, conn, b)


def test_masks_are_what_they_claim():
    big = ci.SHAPES[-1]
    V = big[1] * big[2] * big[3]
    assert all(s > t for s, t in zip(big[1:], ci.TILE))                           # a tile boundary in each axis
    assert [int(ci.labels_of("checker", big, c)[1][0]) for c in ci.CONNECTIVITIES] == [(V + 1) // 2, 1, 1]
    assert [int(ci.labels_of("snake", big, c)[1][0]) for c in ci.CONNECTIVITIES] == [1, 1, 1]
    assert [int(ci.labels_of("comb", big, c)[1][0]) for c in ci.CONNECTIVITIES] == [1, 1, 1]
    n6, n18, n26 = (int(ci.labels_of("diagonals", big, c)[1][0]) for c in ci.CONNECTIVITIES)
    assert n6 > n18 > n26 > 0                                                     # edges and corners tell the three apart
    assert ci.labels_of("two_samples", big, 26)[1].tolist() == [1, 0]
    for mode in ci.MODES:
        for vk in ci.VALUES:
            a = ci.values(vk, "random31", big, mode)
            assert np.array_equal(ci.foreground(a, [ci.THR] * big[0], mode), ci.mask("random31", big)), (mode, vk)
    z = ci.values("zeros_nan", "random31", big, "pos")
    assert np.isnan(z).sum() >= 2 and (np.signbit(z) & (z == 0)).any()


@pytest.mark.parametrize("conn", ci.CONNECTIVITIES)
@pytest.mark.parametrize("shape", ci.SHAPES, ids=ci.shape_id)
def test_clusters_torch_against_the_reference(shape, conn):
    """Every mask x mode (the value kinds in turn): labels, n and the five table outputs equal the reference; clusters on CPU
    tensors is the same function."""
    from transmf_ad_amd import clusters, clusters_torch
    for i, mk in enumerate(ci.MASKS):
        lab, n = ci.labels_of(mk, shape, conn)
        for j, mode in enumerate(ci.MODES):
            vk = ci.VALUES[(i + j) % len(ci.VALUES)]
            a = ci.values(vk, mk, shape, mode)
            cl = clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, mode=mode, connectivity=conn)
            what = (mk, mode, vk)
            same(cl.labels.numpy(), lab, what)
            same(cl.n.numpy(), n, what)
            K = max(1, int(n.max()))
            assert cl.K == K
            check_table(cl, ci.reference_table(a, lab, mode, K), what)
        c2 = clusters(torch.from_numpy(a.copy()).unsqueeze(1), threshold=torch.full((shape[0],), ci.THR), mode=mode, connectivity=conn)
        assert torch.equal(c2.labels, cl.labels) and torch.equal(c2.size, cl.size) and torch.equal(c2.argmax, cl.argmax)


@pytest.mark.parametrize("dtype", (torch.float64, torch.bfloat16), ids=("f64", "bf16"))
def test_other_dtypes(dtype):
    from transmf_ad_amd import clusters
    shape = ci.SHAPES[1]
    a = torch.from_numpy(ci.values("randn", "random31", shape, "abs").copy()).to(dtype)
    cl = clusters(a, threshold=ci.THR, mode="abs", connectivity=18)
    lab, n = ci.labels_of("random31", shape, 18)
    same(cl.labels.numpy(), lab, dtype)
    assert cl.peak.dtype == dtype and cl.labels.dtype == torch.int32 and cl.coord_sum.dtype == torch.int64
    ref = ci.reference_table(a.double().numpy(), lab, "abs", cl.K)
    assert np.array_equal(cl.peak.double().numpy(), ref["peak"]) and np.array_equal(cl.argmax.numpy(), ref["argmax"])


@pytest.mark.parametrize("mode", ci.MODES)
def test_top_against_a_numpy_sort(mode):
    """top=p: the threshold of sample b is its ceil(p*V)-th largest s(a); ties go together."""
    from transmf_ad_amd import clusters_torch
    rng = np.random.default_rng(5)
    a = rng.standard_normal((3, 6, 7, 9)).astype(np.float32)
    a[1] = np.round(a[1] * 2) / 2                                     # many ties
    V = a[0].size
    for top in (0.01, 0.05, 0.5, 1.0):
        count = int(np.ceil(top * V))
        thr = np.array([np.sort(ci.score(x, mode).reshape(-1))[::-1][count - 1] for x in a], np.float32)
        lab, n = ci.reference_clusters(a, thr, mode, 26)
        cl = clusters_torch(torch.from_numpy(a), top=top, mode=mode)
        same(cl.labels.numpy(), lab, (mode, top))
        same(cl.n.numpy(), n, (mode, top))
        assert all(int((l > 0).sum()) >= count for l in cl.labels.numpy())
    assert int((clusters_torch(torch.from_numpy(a), top=0.5, mode=mode).labels[1] > 0).sum()) > int(np.ceil(0.5 * V))      # the ties


def test_min_size_renumbers_consecutively():
    from transmf_ad_amd import clusters_torch
    shape = ci.SHAPES[-1]
    a = ci.values("randn", "random10", shape, "pos")
    every = clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, connectivity=6)
    for min_size in (2, 3, 50):
        lab, n = ci.labels_of("random10", shape, 6, min_size)
        cl = clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, connectivity=6, min_size=min_size)
        same(cl.labels.numpy(), lab, min_size)
        same(cl.n.numpy(), n, min_size)
        for b in range(shape[0]):
            kept = every.size[b][: int(every.n[b])] >= min_size
            assert int(kept.sum()) == int(n[b])
            assert torch.equal(cl.size[b][: int(n[b])], every.size[b][: int(every.n[b])][kept])      # the same clusters, in order
            assert np.array_equal(np.unique(cl.labels[b].numpy()), np.arange(int(n[b]) + 1))
    assert int(clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, connectivity=6, min_size=50).n.max()) == 0


def test_max_clusters_below_n_and_above():
    from transmf_ad_amd import clusters_torch
    shape = ci.SHAPES[1]
    a = ci.values("randn", "random31", shape, "neg")
    lab, n = ci.labels_of("random31", shape, 6)
    assert int(n.min()) > 4
    for K in (1, 3, int(n.max()), int(n.max()) + 5):
        cl = clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, mode="neg", connectivity=6, max_clusters=K)
        same(cl.labels.numpy(), lab, K)                               # clusters above K keep their labels
        assert cl.K == K
        check_table(cl, ci.reference_table(a, lab, "neg", K), K)
        assert len(cl.table()) == int(np.minimum(n, K).sum())
    assert clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, mode="neg", max_clusters=10 ** 9).K == a[0].size


def test_derived_views():
    from transmf_ad_amd import clusters_torch
    shape = ci.SHAPES[1]
    B, D, H, W = shape
    a = ci.values("randn", "random31", shape, "abs")
    cl = clusters_torch(torch.from_numpy(a.copy()), threshold=ci.THR, mode="abs", connectivity=6)
    lab, n = ci.labels_of("random31", shape, 6)
    ref = ci.reference_table(a, lab, "abs", cl.K)
    cen = cl.centroid.numpy()
    assert cen.dtype == np.float64
    for b in range(B):
        for k in range(cl.K):
            at = np.argwhere(lab[b] == k + 1)
            if len(at):
                assert np.array_equal(cen[b, k], at.sum(0) / len(at))
                assert np.array_equal(ref["bbox"][b, k], np.concatenate([at.min(0), at.max(0)]))
                assert tuple(cl.peak_voxel(k + 1)[b].tolist()) == np.unravel_index(ref["argmax"][b, k], (D, H, W))
                assert abs(a[b].reshape(-1)[ref["argmax"][b, k]]) == np.abs(a[b][lab[b] == k + 1]).max()
            else:
                assert np.isnan(cen[b, k]).all() and cl.peak_voxel(k + 1)[b].tolist() == [-1, -1, -1]
    for by, key in (("size", ref["size"].astype(np.float64)),
                    ("peak", np.where(ref["size"] > 0, np.abs(ref["peak"]).astype(np.float64), -np.inf))):
        order = cl.order(by).numpy()
        for b in range(B):
            want = sorted(range(cl.K), key=lambda k: (-np.nan_to_num(key[b, k], nan=-np.inf), k))
            assert order[b].tolist() == [k + 1 for k in want], by
    rows = cl.table()
    assert len(rows) == int(n.sum()) and [r["sample"] for r in rows] == sorted(r["sample"] for r in rows)
    r = rows[0]
    assert r["cluster"] == 1 and r["size"] == int(ref["size"][0, 0]) and r["peak"] == float(ref["peak"][0, 0])
    assert r["bbox"] == tuple(ref["bbox"][0, 0].tolist()) and r["centroid"] == tuple(cen[0, 0].tolist())
    assert r["peak_voxel"] == np.unravel_index(ref["argmax"][0, 0], (D, H, W))
    # constant maps: every peak ties, the lowest index of the cluster wins
    c = ci.values("constant", "random31", shape, "pos")
    cc = clusters_torch(torch.from_numpy(c.copy()), threshold=ci.THR, connectivity=6)
    for b in range(B):
        firsts = [int(np.flatnonzero(lab[b].reshape(-1) == k + 1)[0]) for k in range(int(n[b]))]
        assert cc.argmax[b][: int(n[b])].tolist() == firsts and firsts == sorted(firsts)


def test_stats_agree_with_region_stats_torch():
    from transmf_ad_amd import clusters_torch, ops, region_stats_torch
    shape = ci.SHAPES[1]
    a = torch.from_numpy(ci.values("randn", "random31", shape, "pos").copy())
    other = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    cl = clusters_torch(a, threshold=ci.THR, connectivity=18)
    stats = cl.stats(other.unsqueeze(1))
    assert len(stats) == shape[0]
    for b, rs in enumerate(stats):
        want = region_stats_torch(other[b:b + 1], cl.labels[b], R=min(cl.K, ops.REGION_MAX))
        for f in ops.REGION_FIELDS:
            assert torch.equal(getattr(rs, f), getattr(want, f)), f
        assert torch.equal(rs.count[1:], cl.size[b])
        assert torch.equal(cl.stats(a)[b].max[0, 1: int(cl.n[b]) + 1], cl.peak[b, : int(cl.n[b])])
    with pytest.raises(ValueError):
        cl.stats(other[:, :-1])


def test_value_errors():
    from transmf_ad_amd import clusters, clusters_torch, ops
    a = torch.randn(2, 4, 5, 6)
    for fn in (clusters, clusters_torch):
        for bad in (a[0], a.long(), torch.randn(2, 2, 4, 5, 6), torch.randn(0, 4, 5, 6), "x"):
            with pytest.raises(ValueError):
                fn(bad, threshold=0.5)
        for kw in ({}, dict(threshold=0.5, top=0.1), dict(threshold="0.5"), dict(threshold=torch.zeros(3)), dict(threshold=torch.zeros(2, dtype=torch.long)),
                   dict(top=0.0), dict(top=1.5), dict(top=-0.1), dict(top=True), dict(threshold=0.5, mode="both"),
                   dict(threshold=0.5, connectivity=8), dict(threshold=0.5, connectivity="26"), dict(threshold=0.5, min_size=0),
                   dict(threshold=0.5, min_size=1.5), dict(threshold=0.5, max_clusters=0), dict(threshold=0.5, max_clusters=2.0)):
            with pytest.raises(ValueError):
                fn(a, **kw)
    cl = clusters_torch(a, threshold=0.5)
    for bad in (0, cl.K + 1, True, 1.0):
        with pytest.raises(ValueError):
            cl.peak_voxel(bad)
    with pytest.raises(ValueError):
        cl.order("volume")
    thr = torch.zeros(2)
    for args in ((a[0], thr), (a, torch.zeros(3)), (a, thr, "both"), (a, thr, "pos", 8), (a, thr, "pos", 6, 0)):
        for fn in (ops.cluster_label, ops.cluster_label_torch):
            with pytest.raises(ValueError):
                fn(*args)
    lab = torch.zeros(2, 4, 5, 6, dtype=torch.int32)
    for args in ((a, lab[0]), (a, lab.float()), (a, lab, "both"), (a, lab, "pos", 0), (a, lab, "pos", 121), (a, lab, "pos", True)):
        for fn in (ops.cluster_table, ops.cluster_table_torch):
            with pytest.raises(ValueError):
                fn(*args)
    nan = clusters_torch(a, threshold=float("nan"))
    assert int(nan.n.max()) == 0 and not nan.labels.any() and nan.K == 1 and nan.table() == []
    assert bool(torch.isnan(nan.peak).all()) and nan.argmax.tolist() == [[-1], [-1]] and nan.bbox[0, 0].tolist() == [4, 5, 6, -1, -1, -1]


def test_labels_from_anywhere():
    """cluster_table_torch on labels that did not come from cluster_label: labels outside 1..K are ignored, rows may be empty."""
    from transmf_ad_amd import ops
    rng = np.random.default_rng(11)
    shape = ci.SHAPES[1]
    a = rng.standard_normal(shape).astype(np.float32)
    lab = rng.integers(-3, 12, shape).astype(np.int32)
    lab[lab == 4] = 0                                                  # an empty row inside
    for mode in ci.MODES:
        ref = ci.reference_table(a, lab, mode, 9)
        got = ops.cluster_table(torch.from_numpy(a), torch.from_numpy(lab), mode, 9)
        for name, g in zip(FIELDS, got):
            same(g.numpy(), ref[name], (mode, name))
        assert int(ref["size"][0, 3]) == 0 and int(ref["argmax"][0, 3]) == -1


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no launch is reached: these run without a device), header, documents
# ---------------------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    """Every entry returns the negative TMF_E_* the header states - before any launch, so no device is needed and the (never
    dereferenced) device pointers here are made up."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    a, thr, lab, n, ws, size, peak, arg, cs, bbox = (i << 20 for i in range(1, 11))
    B, D, H, W = 2, 9, 10, 40
    nws = lib.tmf_cluster_workspace_bytes(B, D, H, W)
    label = lambda *args: lib.tmf_cluster_label(*args, None)
    good = (a, thr, lab, n, ws)
    tail = (B, D, H, W, 0, 26, 1)
    for i in range(5):
        args = list(good)
        args[i] = None
        assert label(*args, nws, *tail) == _lib.E_NULL, i
    for shape in ((0, D, H, W), (-1, D, H, W), ((1 << 16) + 1, D, H, W), (B, 0, H, W), (B, D, -1, W), (B, D, H, 0),
                  (B, 1 << 11, 1 << 10, 1 << 10), (1, (1 << 31) - 1, 2, 1)):
        assert label(*good, 1 << 60, *shape, 0, 26, 1) == _lib.E_SHAPE, shape
    for mode, conn, min_size in ((-1, 26, 1), (3, 26, 1), (0, 0, 1), (0, 8, 1), (0, 27, 1), (0, 26, 0), (0, 26, -4)):
        assert label(*good, nws, B, D, H, W, mode, conn, min_size) == _lib.E_ARG, (mode, conn, min_size)
    assert label(*good, nws - 1, *tail) == _lib.E_WORKSPACE
    for i in range(5):
        args = list(good)
        args[i] += 2
        assert label(*args, nws, *tail) == _lib.E_ALIGN, i
    args = list(good)
    args[4] += 4                                                       # the workspace: 16 bytes
    assert label(*args, nws, *tail) == _lib.E_ALIGN
    assert b"tmf_cluster_label" in lib.tmf_last_error_string()
    table = lambda *args: lib.tmf_cluster_table(*args, None)
    outs = (size, peak, arg, cs, bbox)
    for args in ((None, lab), (a, None)):
        assert table(*args, *outs, B, D, H, W, 0, 5) == _lib.E_NULL
    for shape in ((0, D, H, W), ((1 << 16) + 1, D, H, W), (B, 0, H, W), (B, D, H, -2), (B, 1 << 11, 1 << 10, 1 << 10)):
        assert table(a, lab, *outs, *shape, 0, 5) == _lib.E_SHAPE, shape
    for mode, K in ((-1, 5), (3, 5), (0, 0), (0, -1), (0, D * H * W + 1)):
        assert table(a, lab, *outs, B, D, H, W, mode, K) == _lib.E_ARG, (mode, K)
    every = [a, lab, *outs]
    for i in range(7):
        args = list(every)
        args[i] += 2
        assert table(*args, B, D, H, W, 0, 5) == _lib.E_ALIGN, i
    args = list(every)
    args[5] += 4                                                       # coord_sum: 8 bytes
    assert table(*args, B, D, H, W, 0, 5) == _lib.E_ALIGN
    assert b"tmf_cluster_table" in lib.tmf_last_error_string()


def test_workspace_bytes():
    from transmf_ad_amd import _lib
    f = _lib.load().tmf_cluster_workspace_bytes
    for bad in ((0, 4, 4, 4), (-1, 4, 4, 4), ((1 << 16) + 1, 4, 4, 4), (2, 0, 4, 4), (2, 4, -1, 4), (2, 4, 4, 0), (1, 1 << 11, 1 << 10, 1 << 10)):
        assert f(*bad) == 0, bad
    assert f(1, 1, 1, 1) > 0 and f(1, 1, 1, 1) % 16 == 0
    V = 96 ** 3
    assert 8 * 8 * V <= f(8, 96, 96, 96) <= 8 * 8 * V + 8 * 4 * (V // 2048 + 2) + 16      # parents, sizes and a little
    assert f(2, 96, 96, 96) < f(3, 96, 96, 96) and f(2, 96, 96, 96) < f(2, 96, 96, 97)
    assert f(1, (1 << 31) - 1, 1, 1) > 0


def test_new_names_in_header_library_binding_and_documents():
    from transmf_ad_amd import _lib, build, ops
    import transmf_ad_amd as T
    with open(os.path.join(ROOT, "include", "tmf_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES["tmf_cluster_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.CLUSTER_POS, _lib.CLUSTER_NEG, _lib.CLUSTER_ABS) == (0, 1, 2)
    assert ops.CLUSTER_MODES == {"pos": 0, "neg": 1, "abs": 2}
    assert "clusters.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "clusters.hip"))
    for fn in ("cluster_ok", "cluster_label", "cluster_label_torch", "cluster_table", "cluster_table_torch"):
        assert callable(getattr(ops, fn)), fn
    for name in ("clusters", "clusters_torch", "Clusters"):
        assert name in T.__all__ and callable(getattr(T, name)), name
    for doc, words in (("DESIGN.md", ("3.32", "tmf_cluster_label", "tmf_cluster_table", "clusters_mi355x.txt")),
                       ("README.md", ("clusters(", "tmf_cluster_label", "clusters_mi355x.txt")),
                       ("INTEGRATION.md", ("tmf_cluster_label", "tmf_cluster_table")),
                       (os.path.join("profiles", "README.md"), ("clusters_mi355x.txt", "cluster_time.py"))):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert all(w in text for w in words), doc
    assert os.path.exists(os.path.join(ROOT, "profiles", "clusters_mi355x.txt"))
    assert os.path.exists(os.path.join(ROOT, "tools", "cluster_time.py"))
