"""Deletion / insertion curves without a device: ops.rank_counts; the torch formulas of ops.rank_thresholds / ops.mask_by_rank
against a plain Python loop; faithfulness_curve_torch on a module whose curves are closed-form; ties, -0.0, baseline against
fill; every ValueError; the caller's state; the entries' refusals (no launch is reached); the committed fixtures' keep rule;
the new names in the header, the ctypes prototypes, the documents and the package."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import _faithfulness_inputs as fi
from _golden import GOLDEN_DIR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"tmf_rank_workspace_bytes": 3, "tmf_rank_thresholds": 10, "tmf_mask_by_rank": 13}


def test_rank_counts():
    from transmf_ad_amd import ops
    for V, steps in ((1, 1), (1, 8), (5, 64), (105, 8), (32768, 20), (43890, 64), (884736, 20), (7, 7), (8, 3)):
        c = ops.rank_counts(V, steps)
        assert c == fi.counts_ref(V, steps) and len(c) == steps and c[-1] == V and c[0] >= 1
        assert all(a <= b for a, b in zip(c, c[1:]))
        assert all(n == -(-k * V // steps) for k, n in enumerate(c, 1))
    assert ops.rank_counts(1, 5) == [1] * 5
    assert ops.rank_counts(3, 7) == [1, 1, 2, 2, 3, 3, 3]                  # V < steps: repeated counts
    assert ops.rank_counts(10, 4) == [3, 5, 8, 10]
    for V, steps in ((0, 4), (-1, 4), (10, 0), (10, 65), (10.0, 4), (10, 4.0), (True, 4)):
        with pytest.raises(ValueError):
            ops.rank_counts(V, steps)


@pytest.mark.parametrize("kind", fi.VALUE_SETS)
def test_torch_formulas_against_a_python_loop(kind):
    """ops.rank_thresholds and ops.mask_by_rank on CPU tensors (their torch path) and the references of the GPU tests, against
    sorted() and comparisons of Python floats."""
    from transmf_ad_amd import ops
    B, V, S = 2, 37, 5
    attr = fi.values(kind, B, V)
    counts = ops.rank_counts(V, S)
    thr, removed = ops.rank_thresholds(attr.view(B, 1, 1, 1, V), counts)
    rthr, rrem = fi.thresholds_ref(attr, counts)
    assert thr.dtype == attr.dtype and removed.dtype == torch.int32 and thr.shape == removed.shape == (B, S)
    assert torch.equal(fi.bits(thr), fi.bits(rthr)) and torch.equal(removed, rrem)
    forced = ops.rank_thresholds_torch(attr.view(B, 1, 1, 1, V), counts)                  # the forced form: same formula
    assert torch.equal(fi.bits(forced[0]), fi.bits(thr)) and torch.equal(forced[1], removed)
    for b in range(B):
        bt, br = fi.thresholds_brute(attr[b].tolist(), counts)
        assert thr[b].tolist() == bt and removed[b].tolist() == br
        assert all(r >= n for r, n in zip(br, counts))
        assert not bool(torch.signbit(thr[b][thr[b] == 0]).any())                     # -0.0 became +0.0
    g = torch.Generator().manual_seed(3)
    vol, fill, base = torch.rand((B, V), generator=g), torch.tensor([-1.0, -2.0]), 2 + torch.rand((B, V), generator=g)
    for mode in fi.MODES:
        for bs in (None, base):
            for j0, K in fi.chunkings(B, S):
                got = ops.mask_by_rank(vol, attr, thr, fill, mode, j0, K, base=bs)
                assert torch.equal(got, fi.mask_ref(vol, attr, thr, fill, mode, j0, K, base=bs))
                assert torch.equal(ops.mask_by_rank_torch(vol, attr, thr, fill, mode, j0, K, base=bs), got)
                for k in range(K):
                    b, s = divmod(j0 + k, S + 1)
                    for e in range(V):
                        m = s > 0 and float(attr[b, e]) + 0.0 >= float(thr[b, s - 1])
                        f = float(fill[b]) if bs is None else float(bs[b, e])
                        want = (f if m else float(vol[b, e])) if mode == "deletion" else (float(vol[b, e]) if m else f)
                        assert float(got[k, e]) == want, (mode, j0, k, e)
    buf = torch.empty((4, V))
    assert ops.mask_by_rank(vol, attr, thr, fill, "deletion", 1, 4, out=buf).data_ptr() == buf.data_ptr()
    for bad in (dict(mode="both"), dict(j0=-1), dict(K=0), dict(j0=B * (S + 1)), dict(fill=torch.zeros(3)), dict(thr=thr[0]),
                dict(attr=attr[:, :-1]), dict(base=base[:, :-1]), dict(out=torch.empty((2, V)))):
        kw = dict(vol=vol, attr=attr, thr=thr, fill=fill, mode="deletion", j0=0, K=1)
        kw.update(bad)
        for fn in (ops.mask_by_rank, ops.mask_by_rank_torch):
            with pytest.raises(ValueError):
                fn(**kw)
    for bad in ([], [0, 1], [2, 1], [1, V + 1], list(range(1, 66))):
        for fn in (ops.rank_thresholds, ops.rank_thresholds_torch):
            with pytest.raises(ValueError):
                fn(attr, bad)


class _Sum(nn.Module):
    """logits[b] = (sum of x[b], sum of y[b]); a second output of ones."""

    def forward(self, x, y):
        out = torch.stack([x.flatten(1).sum(1), y.flatten(1).sum(1)], 1)
        return out, torch.ones_like(out[:, :1])


SIZE = (3, 4, 5)
V = 60


def _sum_inputs(dtype=torch.float64):
    """x[b]: the integers 1..V in a random order (the attribution is the volume itself); y: ones."""
    g = torch.Generator().manual_seed(8)
    x = torch.stack([torch.randperm(V, generator=g) + 1 for _ in range(2)]).to(dtype).view((2, 1) + SIZE)
    return x, torch.ones((2, 1) + SIZE, dtype=dtype)


@pytest.mark.parametrize("steps", (1, 4, 7, 64))
def test_sum_model_curves_are_closed_form(steps):
    """score = the masked volume's sum, values 1..V ranked by themselves, zero fill: deletion leaves the V - n_k smallest,
    sum (V - n_k)(V - n_k + 1) / 2; insertion shows the n_k largest, the rest of V(V+1)/2; the AUC is their trapezoid."""
    from transmf_ad_amd import faithfulness_curve, faithfulness_curve_torch
    x, y = _sum_inputs()
    net = _Sum().eval()
    counts = [0] + fi.counts_ref(V, steps)
    total = V * (V + 1) // 2
    for fn in (faithfulness_curve_torch, faithfulness_curve):                # on the CPU both take the torch formulas
        for mode in fi.MODES:
            fc = fn(net, x, y, attribution=x[:, 0], volume=0, steps=steps, mode=mode, score="logit", target=0, chunk=5)
            low = [(V - n) * (V - n + 1) // 2 for n in counts]
            want = low if mode == "deletion" else [total - s for s in low]
            assert fc.scores.shape == (2, steps + 1) and fc.scores.tolist() == [want, want]
            assert fc.removed.tolist() == [counts, counts] and not fc.removed.dtype.is_floating_point
            assert fc.thresholds.tolist() == [[V - n + 1 for n in counts[1:]]] * 2
            auc = (want[0] / 2 + sum(want[1:steps]) + want[steps] / 2) / steps
            assert torch.allclose(fc.auc, torch.tensor([auc, auc], dtype=torch.float64), rtol=1e-14, atol=0)
            assert torch.equal(fi.auc_ref(fc.scores), fc.auc) or torch.allclose(fi.auc_ref(fc.scores), fc.auc, rtol=1e-14, atol=0)
            assert fc.base_score.tolist() == [total, total] and fc.target.tolist() == [0, 0]
            assert (fc.steps, fc.mode, fc.volume) == (steps, mode, 0) and fc.logits.shape == (2, 2)
    # the other volume, its own attribution; the softmax score; the default arguments
    fc = faithfulness_curve_torch(net, y, x, attribution=x, volume=1, steps=4, mode="insertion", score="logit", target=1)
    assert fc.scores.tolist()[0] == [total - (V - n) * (V - n + 1) // 2 for n in [0] + fi.counts_ref(V, 4)]
    fc = faithfulness_curve_torch(net, x / total, y / (2 * V), attribution=x)
    assert fc.scores.shape == (2, 21) and fc.mode == "deletion" and fc.target.tolist() == [0, 0]
    p = torch.softmax(torch.tensor([[(V - n) * (V - n + 1) / 2 / total, 0.5] for n in [0] + fi.counts_ref(V, 20)],
                                   dtype=torch.float64), 1)[:, 0]
    assert torch.allclose(fc.scores[0], p, rtol=1e-13, atol=0)


def test_ties_negative_zero_and_baseline():
    """Ties go together (a step removes every voxel at its threshold), -0.0 ranks with +0.0, a baseline overrides fill."""
    from transmf_ad_amd import faithfulness_curve_torch
    x, y = _sum_inputs()
    net = _Sum().eval()
    attr = torch.zeros((2,) + SIZE, dtype=torch.float64)
    flat = attr.view(2, V)
    flat[:, :10] = 2.0                                                        # 10 at the top, then 20 tied zeros of both signs,
    flat[:, 10:20] = 0.0
    flat[:, 20:30] = -0.0
    flat[:, 30:] = -1.0                                                       # then 30 tied at -1
    fc = faithfulness_curve_torch(net, x, y, attribution=attr, steps=6, score="logit", target=0)
    assert fc.removed.tolist() == [[0, 10, 30, 30, 60, 60, 60]] * 2          # n_k = 10 .. 60 in tens
    assert fc.thresholds.tolist() == [[2.0, 0.0, 0.0, -1.0, -1.0, -1.0]] * 2
    assert not bool(torch.signbit(fc.thresholds[:, 1:3]).any())
    xs = x.view(2, V)
    want = torch.stack([xs.sum(1), xs[:, 10:].sum(1), xs[:, 30:].sum(1), xs[:, 30:].sum(1)] + [torch.zeros(2, dtype=x.dtype)] * 3, 1)
    assert torch.equal(fc.scores, want)
    base = torch.full_like(x, 100.0)
    fb = faithfulness_curve_torch(net, x, y, attribution=attr, steps=6, score="logit", target=0, baseline=base, fill=7.0)
    assert torch.equal(fb.scores, want + 100.0 * fb.removed.to(x.dtype)) and torch.equal(fb.removed, fc.removed)
    ff = faithfulness_curve_torch(net, x, y, attribution=attr, steps=6, score="logit", target=0, fill=torch.tensor([7.0, -1.0]))
    assert torch.equal(ff.scores, want + torch.tensor([[7.0], [-1.0]], dtype=x.dtype) * ff.removed.to(x.dtype))
    fm = faithfulness_curve_torch(net, x, y, attribution=attr, steps=6, mode="insertion", score="logit", target=0, fill="mean")
    mean = xs.mean(1, keepdim=True)
    assert torch.allclose(fm.scores, xs.sum(1, keepdim=True) - want + mean * (V - fm.removed.to(x.dtype)), rtol=1e-14, atol=0)


def test_value_errors_and_untouched_state():
    from transmf_ad_amd import faithfulness_curve, faithfulness_curve_torch
    x, y = _sum_inputs(torch.float32)
    net = _Sum()
    a = x[:, 0].clone()
    nan = a.clone()
    nan[1, 2, 3, 4] = float("nan")
    for fn in (faithfulness_curve, faithfulness_curve_torch):
        with pytest.raises(ValueError, match="eval"):
            fn(net.train(), x, y, attribution=a)
        net.eval()
        with pytest.raises(ValueError, match="NaN"):
            fn(net, x, y, attribution=nan)
        for bad in (dict(steps=0), dict(steps=65), dict(steps=4.0), dict(steps=True), dict(mode="both"), dict(mode=0),
                    dict(score="margin"), dict(volume=2), dict(volume=-1), dict(volume=0.0), dict(volume=None),
                    dict(attribution=a[:1]), dict(attribution=a[:, :2]), dict(attribution=a.view(2, V)),
                    dict(attribution=a.view((2, 1, 1) + SIZE)), dict(attribution=a.long()), dict(attribution=None),
                    dict(fill="median"), dict(fill=None), dict(fill=torch.zeros(3)), dict(fill=torch.zeros(2, 1)),
                    dict(baseline=a), dict(baseline=x[:1]), dict(baseline=3.0), dict(chunk=0), dict(target=2),
                    dict(target=torch.tensor([0, 1, 0])), dict(output=2)):
            kw = dict(attribution=a)
            kw.update(bad)
            with pytest.raises(ValueError):
                fn(net, x, y, **kw)
        with pytest.raises(ValueError):
            fn(net, x.long(), y, attribution=a)
        with pytest.raises(ValueError):
            fn(net, x.expand(2, 2, *SIZE), y, attribution=a)                     # two channels
        with pytest.raises(TypeError):
            fn(lambda p, q: p, x, y, attribution=a)
    lin = nn.Linear(V, 2)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.lin, self.bn = lin, nn.BatchNorm1d(2)

        def forward(self, p, q):
            return self.bn(self.lin((p - q).flatten(1)))

    net = Net().eval()
    keep = (x.clone(), y.clone(), a.clone(), {k: v.clone() for k, v in net.state_dict().items()}, torch.get_rng_state())
    xr, ar = x.clone().requires_grad_(True), a.clone().requires_grad_(True)
    fc = faithfulness_curve_torch(net, xr, y, attribution=ar, steps=5)
    assert torch.equal(x, keep[0]) and torch.equal(y, keep[1]) and torch.equal(a, keep[2]) and torch.equal(torch.get_rng_state(), keep[4])
    assert all(torch.equal(v, keep[3][k]) for k, v in net.state_dict().items())
    assert all(p.grad is None for p in net.parameters()) and xr.grad is None and ar.grad is None
    assert not fc.scores.requires_grad and not fc.logits.requires_grad and not fc.auc.requires_grad
    assert fc.scores.dtype == torch.float32 and bool(((fc.scores >= 0) & (fc.scores <= 1)).all())


# ---------------------------------------------------------------------------------------------------------------------
# refusals (no launch is reached: these run without a device), fixtures, header, documents
# ---------------------------------------------------------------------------------------------------------------------

def test_entries_refuse_bad_arguments():
    """Every entry returns the negative TMF_E_* the header states - before any launch, so no device is needed and the (never
    dereferenced) device pointers here are made up; counts is real host memory."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    p, q, t, r, w = (i << 20 for i in range(1, 6))
    B, Vx, S = 2, 512, 4
    cnt = lambda c: (ctypes.c_int * len(c))(*c)
    ok = cnt(fi.counts_ref(Vx, S))
    words = 2048 + S * 2048 + S * 1024
    nws = lib.tmf_rank_workspace_bytes(B, Vx, S)
    assert nws >= B * words * 4 and nws % 4 == 0 and lib.tmf_rank_workspace_bytes(1, 884736, 64) < 1 << 20
    assert lib.tmf_rank_workspace_bytes(B, Vx, 0) == 0 == lib.tmf_rank_workspace_bytes(0, Vx, S) == lib.tmf_rank_workspace_bytes(B, 0, S)
    assert lib.tmf_rank_workspace_bytes(B, Vx, 65) == 0
    rank = lambda *a: lib.tmf_rank_thresholds(*a, None)
    for args in ((None, ok, t, r, w), (p, None, t, r, w), (p, ok, None, r, w), (p, ok, t, None, w), (p, ok, t, r, None)):
        assert rank(*args, nws, B, Vx, S) == _lib.E_NULL
    assert rank(p, cnt([1]), t, r, w, nws, B, Vx, 0) == _lib.E_ARG
    assert rank(p, cnt(list(range(1, 66))), t, r, w, 1 << 30, B, Vx, 65) == _lib.E_ARG
    for bad in ([3, 2, 4, 5], [0, 1, 2, 3], [1, 2, 3, Vx + 1], [-1, 2, 3, 4], [1, 2, 4, 3]):
        assert rank(p, cnt(bad), t, r, w, nws, B, Vx, S) == _lib.E_ARG, bad
    for b, v in ((0, Vx), (-1, Vx), (B, 0), (B, -5), (B, 1 << 31), (1 << 17, Vx)):
        assert rank(p, ok, t, r, w, 1 << 40, b, v, S) == _lib.E_SHAPE, (b, v)
    assert rank(p, ok, t, r, w, nws - 1, B, Vx, S) == _lib.E_WORKSPACE
    for args in ((p + 2, ok, t, r, w), (p, ok, t + 1, r, w), (p, ok, t, r + 2, w), (p, ok, t, r, w + 3)):
        assert rank(*args, nws, B, Vx, S) == _lib.E_ALIGN
    assert b"tmf_rank_thresholds" in lib.tmf_last_error_string()
    mask = lambda *a: lib.tmf_mask_by_rank(*a, None)
    for args in ((None, p, t, p, None, q), (p, None, t, p, None, q), (p, p, None, p, None, q), (p, p, t, None, None, q),
                 (p, p, t, p, None, None)):
        assert mask(*args, B, Vx, S, 0, 0, 1) == _lib.E_NULL
    for s in (0, 65, -1):
        assert mask(p, p, t, p, None, q, B, Vx, s, 0, 0, 1) == _lib.E_ARG
    for mode in (-1, 2):
        assert mask(p, p, t, p, None, q, B, Vx, S, mode, 0, 1) == _lib.E_ARG
    for j0, K in ((0, 0), (0, -1), (-1, 1), (10, 1), (8, 3), (0, 11), ((1 << 31) - 1, 1), (0, 1 << 17)):
        assert mask(p, p, t, p, None, q, B, Vx, S, 0, j0, K) == _lib.E_ARG, (j0, K)
    assert mask(p, p, t, p, None, q, 1 << 20, 4, 64, 0, 0, (1 << 16) + 1) == _lib.E_ARG          # K > 65536
    for b, v in ((0, Vx), (-1, Vx), (B, 0), (B, 1 << 31), (1 << 30, Vx)):
        assert mask(p, p, t, p, None, q, b, v, S, 0, 0, 1) == _lib.E_SHAPE, (b, v)
    for args in ((p + 2, p, t, p, None, q), (p, p + 1, t, p, None, q), (p, p, t + 2, p, None, q), (p, p, t, p + 3, None, q),
                 (p, p, t, p, p + 2, q), (p, p, t, p, None, q + 1)):
        assert mask(*args, B, Vx, S, 0, 0, 1) == _lib.E_ALIGN
    assert b"tmf_mask_by_rank" in lib.tmf_last_error_string()


def test_committed_fixtures_keep_rule():
    """faithfulness_cnn_tiny / faithfulness_ad_tiny: every setting, mode and modality with the fp64 and fp32 curves, the fp64
    logits of every job (the curve is their target column), ranges > 0, the reference's fp32 run within 1e-3 of its fp64 run;
    the ties setting really has tied steps."""
    for name in ("cnn_tiny", "ad_tiny"):
        path = os.path.join(GOLDEN_DIR, f"faithfulness_{name}.npz")
        assert os.path.getsize(path) < 1 << 20
        z = np.load(path)
        settings = str(z["settings"]).split(",")
        assert settings == ["smooth", "ties"]
        B = z["logits"].shape[0]
        t = z["target"]
        assert z["logits"].dtype == np.float64 and np.array_equal(t, z["logits"].argmax(1))
        counts = [0] + fi.counts_ref(32 ** 3, 8)
        for s in settings:
            for mode in fi.MODES:
                for mod in ("mri", "pet"):
                    key = f"{s}.{mode}.{mod}"
                    s64, s32, rem, jobs = z[key + ".scores"], z[key + ".scores.f32"], z[key + ".removed"], z[key + ".logits"]
                    assert s64.shape == s32.shape == rem.shape == (B, 9) and s64.dtype == np.float64 and s32.dtype == np.float32
                    assert jobs.shape == (B, 9, 2) and rem.dtype == np.int32
                    assert np.array_equal(s64, jobs[np.arange(B), :, t])
                    assert (rem[:, 0] == 0).all() and (rem[:, -1] == 32 ** 3).all() and (rem >= np.array(counts)).all()
                    assert (np.diff(rem, axis=1) >= 0).all()
                    if s == "smooth":
                        assert (rem == np.array(counts)).all()
                    else:
                        assert (np.diff(rem, axis=1) == 0).any() and (rem[:, 1:-1] > np.array(counts[1:-1])).any()
                    if mode == "deletion":
                        assert np.allclose(jobs[:, 0], z["logits"], rtol=0, atol=1e-12)      # job 0 of a deletion is the volume itself
                    span = s64.max(1) - s64.min(1)
                    assert (span > 0).all() and np.array_equal(span, z["range." + key])
                    dist = (np.abs(s32.astype(np.float64) - s64).max(1) / span).max()
                    assert dist == float(z["dist." + key]) and dist <= 1e-3, (name, key, dist)


def test_new_names_in_header_library_binding_and_documents():
    from transmf_ad_amd import _lib, build, ops
    import transmf_ad_amd as T
    with open(os.path.join(ROOT, "include", "tmf_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        rows = [l for l in f if l.startswith("| **`tmf_rank_thresholds`**") or l.startswith("| **`tmf_mask_by_rank`**")]
    assert len(rows) == 2
    stated = {name: int(n) for row in rows for name, n in re.findall(r"`(tmf_(?:rank|mask)\w*)`[^|`]*?\((\d+) arguments?\)", row)}
    assert stated == ENTRIES
    lib = _lib.load()
    for name, nargs in ENTRIES.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
        assert getattr(lib, name).argtypes == _lib.PROTOTYPES[name][1]
    assert _lib.PROTOTYPES["tmf_rank_workspace_bytes"][0] is ctypes.c_size_t
    assert (_lib.RANK_MAX_STEPS, _lib.RANK_DELETION, _lib.RANK_INSERTION) == (64, 0, 1)
    assert "faithfulness.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "faithfulness.hip"))
    for fn in ("rank_counts", "rank_thresholds", "mask_by_rank", "faithfulness_ok"):
        assert callable(getattr(ops, fn)), fn
    assert "faithfulness_curve" in T.__all__ and "faithfulness_curve_torch" in T.__all__
    assert callable(T.faithfulness_curve) and callable(T.faithfulness_curve_torch)
    for doc, words in (("DESIGN.md", ("3.30", "tmf_rank_thresholds", "tmf_mask_by_rank", "faithfulness_mi355x.txt")),
                       ("README.md", ("faithfulness_curve", "tmf_rank_thresholds")),
                       (os.path.join("profiles", "README.md"), ("faithfulness_mi355x.txt", "faithfulness_time.py"))):
        with open(os.path.join(ROOT, doc)) as f:
            text = f.read()
        assert all(w in text for w in words), doc
    assert os.path.exists(os.path.join(ROOT, "profiles", "faithfulness_mi355x.txt"))
    assert os.path.exists(os.path.join(ROOT, "tools", "faithfulness_time.py"))
