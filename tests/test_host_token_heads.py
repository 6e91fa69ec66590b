"""CPU-only checks of what tests/test_gpu_token_heads.py stands on: the Philox model against the published vectors, the pool
reference against ATen's documented tie / NaN rules restated by hand, the LayerNorm references against F.layer_norm and
autograd in fp64, the properties the generators promise (conditioning classes, exact constant rows, exact column sums, the
planted head features, the ReLU margin), every recorded restatement distance, and the time each reference takes."""
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _token_inputs as ti


# ---------------------------------------------------------------------------------------------------------------------
# keep-masks
# ---------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in ti.PHILOX_VECTORS:
        assert tuple(int(v) for v in ti.philox4x32([ctr], key)[0]) == want
    # vectorised = one at a time; a dropped round or another counter word changes every output
    ctrs = [(i, 7 * i, 3, 1 << 31) for i in range(5)]
    many = ti.philox4x32(ctrs, (5, 6))
    for i, c in enumerate(ctrs):
        assert np.array_equal(many[i], ti.philox4x32([c], (5, 6))[0])
    assert not np.array_equal(ti.philox4x32([ti.PHILOX_VECTORS[2][0]], ti.PHILOX_VECTORS[2][1], rounds=9)[0],
                              np.array(ti.PHILOX_VECTORS[2][2], dtype=np.uint64))


def test_keep_mask_model_properties():
    """Values are 0 or float32(1) / float32(keep), keep 1 keeps everything, the rate is right to 4 sigma, the streams of two
    segments, two offsets and two seeds (high halves included) differ, and a segment does not depend on its neighbours' sizes
    (the counter holds the quad index inside the segment)."""
    n = 1 << 14
    a = ti.keep_masks_model([n, n, 5], [0.5, 0.7, 1.0], 0x1234, 8)
    assert bool((a[2] == 1.0).all())
    for m, keep in zip(a[:2], (0.5, 0.7)):
        inv = np.float32(1.0) / np.float32(keep)
        assert bool(((m == 0) | (m == inv)).all())
        assert abs(float((m != 0).mean()) - keep) <= 4 * math.sqrt(keep * (1 - keep) / n)
    same_keep = ti.keep_masks_model([n, n], [0.5, 0.5], 0x1234, 8)
    assert not np.array_equal(same_keep[0], same_keep[1])
    assert np.array_equal(ti.keep_masks_model([7, n], [0.3, 0.5], 0x1234, 8)[1], same_keep[1])
    for seed, off in ((0x1234, 8 + (1 << 32)), (0x1234 + (1 << 32), 8), (0x1235, 8), (0x1234, 12)):
        assert not np.array_equal(ti.keep_masks_model([n], [0.5], seed, off)[0], same_keep[0])


# ---------------------------------------------------------------------------------------------------------------------
# token pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_by_hand(x):
    """One column at a time, as the kernel's contract words it: a later value replaces the held one when it is larger or NaN."""
    B, N, dim = x.shape
    val, arg = torch.empty((B, dim), dtype=torch.float64), torch.empty((B, dim), dtype=torch.int32)
    for b in range(B):
        for c in range(dim):
            mx, am = -math.inf, 0
            for n in range(N):
                v = float(x[b, n, c])
                if v > mx or v != v:
                    mx, am = v, n
            val[b, c], arg[b, c] = mx, am
    return val, arg


def _same(a, b):
    """NaN-aware equality (NaN in the same places, equal elsewhere)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


def test_pool_reference_is_aten_with_first_tie_and_last_nan():
    mri, pet = ti.pool_special_inputs()
    cls, arg = ti.pool_ref(mri, pet)
    dim = ti.POOL_SPECIAL_DIM
    assert arg[0, 0, :7].tolist() == [4, 3, 5, 0, 2, 0, 0]
    mx = cls[0, 2 * dim:3 * dim]
    assert bool(torch.isnan(mx[:4]).all()) and mx[4] == math.inf and mx[5] == -math.inf and mx[6] == 0
    mean = cls[0, :dim]
    assert bool(torch.isnan(mean[:4]).all()) and mean[4] == math.inf and mean[5] == -math.inf and mean[6] == 0
    assert not bool(torch.isnan(mean[7:]).any()) and not bool(torch.isnan(mx[7:]).any())
    for x, m in ((mri, 0), (pet, 1)):
        val, am = _pool_by_hand(x)
        assert _same(val, cls[:, (2 + m) * dim:(3 + m) * dim]) and torch.equal(am, arg[:, m])
    for B, N, dim in ti.POOL_CASES:
        mri, pet = ti.pool_inputs(B, N, dim)
        cls, arg = ti.pool_ref(mri, pet)
        for x, m in ((mri, 0), (pet, 1)):
            val, am = _pool_by_hand(x)
            assert torch.equal(val, cls[:, (2 + m) * dim:(3 + m) * dim]) and torch.equal(am, arg[:, m])
            for c, toks in ti.POOL_PLANTS.items():
                if max(toks) < N:
                    assert bool((arg[:, m, c] == toks[0]).all()) and bool((cls[:, (2 + m) * dim + c] == 5).all())
            if N > 1:                                            # seven values: a good share of the columns hold their maximum twice
                assert float(((x == x.max(1, keepdim=True).values).sum(1) > 1).float().mean()) > 0.08
    assert {c[0] for c in ti.POOL_CASES} == {1, 3} and {c[1] for c in ti.POOL_CASES} == {1, 2, 3, 4, 5, 7, 8, 9, 13}
    assert {c[2] for c in ti.POOL_CASES} == {20, 64, 65, 130}


@pytest.mark.parametrize("case", ti.POOL_BWD_CASES, ids=str)
def test_pool_backward_reference_is_autograd_and_exact(case):
    B, N, dim, _src = case
    assert N & (N - 1) == 0
    mri, pet = ti.pool_inputs(B, N, dim)
    dcls, ends = ti.pool_bwd_inputs(B, N, dim)
    assert ends.min() == 0 and ends.max() == N - 1
    m, p = mri.double().requires_grad_(True), pet.double().requires_grad_(True)
    out = torch.cat([m.mean(1), p.mean(1), F.adaptive_max_pool1d(m.transpose(1, 2), 1)[..., 0],
                     F.adaptive_max_pool1d(p.transpose(1, 2), 1)[..., 0]], 1)
    out.backward(dcls.double())
    dm, dp = ti.pool_bwd_ref(dcls, ti.pool_ref(mri, pet)[1], N)
    assert torch.equal(dm, m.grad) and torch.equal(dp, p.grad)
    assert torch.equal(dm.float().double(), dm)                  # dyadic: an fp32 number, whatever the order of the two terms


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ti.LN_SHAPES[:8], ids=str)
def test_layernorm_references_agree_with_torch_in_fp64(shape):
    rows, dim = shape
    inp = ti.ln_inputs(rows, dim)
    eps = ti.f32(ti.LN_EPS)
    x = inp["x"].double().requires_grad_(True)
    g, b = inp["gamma"].double().requires_grad_(True), inp["beta"].double().requires_grad_(True)
    y = F.layer_norm(x, (dim,), g, b, eps)
    y.backward(inp["dy"].double())
    r = ti.ln_fwd_ref(inp)

    def close(u, v):
        return float((u - v).abs().max()) <= 1e-11 * max(1.0, float(v.abs().max()))
    assert close(r["y"], y.detach()) and close(r["y_res"], y.detach() + inp["residual"].double())
    assert close(r["mean"], x.detach().mean(1)) and close(r["rstd"], 1 / torch.sqrt(x.detach().var(1, unbiased=False) + eps))
    bw = ti.ln_bwd_ref(inp, r["mean"], r["rstd"])                # on the UNROUNDED statistics: autograd's own
    assert close(bw["dx"], x.grad) and close(bw["dgamma"], g.grad) and torch.equal(bw["dbeta"], b.grad)


@pytest.mark.parametrize("shape", ti.LN_SHAPES, ids=str)
def test_layernorm_inputs_and_recorded_distances(shape):
    """The rows have the conditioning asked for, constant rows are exact (mean = c, variance 0, y = beta bit for bit in fp32
    under either order of additions), gamma has both signs and one zero, the column sums of dy are exact in fp32, the mask holds
    its three values - and the recorded restatement distances have not drifted by more than a factor of 2."""
    rows, dim = shape
    inp = ti.ln_inputs(rows, dim)
    x, cls = inp["x"].double(), ti.ln_class(rows)
    if dim >= 30:
        ratio = x.mean(1).abs() / x.std(1)
        for c, want in ((0, 1000.0), (1, 0.0), (2, 30.0)):
            if bool((cls == c).any()):
                got = ratio[cls == c]                           # the sample sd of 30 .. 2048 values scatters around the row's sd
                assert bool(((got > want / 2) & (got < want * 2)).all() if want else (got < 1.0).all()), (c, got)
    const = cls == 3
    if bool(const.any()):
        assert bool((x[const] == x[const][:, :1]).all())
        for order in ("tree", "chain"):
            r = ti.ln_fwd_ref(inp, torch.float32, order)
            assert torch.equal(r["mean"][const].double(), x[const][:, 0])
            assert torch.equal(r["y"][const], inp["beta"].expand(int(const.sum()), dim))
        r = ti.ln_fwd_ref(inp)
        assert bool((r["rstd"][const] == 1.0 / math.sqrt(ti.f32(ti.LN_EPS))).all())
    g = inp["gamma"]
    assert int((g == 0).sum()) == 1 and bool((g > 0).any()) and (dim < 2 or bool((g < 0).any()))
    k = inp["dy"].double() * 64
    assert torch.equal(k, k.round()) and float(k.abs().sum(0).max()) < 2 ** 24
    assert set(inp["mask"].unique().tolist()) <= {0.0, 2.0, float(np.float32(1.0 / 0.7))}
    t0 = time.perf_counter()
    ti.ln_quantities(inp)
    t_ref = time.perf_counter() - t0
    now, rec = ti.ln_restatement_distance(rows, dim), ti.LN_DISTANCE[shape]
    print(f"LayerNorm {shape}: fp64 reference {t_ref * 1e3:.1f} ms")
    assert t_ref < 2.0
    assert set(now) == set(rec)
    for key in rec:
        a, b = ti.floor_distance(rec[key]), ti.floor_distance(now[key])
        assert a / 2 <= b <= a * 2, f"{shape} {key}: recorded {rec[key]:.3e}, measured {now[key]:.3e}"


def test_layernorm_backward_limit_is_refused_before_any_launch():
    """dim 513 (scalar path: 64 x 8) and dim 2052 (vector path: 64 x 4 x 8) -> TMF_E_SHAPE with the limit in the text; no launch
    happens, so the pointers only have to be non-NULL."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    p = 4096
    for dim, limit in ((513, 512), (2052, 2048)):
        assert lib.tmf_layernorm_bwd(p, p, p, p, p, p, p, 3, dim, None) == -2
        assert f"dim={dim} exceeds {limit}" in lib.tmf_last_error_string().decode()
        assert lib.tmf_layernorm_bwd_masked(p, p, p, p, p, p, p, 3, dim, p, p, None) == -2
        assert f"dim={dim} exceeds {limit}" in lib.tmf_last_error_string().decode()


# ---------------------------------------------------------------------------------------------------------------------
# dense heads
# ---------------------------------------------------------------------------------------------------------------------
def test_heads_cases_cover_the_issue():
    ad = [c for c in ti.HEADS_CASES if c["kind"] == "ad" and c["widths"] == ti.AD_WIDTHS]
    assert {(c["B"], c["train"]) for c in ad} == {(b, t) for b in (2, 3, 16, 17) for t in (True, False)} | {(1, False)}
    assert {c["N"] for c in ad} == {1, 3, 13, 16, 17, 29} and {c["dim"] for c in ad} == {32}
    narrow = [c for c in ti.HEADS_CASES if c["widths"] == ti.NARROW]
    assert {(c["B"], c["N"], c["dim"], c["train"]) for c in narrow} == {(3, 5, 8, True), (17, 5, 8, True)}
    assert len({c["name"] for c in ti.HEADS_CASES}) == len(ti.HEADS_CASES) == len(ti.HEADS_DISTANCE)
    nones = [ti.heads_none_index(c) for c in ti.HEADS_CASES if c["train"] and c["kind"] != "single"]
    assert set(nones) == {0, 1, 2}


@pytest.mark.parametrize("case", ti.HEADS_CASES, ids=lambda c: c["name"])
def test_heads_case_margin_plants_and_recorded_distances(case):
    """No fp64 ReLU input lies within RELU_MARGIN x max |pre-activation| of zero other than the planted exact zeros (a ReLU
    that flips between fp32 and fp64 would be judged as an error of the kernel); the planted features are what they are said
    to be; the recorded restatement distances have not drifted by more than a factor of 2; the reference is quick."""
    assert ti.heads_relu_margin(case) >= ti.RELU_MARGIN
    t0 = time.perf_counter()
    r64, relu_in = ti.heads_run(case, torch.float64)
    t_ref = time.perf_counter() - t0
    print(f"heads {case['name']}: fp64 reference {t_ref * 1e3:.1f} ms")
    assert t_ref < 2.0
    mods = ti.make_heads(case)
    B = case["B"]
    if case["train"]:
        j0, j1 = ti.ZERO_ROW_BETA0, ti.ZERO_ROW_BETA_POS
        # the ReLU inputs in call order: D (MRI call), D (PET call), the hidden layer of fc [, fc_cls.5's]; single: fc's alone
        for a in relu_in[:1 if case["kind"] == "single" else 3]:
            assert bool((a[:, j0] == 0).all()) and bool((a[:, j1] == ti.PLANT_BETA).all())
        assert sum(int((a == 0).sum()) for a in relu_in) == B * (1 if case["kind"] == "single" else 3)
        if case["kind"] == "ad":
            assert not bool(mods["fc"][3].mask[:, ti.ZERO_MASK_COLUMN].any()) and not bool(mods["fc"][7].mask[:, ti.ZERO_MASK_COLUMN].any())
            assert bool(mods["fc"][3].mask.any(0).sum() >= mods["fc"][3].mask.shape[1] // 2)
    now, rec = ti.heads_restatement_distance(case), ti.HEADS_DISTANCE[case["name"]]
    assert set(now) == set(rec)
    for key in rec:
        a, b = ti.floor_distance(rec[key]), ti.floor_distance(now[key])
        assert a / 2 <= b <= a * 2, f"{case['name']} {key}: recorded {rec[key]:.3e}, measured {now[key]:.3e}"
