"""token_ops.hip (LayerNorm, mask_mul, token pool), the Philox keep-mask kernel and the dense heads of heads.hip against the
references of tests/_token_inputs.py.  Everything but the heads is called on its own, through _lib.call with raw pointers and
nothing of ops.py in between; the heads go through ops.HeadsAD / ops.HeadsCNN the way the models call them.

1. token pool: integers (ties everywhere, planted ties across and inside the four token lanes), NaN / inf / signed zeros;
2. LayerNorm: rows of |mean| / sd 1000, 0, 30 and constant rows, judged per row against the measured distance of the fp32
   restatement (LN_DISTANCE) times MARGIN; the dbeta partials exactly; the masked form bit for bit;
3. mask_mul bit for bit;
4. the keep-masks as a known answer of a host Philox model;
5. the heads against the stock modules in fp64 at the model's widths, a narrow hand-built geometry and the CNN-only models.

Every output of a direct call lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs must be unchanged
and every output fully written."""
import ctypes as C
import copy
import functools

import numpy as np
import pytest
import torch
from torch import nn

import _token_inputs as ti
from test_gpu_bn_reduce import Arena, _call, _query, _st

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, I32 = torch.float32, torch.int32


def _same(a, b):
    """NaN-aware equality of two float tensors (NaN in the same places, equal elsewhere; +0 = -0 as everywhere)."""
    return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))


# ---------------------------------------------------------------------------------------------------------------------
# 1. token pool
# ---------------------------------------------------------------------------------------------------------------------
def _pool_fwd(mri, pet, may_nan=()):
    B, N, dim = mri.shape
    a = Arena(dict(mri=mri, pet=pet), dict(cls=((B, 4 * dim), F32), argmax=((B, 2, dim), I32)))
    _call("tmf_token_pool_fwd", a.ptr("mri"), a.ptr("pet"), a.ptr("cls"), a.ptr("argmax"), B, N, dim, _st())
    return a.fetch(may_nan=may_nan)


@pytest.mark.parametrize("case", ti.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_token_pool_forward_ties(case):
    """Integer tokens in [-3, 3] with the planted maxima of POOL_PLANTS: argmax is ATen's (the first of equal maxima, whichever
    token lane holds it), the maxima are bit-equal, the mean is bit-equal where N is a power of two (sum and quotient exact) and
    within one fp32 ulp of the fp64 quotient otherwise (the sum is an exact integer, the division rounds once)."""
    B, N, dim = case
    mri, pet = ti.pool_inputs(B, N, dim)
    ref, arg = ti.pool_ref(mri, pet)
    res = _pool_fwd(mri, pet)
    assert torch.equal(res["argmax"], arg)
    assert torch.equal(res["cls"][:, 2 * dim:], ref[:, 2 * dim:].float())
    mean, want = res["cls"][:, :2 * dim], ref[:, :2 * dim]
    if N & (N - 1) == 0:
        assert torch.equal(mean, want.float())
    else:
        err, tol = (mean.double() - want).abs(), ti.ulp_at(want, F32)
        print(f"{case} mean: worst err / ulp {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= tol).all())


def test_token_pool_forward_nan_inf_and_signed_zero():
    """One column per special of POOL_SPECIALS (N = 9): index and value as ATen's - the LAST NaN wins across and inside token
    lanes, a NaN is not displaced by larger values behind it, the first +inf, index 0 for a column of -inf and for zeros of
    either sign - and the mean column is NaN or +-inf as fp64 gives."""
    mri, pet = ti.pool_special_inputs()
    dim = ti.POOL_SPECIAL_DIM
    ref, arg = ti.pool_ref(mri, pet)
    res = _pool_fwd(mri, pet, may_nan=("cls",))
    assert torch.equal(res["argmax"], arg), (res["argmax"][0, 0, :7].tolist(), arg[0, 0, :7].tolist())
    assert _same(res["cls"][:, 2 * dim:], ref[:, 2 * dim:].float())
    mean, want = res["cls"][:, :2 * dim].double(), ref[:, :2 * dim]
    assert torch.equal(torch.isnan(mean), torch.isnan(want))
    fin = torch.isfinite(want)
    assert torch.equal(mean[~fin & ~torch.isnan(want)], want[~fin & ~torch.isnan(want)])
    assert bool(((mean[fin] - want[fin]).abs() <= ti.ulp_at(want[fin], F32)).all())


@pytest.mark.parametrize("case", ti.POOL_BWD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_token_pool_backward_exact(case):
    """tmf_token_pool_bwd on dyadic dcls with N a power of two: every element equals gavg / N + (n == am) gmax bit for bit, with
    the forward kernel's own argmax and with a hand-made one that routes to token 0 and to token N - 1."""
    B, N, dim, source = case
    mri, pet = ti.pool_inputs(B, N, dim)
    dcls, ends = ti.pool_bwd_inputs(B, N, dim)
    outs = dict(dmri=((B, N, dim), F32), dpet=((B, N, dim), F32))
    if source == "forward":
        outs = dict(cls=((B, 4 * dim), F32), argmax=((B, 2, dim), I32), **outs)
        a = Arena(dict(mri=mri, pet=pet, dcls=dcls), outs)
        _call("tmf_token_pool_fwd", a.ptr("mri"), a.ptr("pet"), a.ptr("cls"), a.ptr("argmax"), B, N, dim, _st())
        am = ti.pool_ref(mri, pet)[1]
    else:
        a = Arena(dict(dcls=dcls, argmax=ends), outs)
        am = ends
    _call("tmf_token_pool_bwd", a.ptr("dcls"), a.ptr("argmax"), a.ptr("dmri"), a.ptr("dpet"), B, N, dim, _st())
    res = a.fetch()
    if source == "forward":
        assert torch.equal(res["argmax"], am)
    dm, dp = ti.pool_bwd_ref(dcls, am, N)
    assert torch.equal(res["dmri"], dm.float()) and torch.equal(res["dpet"], dp.float())


# ---------------------------------------------------------------------------------------------------------------------
# 2. LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ln_case(shape):
    inp = ti.ln_inputs(*shape)
    return inp, ti.ln_quantities(inp), ti.ln_saved(inp)


@pytest.mark.parametrize("shape", ti.LN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layernorm_against_fp64(shape):
    """tmf_layernorm_fwd without and with `residual`, tmf_layernorm_bwd and tmf_layernorm_bwd_masked on one set of inputs.
    y, y + residual, mean, rstd and dx per ROW: |kernel - fp64| <= MARGIN x LN_DISTANCE[shape][quantity, class] x max |fp64| of
    the row; sum_blocks partial[:, 0] per column on the scale sum |terms|.  Exactly: sum_blocks partial[:, 1] = sum_rows dy
    (dyadic: a row skipped or counted twice cannot hide); constant rows give mean = c, y = beta bit for bit and rstd =
    1 / sqrt(eps) to 2 ulp (a correctly rounded square root, then a correctly rounded quotient: 0.5 ulp each, the first carried
    through the quotient once more); both forward calls save the same statistics; the masked backward's dx and partials are
    bit-identical to the plain call's and dx_masked is the fp32 product dx x mask.  The partial buffer has exactly
    tmf_layernorm_bwd_blocks(rows, dim) rows."""
    rows, dim = shape
    inp, r64, (mean_in, rstd_in) = _ln_case(shape)
    nblk = _query("tmf_layernorm_bwd_blocks", rows, dim)
    ins = dict(inp, mean_in=mean_in, rstd_in=rstd_in)
    full, row = ((rows, dim), F32), ((rows,), F32)
    a = Arena(ins, dict(y=full, mean=row, rstd=row, y_res=full, mean2=row, rstd2=row, dx=full, partial=((nblk, 2, dim), F32),
                        dx2=full, dxm=full, partial2=((nblk, 2, dim), F32)))
    p = a.ptr
    eps = ti.LN_EPS
    _call("tmf_layernorm_fwd", p("x"), p("gamma"), p("beta"), None, p("y"), p("mean"), p("rstd"), rows, dim, eps, _st())
    _call("tmf_layernorm_fwd", p("x"), p("gamma"), p("beta"), p("residual"), p("y_res"), p("mean2"), p("rstd2"), rows, dim, eps, _st())
    _call("tmf_layernorm_bwd", p("x"), p("gamma"), p("mean_in"), p("rstd_in"), p("dy"), p("dx"), p("partial"), rows, dim, _st())
    _call("tmf_layernorm_bwd_masked", p("x"), p("gamma"), p("mean_in"), p("rstd_in"), p("dy"), p("dx2"), p("partial2"), rows, dim,
          p("mask"), p("dxm"), _st())
    res = a.fetch()
    # exact statements
    assert torch.equal(res["mean2"], res["mean"]) and torch.equal(res["rstd2"], res["rstd"])
    assert torch.equal(res["partial"][:, 1].double().sum(0), inp["dy"].double().sum(0)), "dbeta partials: a row skipped or counted twice"
    assert torch.equal(res["dx2"], res["dx"]) and torch.equal(res["partial2"], res["partial"])
    assert torch.equal(res["dxm"], res["dx"] * inp["mask"])
    const = ti.ln_class(rows) == 3
    if bool(const.any()):
        k = int(const.sum())
        assert torch.equal(res["mean"][const], inp["x"][const][:, 0])
        assert torch.equal(res["y"][const], inp["beta"].expand(k, dim))
        assert torch.equal(res["y_res"][const], inp["beta"].expand(k, dim) + inp["residual"][const])
        want = r64["rstd"][const]
        assert bool(((res["rstd"][const].double() - want).abs() <= 2 * ti.ulp_at(want, F32)).all())
    # per row / per column against the restatement distances
    got = dict(res, dgamma=res["partial"][:, 0].double().sum(0))
    dist, rec = ti.ln_distances(got, r64, rows), ti.LN_DISTANCE[shape]
    bad = []
    for q in ti.LN_QUANTITIES:
        worst = max((dist[key] / (ti.MARGIN * ti.floor_distance(rec[key])), key[1]) for key in dist if key[0] == q)
        print(f"{shape} {q}: worst err / tol {worst[0]:.3f} (class {worst[1]})")
        if worst[0] > 1.0:
            bad.append((q, worst))
    assert not bad, f"{shape}: {bad} beyond {ti.MARGIN} restatement distances"


def test_layernorm_backward_refuses_beyond_its_limit_without_a_launch():
    """dim 513 (scalar path) and 2052 (vector path) are more than LN_MAXV groups per lane: TMF_E_SHAPE with the limit in the
    text, and no byte of the arena changes."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    for dim, limit in ((513, 512), (2052, 2048)):
        t = torch.ones((3, dim))
        a = Arena(dict(x=t, gamma=t[0], mean=t[:, 0], rstd=t[:, 0], dy=t, dx=t, partial=torch.ones((1, 2, dim)), mask=t, dxm=t), {})
        p = a.ptr
        assert lib.tmf_layernorm_bwd(p("x"), p("gamma"), p("mean"), p("rstd"), p("dy"), p("dx"), p("partial"), 3, dim, _st()) == -2
        assert f"dim={dim} exceeds {limit}" in lib.tmf_last_error_string().decode()
        assert lib.tmf_layernorm_bwd_masked(p("x"), p("gamma"), p("mean"), p("rstd"), p("dy"), p("dx"), p("partial"), 3, dim,
                                            p("mask"), p("dxm"), _st()) == -2
        assert f"dim={dim} exceeds {limit}" in lib.tmf_last_error_string().decode()
        a.fetch()


# ---------------------------------------------------------------------------------------------------------------------
# 3. mask_mul
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ti.MASK_MUL_N)
def test_mask_mul_bit_equal(n):
    """y = x * mask on either side of the 4-wide step and of the 1024-element workgroup: the fp32 product, nothing behind n."""
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    mask = torch.tensor([0.0, 2.0, 1.0 / 0.7])[torch.randint(0, 3, (n,), generator=g)]
    a = Arena(dict(x=x, mask=mask), dict(y=((n,), F32)))
    _call("tmf_mask_mul", a.ptr("x"), a.ptr("mask"), a.ptr("y"), n, _st())
    assert torch.equal(a.fetch()["y"], x * mask)


# ---------------------------------------------------------------------------------------------------------------------
# 4. keep-masks
# ---------------------------------------------------------------------------------------------------------------------
def _keep_masks(numels, keeps, seed, offset):
    n = len(numels)
    a = Arena({}, {f"s{i}": ((k,), F32) for i, k in enumerate(numels)})
    _call("tmf_dropout_keep_masks", n, (C.c_void_p * n)(*[a.ptr(f"s{i}") for i in range(n)]), (C.c_long * n)(*numels),
          (C.c_float * n)(*keeps), seed, offset, _st())
    res = a.fetch()                                             # the 16-byte padding behind a segment is outside its slot
    return [res[f"s{i}"].numpy() for i in range(n)]


@pytest.mark.parametrize("seed,offset", ti.MASK_SEED_OFFSET, ids=["low", "seed-high-offset-2^32", "seed-bit63-offset-2^42"])
def test_keep_masks_equal_the_philox_model(seed, offset):
    """tmf_dropout_keep_masks is a pure function of (seed, offset, segment, element): bit-equal to the host model of
    _token_inputs.keep_masks_model - three segments of 1, 5 and 1027 elements (keep 0.5, 0.7, 1: the last all ones), then
    MASK_SEGMENTS segments of 3 elements; the same call again gives the same bits."""
    from transmf_ad_amd import _lib
    numels, keeps = [1, 5, 1027], [0.5, 0.7, 1.0]
    got = _keep_masks(numels, keeps, seed, offset)
    want = ti.keep_masks_model(numels, keeps, seed, offset)
    for s, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"segment {s}: {int((g != w).sum())} of {g.size} elements differ"
    assert bool((got[2] == 1.0).all())
    again = _keep_masks(numels, keeps, seed, offset)
    assert all(np.array_equal(g, h) for g, h in zip(got, again))
    n = _lib.MASK_SEGMENTS
    numels, keeps = [3] * n, [0.25 + 0.03 * i for i in range(n)]
    got = _keep_masks(numels, keeps, seed, offset)
    want = ti.keep_masks_model(numels, keeps, seed, offset)
    for s, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), f"segment {s} of {n}"


def test_keep_masks_through_ops_follow_the_device_generator():
    """ops.dropout_keep_masks after torch.manual_seed(s): the masks are the model's at (s, the device generator's offset read
    before the call), and that offset advances by 4."""
    from transmf_ad_amd import ops
    seed = 0x5EED00000123
    torch.manual_seed(seed)
    torch.rand(3, device=DEV)                                    # moves the stream offset off zero
    gen = torch.cuda.default_generators[0]
    off = gen.get_offset()
    assert gen.initial_seed() == seed and off > 0
    drops, shapes = [nn.Dropout(0.5), nn.Dropout(0.3)], [(3, 5), (1027,)]
    masks = ops.dropout_keep_masks(list(zip(drops, shapes)), torch.device(DEV))
    torch.cuda.synchronize()
    assert gen.get_offset() == off + 4
    want = ti.keep_masks_model([15, 1027], [1.0 - 0.5, 1.0 - 0.3], seed, off)
    for m, w, shape in zip(masks, want, shapes):
        assert tuple(m.shape) == shape and np.array_equal(m.cpu().numpy().reshape(-1), w)


# ---------------------------------------------------------------------------------------------------------------------
# 5. dense heads
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model_ad(dim):
    import transmf_ad_amd as T
    return T.model_ad(dim, 1, 2, dim // 2, 2 * dim, 0.).to(DEV)


@functools.lru_cache(maxsize=None)
def _heads_ref(name):
    case = next(c for c in ti.HEADS_CASES if c["name"] == name)
    return ti.heads_run(case, torch.float64)[0]


def _heads_on_device(case):
    """The case's stock modules (fp32) moved to the device and run through the one-launch heads -> dict as ti.heads_run."""
    from transmf_ad_amd import mymodel
    kind, train = case["kind"], case["train"]
    mods = copy.deepcopy(ti.make_heads(case)).to(DEV).train(train)
    inp = ti.heads_inputs(case)
    mri = inp["mri"].to(DEV).requires_grad_(True)
    pet = inp["pet"].to(DEV).requires_grad_(True) if inp["pet"] is not None else None
    cls = None
    if kind == "ad":
        net = _model_ad(case["dim"])
        net.fc_cls, net.D = mods["fc"], mods["D"]
        net.train(train)
        mods.train(train)
        cls = inp["cls"].to(DEV).requires_grad_(True)
        assert net._heads_one_call_ok(mri), "the heads of this geometry must take the one-launch path"
        outs = list(net._heads(cls, mri, pet))
        assert type(outs[0].grad_fn).__name__.startswith("HeadsAD")
    else:
        D = mods["D"] if kind == "cnn_ad" else None
        assert mymodel._cnn_heads_one_call_ok(mods, mods["fc"], D, mri, 1 if pet is None else 2)
        out = mymodel._cnn_heads(mods, mods["fc"], D, mri, pet)
        outs = list(out) if isinstance(out, tuple) else [out]
        assert type(outs[0].grad_fn).__name__.startswith("HeadsCNN")
    none = ti.heads_none_index(case)
    keep = [i for i in range(len(outs)) if i != none]
    torch.autograd.backward([outs[i] for i in keep], [inp["go"][i].to(DEV) for i in keep])
    torch.cuda.synchronize()
    res = {k: o.detach() for k, o in zip(("logits", "d_mri", "d_pet"), outs)}

    def grad(t):
        return t.grad if t.grad is not None else torch.zeros_like(t)
    if cls is not None:
        res["d_cls"] = grad(cls)
    res["d_mri_tok"] = grad(mri)
    if pet is not None:
        res["d_pet_tok"] = grad(pet)
    for k, p in mods.named_parameters():
        res["grad/" + k] = grad(p)
    for k, b in mods.named_buffers():
        if not k.endswith(".mask"):
            res["buf/" + k] = b.detach()
    return {k: v.cpu() for k, v in res.items()}


@pytest.mark.parametrize("case", ti.HEADS_CASES, ids=lambda c: c["name"])
def test_heads_against_fp64_stock_modules(case):
    """ops.HeadsAD / ops.HeadsCNN against the stock modules in fp64 on the CPU: the three outputs, d cls, d mri_tok, d pet_tok,
    every head parameter's gradient, the BatchNorm1d running buffers (D's updated twice, MRI call first) and
    num_batches_tracked.  |kernel - fp64| <= MARGIN x HEADS_DISTANCE[case][tensor] x max |fp64| over the whole tensor, no element
    left out; a bias in front of a train-mode BatchNorm1d on the scale of its layer's weight gradient.  Train-mode cases carry
    the planted features of _token_inputs.make_heads (constant hidden features with an exact-zero and a positive ReLU input, a
    keep-mask column of zeros) and leave one of the three output gradients out.
    One tensor carries a margin of 12 instead of 4 (_token_inputs.HEADS_MARGIN): d_mri_tok of ad-B2-N1-train, the cancellation
    residue behind a train-mode BatchNorm1d over two rows, measured err / (D x scale) = 7.58."""
    ref = _heads_ref(case["name"])
    got = _heads_on_device(case)
    rec = ti.HEADS_DISTANCE[case["name"]]
    assert set(got) == set(ref)
    bad, worst = [], {}
    for k, want in ref.items():
        assert got[k].shape == want.shape, k
        if not want.dtype.is_floating_point:
            assert torch.equal(got[k], want), k
            continue
        assert bool(torch.isfinite(got[k]).all()), k
        err = float((got[k].double() - want.double()).abs().max())
        tol = ti.heads_margin(case, k) * ti.floor_distance(rec[k]) * ti.heads_scale(k, ref, case)
        ratio = err / tol if tol > 0 else (0.0 if err == 0 else float("inf"))
        group = k.split("/")[0] if "/" in k else k
        worst[group] = max(worst.get(group, (0.0, k)), (ratio, k))
        if ratio > 1.0:
            bad.append((k, round(ratio, 3)))
    for group, (ratio, k) in worst.items():
        print(f"{case['name']} {group}: worst err / tol {ratio:.3f} ({k})")
    assert not bad, f"{case['name']}: {bad} beyond their margin of restatement distances"
