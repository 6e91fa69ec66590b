"""CPU-only checks of what tests/test_gpu_bn_reduce.py stands on: the fp64 references of tests/_bn_inputs.py against torch
autograd, the exactness budget of the dyadic family in integers, the tie share and the exclusion cap of the generators, the
recorded restatement distances, and the argument errors bn_act_pool.hip / reduce.hip return before any launch."""
import pytest
import torch
import torch.nn.functional as F

import _bn_inputs as bi
from _bn_inputs import POOL_MAX


@pytest.mark.parametrize("pool", bi.POOLS)
@pytest.mark.parametrize("shape", [(2, 5, 7, 6), (2, 4, 6, 4), (1, 1, 4, 4)])
def test_formula_references_agree_with_autograd(shape, pool):
    """forward_ref / dy_ref / sums_ref / dz_ref / bn_finalize_ref / bn_bwd_finalize_ref against torch autograd through
    F.batch_norm(training=True) -> leaky_relu -> pool, everything fp64: to 1e-12."""
    B, D, H, W = shape
    C, slope, eps, mom = 5, 0.01, 2.0 ** -17, 0.125      # eps and momentum travel as C floats: values a float holds exactly
    g = torch.Generator().manual_seed(D + 10 * pool)
    z = (torch.randn((B, D, H, W, C), generator=g, dtype=torch.float64) * 2 + 3).requires_grad_(True)
    gamma = (torch.randn(C, generator=g, dtype=torch.float64) + 0.2).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    rmean0, rvar0 = torch.randn(C, generator=g, dtype=torch.float64), torch.rand(C, generator=g, dtype=torch.float64) + 0.5
    dout = torch.randn(bi.pooled_shape(shape, pool) + (C,), generator=g, dtype=torch.float64)
    rmean, rvar = rmean0.clone(), rvar0.clone()
    a = F.leaky_relu(F.batch_norm((z + bias).permute(0, 4, 1, 2, 3), rmean, rvar, gamma, beta, True, mom, eps), slope)
    out = bi._pool(a, pool).permute(0, 2, 3, 4, 1)
    if out.numel():
        out.backward(dout)
    else:
        (a.sum() * 0).backward()
    count = B * D * H * W
    zd = z.detach()
    part = torch.stack([zd.sum((0, 1, 2, 3)), (zd * zd).sum((0, 1, 2, 3))]).unsqueeze(0)
    fin = bi.bn_finalize_ref(part, count, gamma.detach(), beta.detach(), bias, rmean0, rvar0, mom, eps)

    def close(u, v):
        return float((u - v).abs().max()) <= 1e-12 * max(1.0, float(v.abs().max())) if v.numel() else True
    assert close(fin["running_mean"], rmean) and close(fin["running_var"], rvar)
    m = zd.mean((0, 1, 2, 3))
    assert close(fin["mean"], m) and close(fin["var"], zd.var((0, 1, 2, 3), unbiased=False))
    invstd = 1.0 / torch.sqrt(fin["var"] + eps)
    scale = gamma.detach() * invstd
    shift = beta.detach() - m * scale
    assert close(bi.forward_ref(zd, scale, shift, slope, pool), out.detach())
    dy = bi.dy_ref(zd, dout, scale, shift, slope, pool)
    s1, s2 = bi.sums_ref(zd, dy, m, invstd)
    assert close(s1, beta.grad) and close(s2, gamma.grad)
    dgamma, dbeta, coef = bi.bn_bwd_finalize_ref(torch.stack([s1, s2]).unsqueeze(0), count)
    assert torch.equal(dgamma, s2) and torch.equal(dbeta, s1)
    assert close(bi.dz_ref(zd, dy, scale, m, invstd, coef), z.grad)
    assert close(bi.dz_ref_folded(zd, dy, scale, m, invstd, coef), z.grad)


def test_finalize_reference_clamp_and_count_one():
    """var < 0 is clamped (invstd = 1 / sqrt(eps) exactly), count 1 leaves the variance as it is, and the constant channels of
    stat_partials land on BOTH sides of zero over the cases the GPU test runs."""
    part = torch.tensor([[[3.0, 1.0], [8.9, 1.0]]])                         # channel 0: E[z^2] - m^2 = 8.9 - 9 < 0
    r = bi.bn_finalize_ref(part, 1.0, torch.ones(2), torch.zeros(2), None, torch.zeros(2), torch.zeros(2), 1.0, 1e-5)
    assert r["var"][0] == 0 and r["invstd"][0] == 1.0 / torch.sqrt(torch.tensor(bi.f32(1e-5), dtype=torch.float64))
    assert r["running_var"][1] == r["var"][1] == 0.0 and r["running_var"][0] == 0
    r = bi.bn_finalize_ref(torch.tensor([[[4.0], [10.0]]]), 2.0, torch.ones(1), torch.zeros(1), None, None, torch.zeros(1), 1.0, 1e-5)
    assert r["var"][0] == 1.0 and r["running_var"][0] == 2.0 and "running_mean" not in r
    signs = set()
    for nblk in bi.FIN_NBLK:
        for C in bi.FIN_CHANNELS[1:]:
            count = float(37 * nblk + 5)
            s = bi.stat_partials(nblk, C, count).double().sum(0)
            v = s[1] / count - (s[0] / count) ** 2
            for c in (1, 2):
                assert abs(float(v[c])) < 1e-3 * 37.3 ** 2
                signs.add(float(v[c]) < 0)
    assert signs == {True, False}


@pytest.mark.parametrize("pool", bi.POOLS)
@pytest.mark.parametrize("C", [6, 64])
@pytest.mark.parametrize("shape", bi.EXACT_SHAPES + [c[0] for c in bi.EXACT_GRID_STRIDE[:1]])
def test_exact_family_budget_in_integers(shape, C, pool):
    """Scaled to integers, every term of S1 / S2 of the dyadic family is integral and sum |terms| < 2^24 (so every partial sum of
    every order is an fp32 number); y is never 0; the tensors are bf16-exact; and an fp32 evaluation of either algebraic form of dz
    equals the fp64 one."""
    inp = bi.exact_inputs(shape, C, pool)
    z, dout = inp["z"], inp["dout"]
    for t in (z, dout):
        assert torch.equal(t.bfloat16().float(), t)
    y = z.double() * inp["scale"].double() + inp["shift"].double()
    assert torch.equal(y * 16, (y * 16).round()) and bool(((y * 16).long() % 2 == 1).all()) and float(y.abs().max()) <= 5.0625
    s = bi.f32(bi.EXACT_SLOPE)
    dy = bi.dy_ref(z, dout, inp["scale"], inp["shift"], s, pool)
    xhat = (z.double() - inp["mean"].double()) * inp["invstd"].double()
    for terms in (dy, dy * xhat):
        t64 = terms * 64
        assert torch.equal(t64, t64.round()) and float(terms.abs().max()) < 16
        assert int(t64.abs().long().sum((0, 1, 2, 3)).max()) < 1 << 24
    dz = bi.dz_ref(z, dy, inp["scale"], inp["mean"], inp["invstd"], inp["coef"])
    assert torch.equal(bi.dz_ref(z, dy, inp["scale"], inp["mean"], inp["invstd"], inp["coef"], torch.float32).double(), dz)
    assert torch.equal(bi.dz_ref_folded(z, dy, inp["scale"], inp["mean"], inp["invstd"], inp["coef"], torch.float32).double(), dz)
    out = bi.forward_ref(z, inp["scale"], inp["shift"], s, pool)
    assert torch.equal(bi.forward_ref(z, inp["scale"], inp["shift"], s, pool, torch.float32).double(), out)


@pytest.mark.parametrize("C", bi.EXACT_CHANNELS[:6])
@pytest.mark.parametrize("shape", [s for s in bi.EXACT_SHAPES if 0 not in bi.pooled_shape(s, POOL_MAX)])
def test_exact_family_has_ties(shape, C):
    inp = bi.exact_inputs(shape, C, POOL_MAX)
    assert bi.tie_share(inp["z"], inp["scale"], inp["shift"]) > 0.5
    assert C == 1 or int((inp["scale"] == 0).sum()) >= 1


@pytest.mark.parametrize("case", bi.COND_CASES, ids=str)
def test_conditioning_family_exclusions_and_distances(case):
    """The ambiguity exclusion stays below 1 % of the windows / voxels of every case, the channels have the conditioning asked
    for, and the recorded restatement distances have not drifted by more than a factor of 2."""
    C, io, shape, pool = case
    inp, excluded = bi.cond_inputs(C, io, shape, pool)
    assert excluded <= bi.COND_MAX_EXCLUDED
    z = inp["z"].double()
    ratio = z.mean((0, 1, 2, 3)).abs() / z.std((0, 1, 2, 3))
    for r, want in zip(ratio[:3], bi.COND_RATIOS):
        assert abs(float(r) - want) < 0.1 * want + 0.15
    assert bool((inp["scale"] > 0).any()) and bool((inp["scale"] < 0).any())
    now, rec = bi.cond_restatement_distance(C, io, shape, pool), bi.COND_DISTANCE[case]
    for k in bi.COND_QUANTITIES:
        assert rec[k] / 2 <= now[k] <= rec[k] * 2, f"{case} {k}: recorded {rec[k]:.3e}, measured {now[k]:.3e}"


def test_colsum_partials_cancel():
    for nblk in bi.COLSUM_NBLK:
        p = bi.colsum_partials(nblk, 65)
        assert int(p.abs().max()) <= 1 << 20 and int(p.sum(0).abs().max()) <= 8
        assert nblk < 3 or int(p.abs().max()) > 1 << 16


def test_argument_errors_before_any_launch():
    """io = 2 -> TMF_E_ARG; C = 257 and C = 1028 (more than 256 lanes per row) -> TMF_E_SHAPE; a misaligned tensor pointer ->
    TMF_E_ALIGN; nblk = 0 -> TMF_E_SHAPE.  No launch happens, so the pointers only have to be non-NULL."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    E_SHAPE, E_ALIGN, E_ARG = -2, -3, -5
    p, q = 4096, 4096 + 4                                        # aligned / misaligned
    geo = (2, 4, 4, 4)
    for io, C, z, rc in ((2, 8, p, E_ARG), (0, 257, p, E_SHAPE), (0, 1028, p, E_SHAPE), (3, 1028, p, E_SHAPE), (0, 8, q, E_ALIGN)):
        for pool in bi.POOLS:
            assert lib.tmf_bn_act_pool_fwd_t(z, p, p, p, *geo, C, pool, 0.01, io, None) == rc
            assert lib.tmf_bn_act_pool_bwd_reduce_t(z, p, p, p, p, p, p, *geo, C, pool, 0.01, io, None) == rc
            assert lib.tmf_bn_act_pool_bwd_apply_t(z, p, p, p, p, p, p, p, *geo, C, pool, 0.01, io, None) == rc
        if io == 0:
            assert lib.tmf_bn_act_pool_fwd_route(z, p, p, p, p, *geo, C, 0.01, None) == rc
            assert lib.tmf_bn_act_pool_bwd_reduce_route(z, p, p, p, p, p, p, *geo, C, 0.01, None) == rc
    assert lib.tmf_bn_act_pool_fwd_t(p, p, p, q, *geo, 8, 1, 0.01, 0, None) == E_ALIGN
    assert lib.tmf_bn_act_pool_bwd_apply_t(p, p, p, p, p, p, p, q, *geo, 8, 1, 0.01, 0, None) == E_ALIGN
    assert lib.tmf_bn_act_pool_fwd_t(p, p, p, p, *geo, 8, 3, 0.01, 0, None) == E_ARG               # unknown pool
    assert lib.tmf_bn_finalize(p, 0, 8, 64.0, p, p, None, None, None, 0.1, 1e-5, p, p, p, p, None) == E_SHAPE
    assert lib.tmf_bn_bwd_finalize(p, 0, 8, 64.0, None, None, p, None) == E_SHAPE
    assert lib.tmf_colsum_finalize(p, 0, 8, p, None) == E_SHAPE
    assert lib.tmf_bn_eval_coeffs(p, p, None, p, p, 1e-5, 0, p, p, None) == E_SHAPE
