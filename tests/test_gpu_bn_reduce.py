"""bn_act_pool.hip and reduce.hip called on their own (through _lib.call with raw pointers, nothing of ops.py in between)
against the fp64 references of tests/_bn_inputs.py.

A. exact arithmetic: dyadic inputs on which every result is exact under ANY order of additions, with planted ties, exact
   zeros of scale and border windows - torch.equal to the fp64 reference cast to the output type;
B. conditioning: channels with |mean| / sd of 0, 3 and 30 in one tensor, judged per channel against the measured distance of the
   fp32 restatement of the reference (COND_DISTANCE) times COND_MARGIN;
C. the three finalize kernels on partials of the test's choosing (clamped variance, count 1, NULL buffers);
D. tmf_reduce_slabs under each of its plans through the weight gradients, in integers, and tmf_colsum_finalize.

Every output lives in one device arena between bands of NaN bytes; the arena is read back once and every byte outside the
outputs (the inputs included) must be unchanged, every output free of NaN."""
import functools
import math

import pytest
import torch

import _bn_inputs as bi
from _bn_inputs import POOL_MAX, POOL_NONE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND = 512                  # bytes between two slots: 128 float / 256 bf16 sentinel elements on either side of every tensor


class Arena:
    """One device allocation holding the inputs (first) and the outputs of a case at 256-byte aligned offsets, BAND bytes of
    0xFF (NaN in float and in bf16) between neighbours and at both ends.  Outputs start as NaN.  `tail`: more such bytes behind
    the last slot, for kernels that walk rows of a buffer - a loop bound that is off by an unroll step then reads inside this
    allocation (and NaN) instead of beyond it."""

    def __init__(self, inputs, outputs, tail=0):
        self.slots, self.out_names = {}, list(outputs)
        at = BAND
        for name, t in inputs.items():
            n = t.numel() * t.element_size()
            self.slots[name] = (at, n, t.dtype, tuple(t.shape))
            at += (n + 255) // 256 * 256 + BAND
        for name, (shape, dtype) in outputs.items():
            n = math.prod(shape) * torch.empty(0, dtype=dtype).element_size()
            self.slots[name] = (at, n, dtype, tuple(shape))
            at += (n + 255) // 256 * 256 + BAND
        self.host = torch.full((at + tail,), 0xFF, dtype=torch.uint8)
        for name, t in inputs.items():
            off, n = self.slots[name][:2]
            self.host[off:off + n] = t.contiguous().view(-1).view(torch.uint8)
        self.dev = self.host.to(DEV)
        self.base = self.dev.data_ptr()
        assert self.base % 256 == 0

    def ptr(self, name):
        return self.base + self.slots[name][0]

    def fetch(self, may_nan=(), workspace=(), written=None):
        """Synchronise, check the bytes outside the outputs, return {output name: host tensor}.  `may_nan`: outputs whose
        values may be NaN by computation (they must still be fully written: no element keeps the fill pattern, which no
        arithmetic produces); `workspace`: scratch slots - their surroundings are checked, their content is not judged;
        `written`: {output name: bool tensor of its shape} for an output that is a strided block of its slot - the elements
        marked False must keep the fill pattern, the checks above apply to the others."""
        torch.cuda.synchronize()
        back = self.dev.cpu()
        at = 0
        for name in self.out_names:
            off, n = self.slots[name][:2]
            assert torch.equal(back[at:off], self.host[at:off]), f"bytes ahead of '{name}' were written"
            at = off + n
        assert torch.equal(back[at:], self.host[at:]), "bytes behind the last output were written"
        res = {}
        for name in self.out_names:
            off, n, dtype, shape = self.slots[name]
            res[name] = back[off:off + n].view(dtype).view(shape)
            if name in workspace:
                continue
            live = written.get(name) if written else None
            if live is not None or name in may_nan or not dtype.is_floating_point:
                word = {2: torch.int16, 4: torch.int32}[torch.empty(0, dtype=dtype).element_size()]
                fill = back[off:off + n].view(word).view(shape) == -1
            if live is None:
                live = ...
            else:
                assert bool(fill[~live].all()), f"'{name}': elements outside the output block were written"
            if name in may_nan or not dtype.is_floating_point:
                assert not bool(fill[live].any()), f"'{name}' holds unwritten elements"
            else:
                assert not torch.isnan(res[name][live]).any(), f"'{name}' holds NaN (unwritten or computed)"
        return res


def _st():
    return torch.cuda.current_stream().cuda_stream


def _call(name, *args):
    from transmf_ad_amd import _lib
    _lib.call(name, *args)


def _query(name, *args):
    from transmf_ad_amd import _lib
    return _lib.query(name, *args)


def run_block(inp, shape, C, pool, io, slope, coef=None, steps=("fwd", "reduce", "apply")):
    """tmf_bn_act_pool_fwd_t, tmf_bn_act_pool_bwd_reduce_t + tmf_bn_bwd_finalize, tmf_bn_act_pool_bwd_apply_t on one case.
    -> dict(out, partial, dgamma, dbeta, coef, dz) of host tensors (those of the steps asked for)."""
    B, D, H, W = shape
    zdt, ydt = bi.z_dtype(io), bi.y_dtype(io)
    coef = inp["coef"] if coef is None else coef
    ins = dict(scale=inp["scale"], shift=inp["shift"], mean=inp["mean"], invstd=inp["invstd"], coef_in=coef,
               dout=inp["dout"].to(ydt), z=inp["z"].to(zdt))
    nblk = _query("tmf_bn_act_pool_bwd_blocks", B, D, H, W, C, pool)
    outs = {}
    if "fwd" in steps:
        outs["out"] = (bi.pooled_shape(shape, pool) + (C,), ydt)
    if "reduce" in steps:
        outs.update(partial=((nblk, 2, C), torch.float32), dgamma=((C,), torch.float32), dbeta=((C,), torch.float32),
                    coef=((2, C), torch.float32))
    if "apply" in steps:
        outs["dz"] = ((B, D, H, W, C), zdt)
    a = Arena(ins, outs)
    p = a.ptr
    if "fwd" in steps:
        _call("tmf_bn_act_pool_fwd_t", p("z"), p("scale"), p("shift"), p("out"), B, D, H, W, C, pool, slope, io, _st())
    if "reduce" in steps:
        _call("tmf_bn_act_pool_bwd_reduce_t", p("z"), p("dout"), p("scale"), p("shift"), p("mean"), p("invstd"), p("partial"),
              B, D, H, W, C, pool, slope, io, _st())
        _call("tmf_bn_bwd_finalize", p("partial"), nblk, C, float(B * D * H * W), p("dgamma"), p("dbeta"), p("coef"), _st())
    if "apply" in steps:
        _call("tmf_bn_act_pool_bwd_apply_t", p("z"), p("dout"), p("scale"), p("shift"), p("mean"), p("invstd"), p("coef_in"),
              p("dz"), B, D, H, W, C, pool, slope, io, _st())
    return a.fetch()


# ---------------------------------------------------------------------------------------------------------------------
# A. exact arithmetic
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _exact_case(shape, C, pool):
    """Inputs and fp64 references of one exact case at both slopes (shared by the io modes; never modified)."""
    inp = bi.exact_inputs(shape, C, pool)
    if 0 not in bi.pooled_shape(shape, POOL_MAX):
        assert bi.tie_share(inp["z"], inp["scale"], inp["shift"]) > 0.5, "the exact family has too few ties"
    count = inp["z"].numel() // C
    refs = {}
    for slope in (bi.f32(bi.EXACT_SLOPE), bi.f32(0.01)):
        dy = bi.dy_ref(inp["z"], inp["dout"], inp["scale"], inp["shift"], slope, pool)
        s1, s2 = bi.sums_ref(inp["z"], dy, inp["mean"], inp["invstd"])
        refs[slope] = dict(out=bi.forward_ref(inp["z"], inp["scale"], inp["shift"], slope, pool), dy=dy,
                           dz=bi.dz_ref(inp["z"], dy, inp["scale"], inp["mean"], inp["invstd"], inp["coef"]),
                           dbeta=s1, dgamma=s2, coef=torch.stack([s1, s2]) / count)
    return inp, refs


def _check_exact(res, ref, io, what):
    for k in ("out", "dz"):
        if k in res:
            dt = bi.y_dtype(io) if k == "out" else bi.z_dtype(io)
            assert torch.equal(res[k], ref[k].to(dt)), f"{what}: {k} differs from the fp64 reference"
    if "partial" in res:
        for k in ("dgamma", "dbeta", "coef"):
            assert torch.equal(res[k], ref[k].float()), f"{what}: {k} differs from the fp64 reference"


def _check_one_ulp(res, ref, inp, pool, io, slope, what):
    """slope = 0.01 is not dyadic.  Where y >= 0 nothing changes (equality); where y < 0 the result may differ from the cast
    reference by one ulp of the output type, taken at the magnitude of the terms the kernel adds:
      out: |out| for no / max pool (one correctly rounded product); sum_k |a_k| for the average (8 rounded products and 7 rounded
           additions of at most ulp(sum |a|) / 2 each, then an exact / 8);
      dz:  |scale| (|dy| + |coef0| + |coef1| invstd (|z| + |mean|)) - dy = dout * c * slope is exact (dout and c are powers of two
           or 0), so either algebraic form rounds at most twice, by half an ulp at no more than that magnitude each."""
    z, sc, sh = inp["z"].double(), inp["scale"].double(), inp["shift"].double()
    y = z * sc + sh
    a = torch.where(y > 0, y, y * slope)
    ydt, zdt = bi.y_dtype(io), bi.z_dtype(io)
    if "out" in res and res["out"].numel():
        if pool == POOL_NONE:
            neg, mag = y < 0, ref["out"].abs()
        elif pool == POOL_MAX:
            neg, mag = ref["out"] < 0, ref["out"].abs()
        else:
            neg, mag = (bi.windows(y) < 0).any(-1), bi.windows(a).abs().sum(-1)
        tol = torch.where(neg, bi.ulp_at(mag, ydt), torch.zeros_like(mag))
        err = (res["out"].double() - ref["out"].to(ydt).double()).abs()
        assert bool((err <= tol).all()), f"{what}: out, worst excess {float((err - tol).max()):.3e}"
    if "dz" in res:
        k0, k1 = inp["coef"].double()
        mag = sc.abs() * (ref["dy"].abs() + k0.abs() + k1.abs() * inp["invstd"].double() * (z.abs() + inp["mean"].double().abs()))
        tol = torch.where(y < 0, bi.ulp_at(mag, zdt), torch.zeros_like(mag))
        err = (res["dz"].double() - ref["dz"].to(zdt).double()).abs()
        assert bool((err <= tol).all()), f"{what}: dz, worst excess {float((err - tol).max()):.3e}"


@pytest.mark.parametrize("io", bi.IO_MODES)
@pytest.mark.parametrize("pool", bi.POOLS)
@pytest.mark.parametrize("C", bi.EXACT_CHANNELS)
@pytest.mark.parametrize("shape", bi.EXACT_SHAPES)
def test_exact_block_equals_fp64(shape, C, pool, io):
    """Forward, reduce + finalize and apply on the dyadic grids: equal to the fp64 reference cast to the output type at slope
    1/4; at slope 0.01 equal where y >= 0 and within one ulp where y < 0 (the sums are not exact there and are left to B)."""
    inp, refs = _exact_case(shape, C, pool)
    s = bi.f32(bi.EXACT_SLOPE)
    res = run_block(inp, shape, C, pool, io, s)
    if pool != POOL_NONE and 0 in bi.pooled_shape(shape, pool):          # no pooled voxel: no gradient reaches the sums
        assert int((res["partial"] != 0).sum()) == 0
    _check_exact(res, refs[s], io, f"{shape} C={C} pool={pool} io={io}")
    s = bi.f32(0.01)
    res = run_block(inp, shape, C, pool, io, s, steps=("fwd", "apply"))
    _check_one_ulp(res, refs[s], inp, pool, io, s, f"{shape} C={C} pool={pool} io={io} slope=0.01")


@pytest.mark.parametrize("io", (0, 3))
@pytest.mark.parametrize("case", bi.EXACT_GRID_STRIDE, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}")
def test_exact_block_grid_stride(case, io):
    """More rows than the workgroup cap of the elementwise plan, so that workgroups walk several rows: the elementwise passes stay
    exact at any size; the sums only of the case that keeps the exactness budget (2744 voxels per channel, no pool)."""
    shape, C, pool = case
    inp = bi.exact_inputs(shape, C, pool)
    s = bi.f32(bi.EXACT_SLOPE)
    B, D, H, W = shape
    assert _query("tmf_bn_act_pool_bwd_blocks", B, D, H, W, C, pool) == 2048 < B * D * H * W // (8 if pool else 1)
    dy = bi.dy_ref(inp["z"], inp["dout"], inp["scale"], inp["shift"], s, pool)
    ref = dict(out=bi.forward_ref(inp["z"], inp["scale"], inp["shift"], s, pool),
               dz=bi.dz_ref(inp["z"], dy, inp["scale"], inp["mean"], inp["invstd"], inp["coef"]))
    steps = ("fwd", "apply")
    if pool == POOL_NONE:
        s1, s2 = bi.sums_ref(inp["z"], dy, inp["mean"], inp["invstd"])
        ref.update(dbeta=s1, dgamma=s2, coef=torch.stack([s1, s2]) / (B * D * H * W))
        steps = ("fwd", "reduce", "apply")
    _check_exact(run_block(inp, shape, C, pool, io, s, steps=steps), ref, io, f"{shape} C={C} pool={pool} io={io}")


@pytest.mark.parametrize("C", bi.EXACT_CHANNELS)
@pytest.mark.parametrize("shape", bi.EXACT_SHAPES)
def test_exact_saved_routing_equals_fp64(shape, C):
    """tmf_bn_act_pool_fwd_route and tmf_bn_act_pool_bwd_reduce_route on the same inputs: z_sel is z at the reference's first
    maximum of y, the pooled output and the finalized sums equal the fp64 reference."""
    inp, refs = _exact_case(shape, C, POOL_MAX)
    s = bi.f32(bi.EXACT_SLOPE)
    ref = refs[s]
    B, D, H, W = shape
    pooled = bi.pooled_shape(shape, POOL_MAX) + (C,)
    nblk = _query("tmf_bn_act_pool_bwd_blocks", B, D, H, W, C, POOL_MAX)
    ins = {k: inp[k] for k in ("scale", "shift", "mean", "invstd", "dout", "z")}
    a = Arena(ins, dict(out=(pooled, torch.float32), z_sel=(pooled, torch.float32), partial=((nblk, 2, C), torch.float32),
                        dgamma=((C,), torch.float32), dbeta=((C,), torch.float32), coef=((2, C), torch.float32)))
    p = a.ptr
    _call("tmf_bn_act_pool_fwd_route", p("z"), p("scale"), p("shift"), p("out"), p("z_sel"), B, D, H, W, C, s, _st())
    _call("tmf_bn_act_pool_bwd_reduce_route", p("z_sel"), p("dout"), p("scale"), p("shift"), p("mean"), p("invstd"), p("partial"),
          B, D, H, W, C, s, _st())
    _call("tmf_bn_bwd_finalize", p("partial"), nblk, C, float(B * D * H * W), p("dgamma"), p("dbeta"), p("coef"), _st())
    res = a.fetch()
    zw = bi.windows(inp["z"])
    y = zw.double() * inp["scale"].double().view(1, 1, 1, 1, C, 1) + inp["shift"].double().view(1, 1, 1, 1, C, 1)
    if zw.numel():
        assert torch.equal(res["z_sel"], zw.gather(-1, bi.first_max(y)[0].unsqueeze(-1)).squeeze(-1))
    _check_exact(res, ref, 0, f"route {shape} C={C}")


@pytest.mark.parametrize("ncol", bi.COLSUM_NCOL)
@pytest.mark.parametrize("nblk", bi.COLSUM_NBLK)
def test_colsum_finalize_integers(nblk, ncol):
    """tmf_colsum_finalize on integer partials up to 2^20 that cancel to small integers: equal to the integer column sums, for
    row counts on either side of every bound of the four-way unrolled loop of 16 slab lanes and its tail."""
    part = bi.colsum_partials(nblk, ncol)
    a = Arena(dict(part=part.float()), dict(out=((ncol,), torch.float32)), tail=64 * ncol * 4)
    _call("tmf_colsum_finalize", a.ptr("part"), nblk, ncol, a.ptr("out"), _st())
    assert torch.equal(a.fetch()["out"].long(), part.sum(0))


# ---------------------------------------------------------------------------------------------------------------------
# B. conditioning
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bi.COND_CASES, ids=lambda c: f"C{c[0]}-io{c[1]}-{'x'.join(map(str, c[2]))}-pool{c[3]}")
def test_conditioned_block_against_fp64(case):
    """Channels with |mean| / sd of 0, 3 and 30 and gamma of both signs in one tensor.  Each channel is judged against its own
    scale (cond_quantities: max |fp64| of the channel; sum |terms| of the channel for the two sums):
    |kernel - fp64| <= COND_MARGIN x COND_DISTANCE[case] x scale, plus half a bf16 ulp of the reference where the output is a
    bf16 tensor."""
    C, io, shape, pool = case
    inp, excluded = bi.cond_inputs(C, io, shape, pool)
    assert excluded <= bi.COND_MAX_EXCLUDED
    s = bi.f32(bi.COND_SLOPE)
    ref = bi.cond_quantities(inp, s, pool, torch.float64)
    res = run_block(inp, shape, C, pool, io, s, coef=ref["coef"])
    dist = bi.COND_DISTANCE[case]
    bad = []
    for k in bi.COND_QUANTITIES:
        got, want = res[k].double().reshape(-1, C), ref[k].reshape(-1, C)
        top = ref["top"][k].double()
        tol = bi.COND_MARGIN * dist[k] * top.view(1, C).expand_as(want).clone()
        dt = {"out": bi.y_dtype(io), "dz": bi.z_dtype(io)}.get(k, torch.float32)
        if dt == torch.bfloat16:
            tol += 0.5 * bi.ulp_at(want, dt)
        err = (got - want).abs()
        print(f"{case} {k}: kernel distance {bi.per_channel_distance(got, want, top):.3e}, restatement {dist[k]:.3e}, "
              f"worst err / tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
        if not bool((err <= tol).all()):
            bad.append(k)
    assert not bad, f"{case}: {bad} beyond {bi.COND_MARGIN} restatement distances"


# ---------------------------------------------------------------------------------------------------------------------
# C. finalize kernels
# ---------------------------------------------------------------------------------------------------------------------
def _within_ulps(got, ref, n, what):
    err = (got.double() - ref).abs()
    tol = n * bi.ulp_at(ref, torch.float32)
    assert bool((err <= tol).all()), f"{what}: worst {float((err / tol.clamp_min(1e-300)).max()) * n:.2f} ulp"


def _within_terms(got, ref, terms, what):
    err = (got.double() - ref).abs()
    tol = 4 * bi.U32 * terms
    assert bool((err <= tol).all()), f"{what}: worst err / (4 u sum|terms|) {float((err / tol.clamp_min(1e-300)).max()):.2f}"


FIN_VARIANTS = [dict(bias=True, running=True, momentum=0.1), dict(bias=False, running=True, momentum=1.0),
                dict(bias=True, running=False, momentum=0.1), dict(bias=False, running=True, momentum=0.1, count1=True)]


@pytest.mark.parametrize("variant", range(len(FIN_VARIANTS)))
@pytest.mark.parametrize("C", bi.FIN_CHANNELS)
@pytest.mark.parametrize("nblk", bi.FIN_NBLK)
def test_bn_finalize_chosen_partials(nblk, C, variant):
    """tmf_bn_finalize on partials with mean / sd up to 1e3 and constant channels (a variance a rounding error from zero: finite
    and equal to the clamped reference), with and without the folded conv bias and the running buffers, momentum 0.1 and 1,
    count 1 (nblk 1).  mean, invstd, scale within 2 fp32 ulp of fp64; shift and the running buffers within 4 u sum |terms|."""
    v = FIN_VARIANTS[variant]
    count = 1.0 if v.get("count1") and nblk == 1 else float(37 * nblk + 5)
    part = bi.stat_partials(nblk, C, count)
    gamma, beta, bias, rmean, rvar = bi.channel_vectors(C)
    ins = dict(part=part, gamma=gamma, beta=beta, bias=bias)
    outs = {k: ((C,), torch.float32) for k in ("mean", "invstd", "scale", "shift")}
    a = Arena(ins, outs)
    run = None
    if v["running"]:                                            # updated in place: device tensors of their own, compared whole
        run = torch.stack([rmean, rvar]).to(DEV)
    _call("tmf_bn_finalize", a.ptr("part"), nblk, C, count, a.ptr("gamma"), a.ptr("beta"), a.ptr("bias") if v["bias"] else None,
          run[0].data_ptr() if v["running"] else None, run[1].data_ptr() if v["running"] else None, v["momentum"], 1e-5,
          a.ptr("mean"), a.ptr("invstd"), a.ptr("scale"), a.ptr("shift"), _st())
    res = a.fetch()
    ref = bi.bn_finalize_ref(part, count, gamma, beta, bias if v["bias"] else None, rmean if v["running"] else None,
                             rvar if v["running"] else None, v["momentum"], 1e-5)
    what = f"nblk={nblk} C={C} {v}"
    for k in ("mean", "invstd", "scale"):
        assert bool(torch.isfinite(res[k]).all())
        _within_ulps(res[k], ref[k], 2, f"{what} {k}")
    _within_terms(res["shift"], ref["shift"], ref["terms"]["shift"], f"{what} shift")
    if v["running"]:
        run = run.cpu()
        assert bool(torch.isfinite(run).all())
        _within_terms(run[0], ref["running_mean"], ref["terms"]["running_mean"], f"{what} running_mean")
        _within_terms(run[1], ref["running_var"], ref["terms"]["running_var"], f"{what} running_var")


@pytest.mark.parametrize("null_grads", [False, True])
@pytest.mark.parametrize("C", bi.FIN_CHANNELS)
@pytest.mark.parametrize("nblk", bi.FIN_NBLK)
def test_bn_bwd_finalize_chosen_partials(nblk, C, null_grads):
    """tmf_bn_bwd_finalize on cancelling partials, with and without dgamma / dbeta: within 2 fp32 ulp of the fp64 sums."""
    part = bi.grad_partials(nblk, C)
    count = float(37 * nblk + 5)
    outs = dict(coef=((2, C), torch.float32))
    if not null_grads:
        outs.update(dgamma=((C,), torch.float32), dbeta=((C,), torch.float32))
    a = Arena(dict(part=part), outs)
    _call("tmf_bn_bwd_finalize", a.ptr("part"), nblk, C, count, None if null_grads else a.ptr("dgamma"),
          None if null_grads else a.ptr("dbeta"), a.ptr("coef"), _st())
    res = a.fetch()
    dgamma, dbeta, coef = bi.bn_bwd_finalize_ref(part, count)
    _within_ulps(res["coef"], coef, 2, f"nblk={nblk} C={C} coef")
    if not null_grads:
        _within_ulps(res["dgamma"], dgamma, 2, f"nblk={nblk} C={C} dgamma")
        _within_ulps(res["dbeta"], dbeta, 2, f"nblk={nblk} C={C} dbeta")


@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("C", bi.EVAL_CHANNELS)
def test_bn_eval_coeffs(C, with_bias):
    """tmf_bn_eval_coeffs (fp32 throughout) within 4 u sum |terms| of its closing expressions in fp64."""
    gamma, beta, bias, rmean, rvar = bi.channel_vectors(C)
    a = Arena(dict(gamma=gamma, beta=beta, bias=bias, rmean=rmean, rvar=rvar), dict(scale=((C,), torch.float32), shift=((C,), torch.float32)))
    _call("tmf_bn_eval_coeffs", a.ptr("gamma"), a.ptr("beta"), a.ptr("bias") if with_bias else None, a.ptr("rmean"), a.ptr("rvar"),
          1e-5, C, a.ptr("scale"), a.ptr("shift"), _st())
    res = a.fetch()
    scale, shift, terms = bi.bn_eval_coeffs_ref(gamma, beta, bias if with_bias else None, rmean, rvar, 1e-5)
    _within_terms(res["scale"], scale, scale.abs(), f"C={C} scale")
    _within_terms(res["shift"], shift, terms, f"C={C} shift")


# ---------------------------------------------------------------------------------------------------------------------
# D. the slab reduction under every plan, through its callers
# ---------------------------------------------------------------------------------------------------------------------
BIG, MID, SMALL = (2, 16, 24, 24), (2, 12, 24, 24), (1, 8, 8, 8)         # 72, 54 and 8 bricks of the 3x3x3 kernels
# (entry, shape, cin, cout, ksize, plan): plan = stages and width of tmf_reduce_slabs for n = k^3 cin cout sums
WGRAD_CASES = [
    ("tmf_conv3d_wgrad", BIG, 8, 8, 3, "two-wide"), ("tmf_conv3d_wgrad", BIG, 5, 7, 3, "two-scalar"),
    ("tmf_conv3d_wgrad", SMALL, 8, 8, 3, "one-wide"), ("tmf_conv3d_wgrad", SMALL, 5, 7, 3, "one-scalar"),
    ("tmf_conv3d_wgrad", MID, 8, 8, 3, "one-wide-unrolled"), ("tmf_conv3d_wgrad", MID, 5, 7, 3, "one-scalar-unrolled"),
    ("tmf_conv3d_wgrad", BIG, 32, 32, 1, "two-wide"), ("tmf_conv3d_wgrad", BIG, 8, 8, 1, "two-scalar"),
    ("tmf_conv3d_wgrad", SMALL, 8, 8, 1, "one-scalar"),
    ("tmf_conv3d_c1_wgrad", BIG, 1, 64, 3, "two-wide"), ("tmf_conv3d_c1_wgrad", BIG, 1, 32, 3, "two-scalar"),
    ("tmf_conv3d_c1_wgrad", SMALL, 1, 32, 3, "one-scalar"),
    ("tmf_conv3d_wgrad_bf16", BIG, 8, 8, 3, "two-wide"), ("tmf_conv3d_wgrad_bf16", SMALL, 8, 8, 3, "one-wide"),
]


@functools.lru_cache(maxsize=None)
def _wgrad_case(shape, cin, cout, ksize):
    x, dz = bi.wgrad_inputs(shape, cin, cout)
    return x, dz, bi.wgrad_ref(x, dz, ksize)


@pytest.mark.parametrize("layout", [0, 1], ids=["tapmajor", "reference"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: f"{c[0][4:]}-{'x'.join(map(str, c[1]))}-{c[2]}-{c[3]}-k{c[4]}-{c[5]}")
def test_weight_gradient_integers_every_reduce_plan(case, layout):
    """Integer x and dz in [-2, 2]: every slab, the fp64 sums and the fp32 round trip through scratch are exact, so dw equals the
    fp64 conv3d weight gradient in both layouts - with one and two stages, 4-wide and scalar.  The plan is read from the
    workspace size (slabs + groups: at most 65 with one stage, at least 69 with two) and asserted, so that a change of planner
    that empties a case fails here."""
    entry, shape, cin, cout, ksize, plan = case
    B, D, H, W = shape
    x, dz, ref = _wgrad_case(shape, cin, cout, ksize)
    n = ksize ** 3 * cin * cout
    if entry == "tmf_conv3d_wgrad":
        nbytes = _query("tmf_conv3d_wgrad_workspace_bytes", B, D, H, W, cin, cout, ksize)
    elif entry == "tmf_conv3d_c1_wgrad":
        nbytes = _query("tmf_conv3d_c1_wgrad_workspace_bytes", B, D, H, W, cout)
    else:
        nbytes = _query("tmf_conv3d_wgrad_bf16_workspace_bytes", B, D, H, W, cin, cout)
    slabs_groups = nbytes // (4 * n)
    assert nbytes == slabs_groups * 4 * n
    stages, width = plan.split("-")[:2]
    assert slabs_groups <= 65 if stages == "one" else slabs_groups >= 69, f"plan changed: slabs + groups = {slabs_groups}"
    if plan.endswith("unrolled"):                               # more than 48 slabs in one group: the four-way unrolled loop runs
        assert 50 <= slabs_groups <= 65
    assert (n % 4 == 0 and n >= 1024) == (width == "wide")
    if entry == "tmf_conv3d_c1_wgrad":
        x = x[..., 0]
    a = Arena(dict(x=x, dz=dz), dict(dw=((n,), torch.float32), ws=((nbytes // 4,), torch.float32)), tail=64 * n * 4)
    a.dev[a.slots["ws"][0]:a.slots["ws"][0] + nbytes] = 0          # the workspace is scratch: only its surroundings are judged
    p = a.ptr
    if entry == "tmf_conv3d_wgrad":
        _call(entry, p("x"), p("dz"), p("dw"), p("ws"), nbytes, B, D, H, W, cin, cout, ksize, layout, _st())
    elif entry == "tmf_conv3d_c1_wgrad":
        _call(entry, p("x"), p("dz"), p("dw"), p("ws"), nbytes, B, D, H, W, cout, layout, _st())
    elif layout == 0:
        _call("tmf_conv3d_wgrad_bf16", p("x"), p("dz"), p("dw"), p("ws"), nbytes, B, D, H, W, cin, cout, _st())
    else:                                                       # the entry with a layout argument (float tensors: io 0)
        _call("tmf_conv3d_wgrad_bf16_t", p("x"), p("dz"), p("dw"), p("ws"), nbytes, B, D, H, W, cin, cout, 0, layout, _st())
    dw = a.fetch()["dw"]
    want = ref if layout == 1 else bi.tap_major(ref)
    assert torch.equal(dw.double(), want.reshape(-1))
