"""Input-volume gradients on the GPU: the first block's data-gradient kernel (csrc/conv1_dgrad.hip) called on its own against
the fp64 reference of tests/_dgrad_inputs.py, the block path of ops.py against today's generic route, and the public
saliency interface."""
import functools

import pytest
import torch

import _dgrad_inputs as di

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _st():
    return torch.cuda.current_stream().cuda_stream


def run_dgrad(inp, shape, slope, split=1):
    """tmf_c1_bwd_dgrad on one case -> dx (B, D, H, W) on the host.  dx starts as NaN: every voxel must be written."""
    from transmf_ad_amd import _lib
    B, D, H, W, C = shape
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    dx = torch.full((B, D, H, W), float("nan"), device=DEV)
    nbytes = _lib.query("tmf_c1_bwd_dgrad_workspace_bytes", B, D, H, W, C)
    ws = torch.empty(nbytes // 4, device=DEV)
    _lib.call("tmf_set_option", b"c1_split", split)
    try:
        _lib.call("tmf_c1_bwd_dgrad", d["x"].data_ptr(), d["w"].data_ptr(), d["scale"].data_ptr(), d["shift"].data_ptr(),
                  d["mean"].data_ptr(), d["invstd"].data_ptr(), d["coef"].data_ptr(), d["dpool"].data_ptr() if d["dpool"].numel() else 0,
                  dx.data_ptr(), ws.data_ptr(), nbytes, B, D, H, W, C, float(slope), _st())
        torch.cuda.synchronize()
    finally:
        _lib.call("tmf_set_option", b"c1_split", 1)
    return dx.cpu()


@functools.lru_cache(maxsize=None)
def _exact(shape, train):
    inp = di.exact_inputs(shape, train)
    return inp, di.dx_ref(inp, di.EXACT_SLOPE)


@functools.lru_cache(maxsize=None)
def _cond(shape, train):
    inp, _ = di.cond_inputs(shape, train)
    return inp, di.dx_ref(inp, di.f32(di.COND_SLOPE))


# ---- 1. the kernel against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", (1, 0))
@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("shape", di.SHAPES)
def test_dgrad_exact_family_equals_fp64(shape, train, split):
    inp, ref = _exact(shape, train)
    got = run_dgrad(inp, shape, di.EXACT_SLOPE, split)
    bad = (got.double() != ref)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:8].tolist(), got[bad][:8].tolist(), ref[bad][:8].tolist())


@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("shape", di.SHAPES)
def test_dgrad_conditioning_family_within_table(shape, train):
    inp, ref = _cond(shape, train)
    got = run_dgrad(inp, shape, di.f32(di.COND_SLOPE))
    dist = di.distance(got, ref)
    print(f"dgrad cond {shape} train={train}: distance {dist:.3e}, bound {di.COND_MARGIN * di.COND_DISTANCE[(shape, train)]:.3e}")
    assert dist <= di.COND_MARGIN * di.COND_DISTANCE[(shape, train)], dist


@pytest.mark.parametrize("split", (1, 0))
def test_dgrad_two_runs_are_bit_identical(split):
    shape = di.SHAPES[1]
    inp, _ = _cond(shape, True)
    a = run_dgrad(inp, shape, di.f32(di.COND_SLOPE), split)
    b = run_dgrad(inp, shape, di.f32(di.COND_SLOPE), split)
    assert not torch.isnan(a).any() and torch.equal(a, b)


@pytest.mark.parametrize("train", (True, False))
def test_dgrad_without_pooling_windows_is_the_batchnorm_part(train):
    shape = di.EMPTY_POOL_SHAPE
    inp = di.exact_inputs(shape, train)
    assert inp["dpool"].numel() == 0
    ref = di.dx_ref(inp, di.EXACT_SLOPE)
    got = run_dgrad(inp, shape, di.EXACT_SLOPE)
    assert torch.equal(got.double(), ref)
    assert bool((ref != 0).any()) == train              # eval mode: no BatchNorm part, dx is all zero


# ---- 2. the block path: Conv1BnPool with an input that wants a gradient, against today's generic route ----------------------------
BLOCK_SHAPE = (2, 18, 20, 22)


@functools.lru_cache(maxsize=None)
def _block_case(C, train):
    shape = BLOCK_SHAPE + (C,)
    inp, _ = di.cond_inputs(shape, train)
    ref = di.dx_ref(inp, di.f32(di.COND_SLOPE))
    rest = di.COND_DISTANCE.get((shape, train))
    if rest is None:                                        # (C = 8 is not in the table: the restatement distance of this very case)
        rest = di.distance(di.dx_ref(inp, di.f32(di.COND_SLOPE), torch.float32), ref)
    return inp, ref, rest


def _run_block(fn_name, inp, C, train, want_dx=True, want_params=True):
    """One forward + backward of the first block through ops.Conv1BnPool or ops.ConvBnActPool -> (dx, dweight, dgamma, dbeta)."""
    from transmf_ad_amd import ops
    B, D, H, W = BLOCK_SHAPE
    x = inp["x"].to(DEV).view(B, D, H, W, 1).clone().requires_grad_(want_dx)
    weight = inp["w"].t().reshape(C, 1, 3, 3, 3).contiguous().to(DEV).requires_grad_(want_params)
    gamma = inp["gamma"].to(DEV).requires_grad_(want_params)
    beta = inp["beta"].to(DEV).requires_grad_(want_params)
    rmean, rvar = inp["mean"].to(DEV).clone(), inp["var"].to(DEV).clone()
    slope = di.f32(di.COND_SLOPE)
    if fn_name == "Conv1BnPool":
        out = ops.Conv1BnPool.apply(x, weight, None, gamma, beta, rmean, rvar, train, 0.1, di.COND_EPS, slope, False, None)
    else:
        out = ops.ConvBnActPool.apply(x, weight, None, gamma, beta, rmean, rvar, train, 0.1, di.COND_EPS, slope, "max", False, None)
    out.backward(inp["dpool"].to(DEV))
    torch.cuda.synchronize()
    return tuple(None if t.grad is None else t.grad.detach().cpu() for t in (x, weight, gamma, beta))


@pytest.mark.parametrize("train", (True, False))
@pytest.mark.parametrize("C", (8, 32))
def test_block_input_gradient_new_route_against_generic_route(C, train):
    """Both routes are fp32 evaluations of the same formulas: each may sit COND_MARGIN restatement distances from fp64, so the two
    differ by at most twice that."""
    inp, ref, rest = _block_case(C, train)
    new = _run_block("Conv1BnPool", inp, C, train)[0].view(BLOCK_SHAPE)
    old = _run_block("ConvBnActPool", inp, C, train)[0].view(BLOCK_SHAPE)
    top = float(ref.abs().max())
    d_new, d_old = di.distance(new, ref), di.distance(old, ref)
    d_pair = float((new.double() - old.double()).abs().max()) / top
    print(f"block C={C} train={train}: new {d_new:.3e}, generic {d_old:.3e}, new - generic {d_pair:.3e}, restatement {rest:.3e}")
    assert d_new <= di.COND_MARGIN * rest
    assert d_pair <= 2 * di.COND_MARGIN * rest


@pytest.mark.parametrize("gram", (1, 0))
@pytest.mark.parametrize("train", (True, False))
def test_block_parameter_gradients_do_not_depend_on_the_input_gradient(train, gram):
    from transmf_ad_amd import _lib
    C = 32
    inp, _ref, _rest = _block_case(C, train)
    _lib.call("tmf_set_option", b"c1_gram", gram)
    try:
        with_dx = _run_block("Conv1BnPool", inp, C, train, want_dx=True)
        without = _run_block("Conv1BnPool", inp, C, train, want_dx=False)
        frozen = _run_block("Conv1BnPool", inp, C, train, want_dx=True, want_params=False)
    finally:
        _lib.call("tmf_set_option", b"c1_gram", 1)
    assert without[0] is None and with_dx[0] is not None
    for a, b, name in zip(with_dx[1:], without[1:], ("dweight", "dgamma", "dbeta")):
        assert torch.equal(a, b), name
    assert all(t is None for t in frozen[1:])
    if not (train and gram):                                 # (the Gram pass takes its coef from other sums than tmf_bn_bwd_finalize's)
        assert torch.equal(frozen[0], with_dx[0])


# ---- 3. one call -----------------------------------------------------------------------------------------------------------------
def _snet_run(dim, one_call, vol_grad, frozen):
    import transmf_ad_amd as T
    from transmf_ad_amd import ops
    torch.manual_seed(21)
    net = T.sNet(dim).to(DEV).train()
    g = torch.Generator().manual_seed(22)
    vol = torch.randn((2, 1, 16, 18, 32), generator=g).to(DEV).requires_grad_(vol_grad)
    R = torch.randn((2, dim, 1, 1, 2), generator=g).to(DEV)
    if frozen:
        for p in net.parameters():
            p.requires_grad_(False)
    ops.SNET_ONE_CALL = one_call
    try:
        out = net(vol)
        node = type(out.grad_fn.next_functions[0][0]).__name__
        (out * R).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.SNET_ONE_CALL = True
    return node, vol.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in net.named_parameters()}


@pytest.mark.parametrize("dim", (32, 64))
def test_one_call_input_gradient_is_bit_identical_to_block_by_block(dim):
    node, dv1, g1 = _snet_run(dim, True, True, False)
    assert node.startswith("SNetTrain"), node
    node2, dv2, g2 = _snet_run(dim, False, True, False)
    assert not node2.startswith("SNetTrain")
    assert dv1 is not None and bool(torch.isfinite(dv1).all()) and float(dv1.abs().max()) > 0
    assert torch.equal(dv1, dv2)
    assert len(g1) == 28
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    # without the input gradient (tmf_snet_train_bwd = dvol NULL): the same 28 parameter gradients
    _n, dv0, g0 = _snet_run(dim, True, False, False)
    assert dv0 is None
    for k in g1:
        assert torch.equal(g1[k], g0[k]), k
    # frozen parameters (every dweight NULL)
    node3, dv3, g3 = _snet_run(dim, True, True, True)
    _n4, dv4, _g4 = _snet_run(dim, False, True, True)
    assert node3.startswith("SNetTrain") and all(v is None for v in g3.values())
    assert torch.equal(dv3, dv4)


# ---- 4. against the oracle -------------------------------------------------------------------------------------------------------
# Input gradient of a random linear read-out of the encoder output (the well-conditioned functional of
# test_gpu_model.test_activations_and_grads_match_oracle) for sNet(32) on (2, 1, 16, 16, 32).  The yardstick is the oracle's own
# fp32 run against its fp64 run on the same inputs, measured on the CPU (torch 2.x): (max-relative, L2-relative); the library may
# sit ORACLE_MARGIN of them from fp64.
ORACLE_FP32_DISTANCE = {True: (1.28e-06, 1.43e-06), False: (3.99e-07, 5.56e-07)}
ORACLE_MARGIN = 4.0


def _oracle_case(dim=32):
    import transmf_ad_amd as T
    torch.manual_seed(11)
    net = T.sNet(dim)
    g = torch.Generator().manual_seed(12)
    sd = net.state_dict()
    for k in sd:
        if k.endswith("running_mean"):
            sd[k].copy_(0.1 * torch.randn(sd[k].shape, generator=g))
        if k.endswith("running_var"):
            sd[k].copy_(0.5 + torch.rand(sd[k].shape, generator=g))
    x = torch.randn((2, 1, 16, 16, 32), generator=g)
    R = torch.randn((2, dim), generator=g)
    return net, x, R


def _oracle_grad(net, x, R, train, dtype):
    from oracle import tmf_oracle as O
    S = {k: (v.detach().clone().to(dtype) if v.dtype.is_floating_point else v.clone()) for k, v in net.state_dict().items()}
    xx = x.to(dtype).detach().clone().requires_grad_(True)
    out = O.snet_forward(S, "", R.shape[1], xx, train)
    return torch.autograd.grad((out.mean((2, 3, 4)) * R.to(dtype)).sum(), xx)[0]


@pytest.mark.parametrize("train", (True, False))
def test_input_gradient_matches_oracle(train):
    net, x, R = _oracle_case()
    ref = _oracle_grad(net, x, R, train, torch.float64)
    net = net.to(DEV)
    net.train(train)
    vol = x.to(DEV).requires_grad_(True)
    out = net(vol)
    got = torch.autograd.grad((out.mean((2, 3, 4)) * R.to(DEV)).sum(), vol)[0].double().cpu()
    d = got - ref
    dmax, dl2 = float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())
    bmax, bl2 = (ORACLE_MARGIN * v for v in ORACLE_FP32_DISTANCE[train])
    print(f"oracle train={train}: max-rel {dmax:.3e} (bound {bmax:.3e}), L2-rel {dl2:.3e} (bound {bl2:.3e})")
    assert dl2 <= bl2
    assert dmax <= bmax


# ---- 5. saliency -----------------------------------------------------------------------------------------------------------------
def _model_ad():
    import transmf_ad_amd as T
    torch.manual_seed(31)
    return T.model_ad(dim=64, depth=1, heads=4, dim_head=16, mlp_dim=256, dropout=0.0).to(DEV)


def _pair():
    g = torch.Generator().manual_seed(32)
    return tuple(torch.randn((2, 1, 32, 32, 32), generator=g).to(DEV) for _ in range(2))


def _hand_written(model, vols, target):
    leaves = [v.detach().clone().requires_grad_(True) for v in vols]
    out = model(*leaves)
    logits = out[0] if isinstance(out, tuple) else out
    if target is None:
        target = logits.detach().argmax(1)
    return torch.autograd.grad(logits.gather(1, target.view(-1, 1)).sum(), leaves)


@pytest.mark.parametrize("target", (None, [1, 0]))
@pytest.mark.parametrize("train", (False, True))
def test_input_gradients_of_model_ad(train, target):
    from transmf_ad_amd import input_gradients
    m = _model_ad()
    m.train(train)
    mri, pet = _pair()
    tgt = None if target is None else torch.tensor(target, device=DEV)
    torch.manual_seed(5)                                    # (train mode: the head's Dropout masks)
    got = input_gradients(m, mri, pet, target=tgt)
    assert all(p.requires_grad and p.grad is None for p in m.parameters())
    assert not mri.requires_grad and mri.grad is None
    for p in m.parameters():
        p.requires_grad_(False)
    torch.manual_seed(5)
    want = _hand_written(m, (mri, pet), tgt)
    assert len(got) == 2
    for g_, w_, v in zip(got, want, (mri, pet)):
        assert g_.shape == v.shape and bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0
        assert torch.equal(g_, w_)


def test_model_single_and_integrated_gradients():
    import transmf_ad_amd as T
    from transmf_ad_amd import input_gradients, integrated_gradients
    torch.manual_seed(41)
    m = T.model_single(128).to(DEV).eval()
    vol = _pair()[0]
    (g_,) = input_gradients(m, vol)
    assert g_.shape == vol.shape and bool(torch.isfinite(g_).all()) and float(g_.abs().max()) > 0
    # integrated gradients = its definition, written as a loop over input_gradients
    steps = 4
    with torch.no_grad():
        target = m(vol).argmax(1)
    acc = torch.zeros_like(vol)
    for k in range(steps):
        acc += input_gradients(m, ((k + 0.5) / steps) * vol, target=target)[0]
    (ig,) = integrated_gradients(m, vol, steps=steps)
    assert torch.equal(ig, vol * (acc / steps))
    assert all(p.requires_grad and p.grad is None for p in m.parameters())


# ---- 6. the routing is the forward's, on windows NO reference can decide ---------------------------------------------------------
# x = 1 + k 2^-22 (k in -4 .. 4): the z of a window's eight voxels are a few units in the last place apart, so which of them is the
# maximum depends on the order of the 27 products — in fp64 most of these windows are "ambiguous" and sections 1 - 4 exclude such
# windows or are exact by construction.  Here nothing is excluded: the reference takes the routing from the FORWARD kernel
# (tmf_c1_bn_pool_fwd_route's arg and z_sel) and only the sums from fp64, so one window routed differently from the forward shows
# as an error of the size of a whole term (~1e-2 of max |dx|), four orders above the bound.
NEAR_TIE_SHAPES = [(1, 9, 13, 35, 40), (2, 18, 20, 22, 32)]


@functools.lru_cache(maxsize=None)
def _near_tie_inputs(shape):
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(77 + C)
    x = 1.0 + torch.randint(-4, 5, (B, D, H, W), generator=g).float() * 2.0 ** -22
    w = (0.2 * torch.randn((27, C), generator=g)).float()
    scale = ((0.5 + torch.rand(C, generator=g)) * torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)).float()
    z = di.z_ref(x, w)
    shift = (-(z.mean((0, 2, 3, 4)) * scale.double())).float() + 1e-6 * torch.randn(C, generator=g)      # y straddles 0: both LeakyReLU branches
    dpool = torch.randn((B, D // 2, H // 2, W // 2, C), generator=g).float()
    zero = torch.zeros(C)
    return dict(x=x, w=w, scale=scale, shift=shift, mean=zero, invstd=torch.ones(C), coef=torch.zeros(2, C), dpool=dpool)


@pytest.mark.parametrize("split", (1, 0))
@pytest.mark.parametrize("shape", NEAR_TIE_SHAPES, ids=str)
def test_dgrad_routes_as_the_forward_kernel_on_undecidable_windows(shape, split):
    import torch.nn.functional as F
    from transmf_ad_amd import _lib
    B, D, H, W, C = shape
    inp = _near_tie_inputs(shape)
    slope = di.f32(di.COND_SLOPE)
    # the case is what it claims: in most windows the top two y are closer than fp32 can tell apart reliably
    z64 = di.z_ref(inp["x"], inp["w"])
    y64 = di.windows((z64 * inp["scale"].double().view(1, -1, 1, 1, 1) + inp["shift"].double().view(1, -1, 1, 1, 1)).permute(0, 2, 3, 4, 1))
    top = y64.topk(2, -1).values
    tight = (top[..., 0] - top[..., 1]) < 8 * 2.0 ** -24 * y64.abs().amax(-1).clamp_min(z64.abs().max() * 2.0 ** -3)
    assert float(tight.float().mean()) > 0.25, float(tight.float().mean())
    # the forward's routing
    d = {k: v.to(DEV).contiguous() for k, v in inp.items()}
    pooled = torch.empty((B, D // 2, H // 2, W // 2, C), device=DEV)
    zsel = torch.empty_like(pooled)
    arg = torch.empty(pooled.shape, device=DEV, dtype=torch.uint8)
    _lib.call("tmf_set_option", b"c1_split", split)
    try:
        _lib.call("tmf_c1_bn_pool_fwd_route", d["x"].data_ptr(), d["w"].data_ptr(), d["scale"].data_ptr(), d["shift"].data_ptr(),
                  pooled.data_ptr(), zsel.data_ptr(), arg.data_ptr(), B, D, H, W, C, float(slope), _st())
        torch.cuda.synchronize()
    finally:
        _lib.call("tmf_set_option", b"c1_split", 1)
    arg, zsel = arg.cpu().long(), zsel.cpu()
    assert int(arg.max()) <= 7 and len(torch.unique(arg)) == 8
    # dy from that routing (k = 4 d + 2 h + w), the LeakyReLU branch from the forward's own y = fma(z_sel, scale, shift)
    ymax = zsel.double() * inp["scale"].double() + inp["shift"].double()      # (the sign of fma(z_sel, scale, shift): one rounding keeps it)
    gl = inp["dpool"].double() * torch.where(ymax > 0, 1.0, slope)
    OD, OH, OW = D // 2, H // 2, W // 2
    dyw = torch.zeros((B, OD, OH, OW, C, 8), dtype=torch.float64).scatter_(-1, arg.unsqueeze(-1), gl.unsqueeze(-1))
    dy = torch.zeros((B, D, H, W, C), dtype=torch.float64)
    dy[:, :2 * OD, :2 * OH, :2 * OW] = dyw.view(B, OD, OH, OW, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(B, 2 * OD, 2 * OH, 2 * OW, C)
    dz = (dy * inp["scale"].double()).permute(0, 4, 1, 2, 3)
    ref = F.conv_transpose3d(dz, di.conv_weight(inp["w"], torch.float64), padding=1)[:, 0]
    rest = di.distance(F.conv_transpose3d(dz.float(), di.conv_weight(inp["w"], torch.float32), padding=1)[:, 0], ref)
    got = run_dgrad(inp, shape, slope, split)
    dist = di.distance(got, ref)
    term = float((inp["scale"].abs().max() * inp["w"].abs().max() * inp["dpool"].abs().median()) / ref.abs().max())
    print(f"near ties {shape} c1_split={split}: tight windows {float(tight.float().mean()):.2f}, distance {dist:.3e}, "
          f"restatement {rest:.3e}, one typical misrouted term {term:.1e}")
    assert dist <= di.COND_MARGIN * rest
