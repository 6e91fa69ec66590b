"""The max-pool routing kept by the forward (option "pool_recompute" 0, the default) against the recomputing kernels
("pool_recompute" 1): the saved z of each window's first maximum (and, in the first block, its index) is the very value the
backward used to re-derive, so every comparison here is torch.equal — partial slabs, gradients and the pooled outputs."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"


def _desc(flags=0, precision=0, B=8, D=96, H=96, W=96, dim=128):
    from transmf_ad_amd import _lib
    desc = _lib.SnetDesc(B=B, D=D, H=H, W=W, dim=dim, precision=precision, storage_bf16=0, flags=flags)
    desc.momentum[:] = [0.1] * 7
    desc.eps[:] = [1e-5] * 7
    desc.slope[:] = [0.01] * 7
    return desc


def test_saved_workspace_grows_by_exactly_the_routing_bytes():
    """Host arithmetic (no GPU): tmf_snet_saved_bytes with the default word holds, per encoder, pooled x 4 B + pooled x 1 B for
    block 0 and pooled x 4 B for blocks 2 and 4 (256-byte granules) more than with the recompute bits; "c1_gram" 0 drops block 0's
    share, the bf16 precision and the eval workspace hold none; the default word itself is unchanged."""
    from transmf_ad_amd import _lib, ops
    lib = _lib.load()
    ALGO, P, X, G, S, RC1, RBN = 0x100, 0x800, 0x1000, 0x2000, 0x8000, 0x10000, 0x20000
    word = ALGO | (3 << 9) | P | X | G | S
    assert lib.tmf_snet_algo_flags() == word

    def saved(flags, **kw):
        return lib.tmf_snet_saved_bytes(ctypes.byref(_desc(flags, **kw)))

    def up256(n):
        return (n + 255) // 256 * 256
    for (B, D, H, W, dim) in [(8, 96, 96, 96, 128), (2, 91, 109, 91, 64)]:
        kw = dict(B=B, D=D, H=H, W=W, dim=dim)
        p0 = B * (D // 2) * (H // 2) * (W // 2) * (dim // 4)
        p2 = B * (D // 4) * (H // 4) * (W // 4) * (dim // 2)
        p4 = B * (D // 8) * (H // 8) * (W // 8) * dim
        c1, bn = up256(4 * p0) + up256(p0), up256(4 * p2) + up256(4 * p4)
        base = saved(word | RC1 | RBN, **kw)
        assert saved(word, **kw) == saved(0, **kw) == base + c1 + bn
        assert saved(word | RC1, **kw) == base + bn and saved(word | RBN, **kw) == base + c1
        no_gram = saved(word & ~G, **kw)
        assert no_gram == saved((word & ~G) | RC1 | RBN, **kw) + bn          # without the Gram path block 0 keeps nothing
        assert saved(word, precision=1, **kw) == saved(word | RC1 | RBN, precision=1, **kw)        # bf16: no routing
        assert lib.tmf_snet_eval_workspace_bytes(ctypes.byref(_desc(word, **kw))) == \
            lib.tmf_snet_eval_workspace_bytes(ctypes.byref(_desc(word | RC1 | RBN, **kw)))
    try:
        for v, bits in ((1, RC1 | RBN), (2, RC1), (3, RBN), (0, 0)):
            assert lib.tmf_set_option(b"pool_recompute", v) == 0
            assert lib.tmf_snet_algo_flags() == word | bits
            assert saved(0) == saved(word | bits)                           # the process option reaches a call without a word ...
            assert saved(word) == saved(word | RC1 | RBN) + up256(4 * 8 * 48 ** 3 * 32) + up256(8 * 48 ** 3 * 32) + \
                up256(4 * 8 * 24 ** 3 * 64) + up256(4 * 8 * 12 ** 3 * 128)   # ... and not one that carries its own
        assert lib.tmf_set_option(b"pool_recompute", 4) != 0
    finally:
        lib.tmf_set_option(b"pool_recompute", 0)
    assert lib.tmf_snet_algo_flags() == word == ops.snet_algo_flags()
    assert ops.snet_algo_flags(dict(pool_recompute=1)) == word | RC1 | RBN
    assert ops.snet_algo_flags(dict(pool_recompute=2)) == word | RC1 and ops.snet_algo_flags(dict(pool_recompute=3)) == word | RBN
    with pytest.raises(ValueError):
        ops.snet_algo_flags(dict(pool_recompute=5))


def _first_max(y):
    """(index, has_tie) of the first maximum over the last axis (8 window voxels in torch scan order), on the CPU."""
    m = y.max(-1, keepdim=True).values
    hit = y == m
    return hit.float().argmax(-1), hit.sum(-1) > 1           # argmax: the first of equal values


def _windows(t):
    """(B, D, H, W, C) -> (B, D/2, H/2, W/2, C, 8): the full 2x2x2 windows, k = 4 d + 2 h + w (floor mode)."""
    B, D, H, W, C = t.shape
    t = t[:, :D // 2 * 2, :H // 2 * 2, :W // 2 * 2]
    t = t.reshape(B, D // 2, 2, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 7, 2, 4, 6)
    return t.reshape(B, D // 2, H // 2, W // 2, C, 8)


BN_SHAPES = [(8, 48, 48, 48), (2, 24, 24, 24), (2, 45, 54, 45), (2, 22, 27, 22)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "negative_gamma", "ties"])
@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("shape", BN_SHAPES)
def test_bn_reduce_from_saved_routing_is_bit_identical(shape, C, kind):
    """bn_bwd_reduce_kernel reading (z_sel, dout) against the pass that streams all of z: `partial` torch.equal; the pooled output
    with and without the extra output torch.equal.  negative_gamma: half of the channels have scale < 0 (the maximum of y is the
    minimum of z); ties: integer-valued z from {-1, 0, 1} with constant planes, scale a power of two and an integer shift, so
    that y is exact and almost every window has several equal maxima (asserted on the CPU, where z_sel is checked too)."""
    from transmf_ad_amd import _lib, ops
    B, D, H, W = shape
    g = torch.Generator().manual_seed(1000 * C + D + len(kind))
    if kind == "ties":
        z = torch.randint(-1, 2, (B, D, H, W, C), generator=g).float()
        z[:, D // 4:D // 2] = 1.0                                            # constant windows
        scale = torch.where(torch.arange(C) % 3 == 0, -0.5, 0.25)
        shift = torch.randint(-1, 2, (C,), generator=g).float()
    else:
        z = torch.randn((B, D, H, W, C), generator=g)
        scale = torch.rand(C, generator=g) + 0.5
        if kind == "negative_gamma":
            scale = torch.where(torch.arange(C) % 2 == 0, -scale, scale)
        shift = torch.randn(C, generator=g) * 0.3
    mean, invstd = torch.randn(C, generator=g) * 0.1, torch.rand(C, generator=g) + 0.5
    OD, OH, OW = D // 2, H // 2, W // 2
    dout = torch.randn((B, OD, OH, OW, C), generator=g)
    small = B * D * H * W * C <= 2 * 24 ** 3 * 128 or kind == "ties" and B * D * H * W <= 2 * 45 * 54 * 45
    if small:
        y = _windows(z) * scale.view(1, 1, 1, 1, C, 1) + shift.view(1, 1, 1, 1, C, 1)
        arg, tie = _first_max(y)
        if kind == "ties":
            assert tie.float().mean().item() > 0.5, "the tie case has no ties"
    zg, dg = z.to(DEV), dout.to(DEV)
    sc, sh, mu, is_ = (t.to(DEV) for t in (scale, shift, mean, invstd))
    nblk = _lib.query("tmf_bn_act_pool_bwd_blocks", B, D, H, W, C, 1)
    out0, out1 = torch.full_like(dg, float("nan")), torch.full_like(dg, float("nan"))
    zsel = torch.full_like(dg, float("nan"))
    _lib.call("tmf_bn_act_pool_fwd_t", zg.data_ptr(), sc.data_ptr(), sh.data_ptr(), out0.data_ptr(), B, D, H, W, C, 1, 0.01, 0, ops._stream())
    _lib.call("tmf_bn_act_pool_fwd_route", zg.data_ptr(), sc.data_ptr(), sh.data_ptr(), out1.data_ptr(), zsel.data_ptr(), B, D, H, W, C,
              0.01, ops._stream())
    p0, p1 = torch.full((nblk, 2, C), float("nan"), device=DEV), torch.full((nblk, 2, C), float("nan"), device=DEV)
    _lib.call("tmf_bn_act_pool_bwd_reduce_t", zg.data_ptr(), dg.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), is_.data_ptr(),
              p0.data_ptr(), B, D, H, W, C, 1, 0.01, 0, ops._stream())
    _lib.call("tmf_bn_act_pool_bwd_reduce_route", zsel.data_ptr(), dg.data_ptr(), sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
              is_.data_ptr(), p1.data_ptr(), B, D, H, W, C, 0.01, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(out0, out1) and not torch.isnan(out1).any()
    assert not torch.isnan(p0).any() and torch.equal(p0, p1)
    if small and kind == "ties":                                             # exact arithmetic: z_sel is z at the first maximum of y
        ref = _windows(z).gather(-1, arg.unsqueeze(-1)).squeeze(-1)
        assert torch.equal(zsel.cpu(), ref)


C1_SHAPES = [(8, 96, 96, 96, 32), (2, 91, 109, 91, 32), (3, 8, 10, 33, 16), (1, 9, 13, 35, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 0])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("shape", C1_SHAPES)
def test_first_block_backward_from_saved_routing_is_bit_identical(shape, ties, split):
    """tmf_c1_bn_pool_fwd_route + tmf_c1_bwd_fused_route against tmf_c1_bn_pool_fwd + tmf_c1_bwd_fused, in both arithmetic forms
    of z ("c1_split" 1 / 0): pooled output, dw, dgamma, dbeta torch.equal.  ties: a volume and taps from {-1, 0, 1} with a constant
    region, scale +-2^-k and integer shifts — z and y are exact small integers / dyadics, so that most windows have several equal
    maxima with DIFFERENT neighbourhoods (the index matters for D); there z_sel and arg are also checked against torch on the CPU."""
    from transmf_ad_amd import _lib, ops
    B, D, H, W, C = shape
    g = torch.Generator().manual_seed(7 * D + W + C + int(ties))
    if ties:
        x = torch.randint(-1, 2, (B, D, H, W), generator=g).float()
        x[:, D // 3:D // 3 + 3, :, W // 2:] = 1.0                            # a constant region
        w = torch.randint(-1, 2, (C, 1, 3, 3, 3), generator=g).float()
    else:
        x = torch.randn((B, D, H, W), generator=g)
        w = torch.randn((C, 1, 3, 3, 3), generator=g) * 0.2
    OD, OH, OW = D // 2, H // 2, W // 2
    go = torch.randn((B, OD, OH, OW, C), generator=g).to(DEV)
    xg = x.to(DEV)
    wp = ops.pack_weight(w.to(DEV)).view(27, C)
    gbytes = _lib.query("tmf_c1_gram_bytes", B, D, H, W, C)
    assert gbytes > 0
    part = torch.empty((2, 2, C), device=DEV)
    gram = torch.empty(gbytes // 8, device=DEV, dtype=torch.float64)
    gamma = (torch.rand(C, generator=g) + 0.5).to(DEV)
    beta = (torch.randn(C, generator=g) * 0.2).to(DEV)
    mean, invstd, scale, shift = (torch.empty(C, device=DEV) for _ in range(4))
    wsb = _lib.query("tmf_c1_bwd_fused_workspace_bytes", B, D, H, W, C)
    res = {}
    _lib.call("tmf_set_option", b"c1_split", split)
    try:
        _lib.call("tmf_c1_stats_g", xg.data_ptr(), wp.data_ptr(), part.data_ptr(), gram.data_ptr(), gbytes, B, D, H, W, C, ops._stream())
        _lib.call("tmf_bn_finalize", part.data_ptr(), 2, C, float(B * D * H * W), gamma.data_ptr(), beta.data_ptr(), None, None, None,
                  0.1, 1e-5, mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), ops._stream())
        if ties:
            scale.copy_(torch.where(torch.arange(C) % 3 == 0, -0.5, 0.25))
            shift.copy_(torch.randint(-1, 2, (C,), generator=g).float())
        for route in (True, False, True):
            pooled = torch.full((B, OD, OH, OW, C), float("nan"), device=DEV)
            zsel = torch.full((B, OD, OH, OW, C), float("nan"), device=DEV)
            arg = torch.full((B, OD, OH, OW, C), 255, device=DEV, dtype=torch.uint8)
            dw = torch.full((C, 1, 3, 3, 3), float("nan"), device=DEV)
            dgam, dbet = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
            ws = torch.empty(wsb, device=DEV, dtype=torch.uint8)
            head = (xg.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr())
            if route:
                _lib.call("tmf_c1_bn_pool_fwd_route", *head, pooled.data_ptr(), zsel.data_ptr(), arg.data_ptr(), B, D, H, W, C, 0.01,
                          ops._stream())
                _lib.call("tmf_c1_bwd_fused_route", *head, mean.data_ptr(), invstd.data_ptr(), go.data_ptr(), zsel.data_ptr(), arg.data_ptr(),
                          gram.data_ptr(), dw.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr(), wsb, B, D, H, W, C, 0.01, 1,
                          ops._stream())
            else:
                _lib.call("tmf_c1_bn_pool_fwd", *head, pooled.data_ptr(), B, D, H, W, C, 0.01, ops._stream())
                _lib.call("tmf_c1_bwd_fused", *head, mean.data_ptr(), invstd.data_ptr(), go.data_ptr(), gram.data_ptr(), dw.data_ptr(),
                          dgam.data_ptr(), dbet.data_ptr(), ws.data_ptr(), wsb, B, D, H, W, C, 0.01, 1, ops._stream())
            torch.cuda.synchronize()
            res.setdefault(route, []).append((pooled.cpu(), dw.cpu(), dgam.cpu(), dbet.cpu(), zsel.cpu(), arg.cpu()))
    finally:
        _lib.call("tmf_set_option", b"c1_split", 1)
    a, a2 = res[True]
    b = res[False][0]
    for u in a[:4]:
        assert not torch.isnan(u).any()
    assert all(torch.equal(u, v) for u, v in zip(a, a2))                    # run to run
    for name, u, v in zip(("pooled", "dw", "dgamma", "dbeta"), a[:4], b[:4]):
        assert torch.equal(u, v), name
    assert int(a[5].max()) <= 7
    if ties and B * D * H * W <= 2 * 91 * 109 * 91:                         # (the CPU evaluation of the largest volume is left out)
        z = F.conv3d(x.unsqueeze(1), w, None, 1, 1).permute(0, 2, 3, 4, 1).contiguous()      # exact: small integers
        sc, sh = scale.cpu(), shift.cpu()
        y = _windows(z) * sc.view(1, 1, 1, 1, C, 1) + sh.view(1, 1, 1, 1, C, 1)
        ref_arg, tie = _first_max(y)
        # evaluated on the CPU when the inputs were chosen: 19-27 % of the windows of these volumes have several equal maxima
        assert tie.float().mean().item() > 0.1, "the tie case has too few ties"
        assert torch.equal(a[5].long(), ref_arg)
        assert torch.equal(a[4], _windows(z).gather(-1, ref_arg.unsqueeze(-1)).squeeze(-1))


@pytest.mark.gpu
def test_encoder_step_is_bit_identical_with_and_without_saved_routing():
    """The one-call encoder (ops.SNetTrain through sNet) forward + backward with "pool_recompute" 0, 1, 2, 3 — a module's own
    choice, all in one process: output and every parameter gradient torch.equal."""
    import transmf_ad_amd as T
    torch.manual_seed(3)
    net = T.networks.sNet(32).to(DEV).train()
    vol = torch.randn((2, 1, 32, 40, 48), device=DEV)
    res = []
    for rec in (0, 1, 2, 3, 0):
        net.set_algorithm(pool_recompute=rec)
        net.zero_grad(set_to_none=True)
        out = net(vol)
        out.square().sum().backward()
        torch.cuda.synchronize()
        res.append([out.detach().cpu()] + [p.grad.cpu().clone() for p in net.parameters()])
    for r in res[1:]:
        assert len(r) == len(res[0]) and all(torch.equal(u, v) for u, v in zip(res[0], r))
