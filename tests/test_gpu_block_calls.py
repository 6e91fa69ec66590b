"""The block-by-block encoder path (ops.conv_bn_act_pool -> ConvBnActPool / Conv1BnPool / conv_bn_act_pool_eval_fused) by the
library entries it calls (MI355X): one forward and one backward per route, the names of every _lib.call and _lib.query in order
against lists written out from the code, and the shapes and dtypes of the output and of every gradient.  The values are the
business of tests/test_gpu_kernels.py and tests/test_gpu_input_grad.py; this pins the launches, so that a route cannot gain,
lose or reorder one unnoticed."""
import contextlib

import pytest
import torch

from _conv_util import _lib, _ops, _rand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, B16 = torch.float32, torch.bfloat16

# ConvBnActPool: what follows the weight packing in forward, and what precedes the convolutions in backward
_BN_FWD = ["tmf_bn_finalize", "tmf_bn_act_pool_fwd_t"]
_BN_BWD = ["tmf_bn_act_pool_bwd_blocks", "tmf_bn_act_pool_bwd_reduce_t", "tmf_bn_bwd_finalize", "tmf_bn_act_pool_bwd_apply_t"]
_ALGO = "tmf_conv_block_algo"
_DIRECT_FWD = ["tmf_conv3d_stat_blocks", "tmf_conv3d_fwd"]
_DIRECT_WGRAD = ["tmf_conv3d_wgrad_workspace_bytes", "tmf_conv3d_wgrad"]
_WINO_PACK = ["tmf_conv3d_wino_weight_bytes", "tmf_pack_conv_weights_wino"]
_WINO_FWD = ["tmf_conv3d_wino_stat_blocks", "tmf_conv3d_fwd_wino"]
_WINO_WGRAD = ["tmf_conv3d_wgrad_wino_workspace_bytes", "tmf_conv3d_wgrad_wino"]
_BF16_FWD = [_ALGO, "tmf_pack_conv_weights_bf16", "tmf_conv3d_bf16_stat_blocks", "tmf_conv3d_fwd_bf16_t"] + _BN_FWD
_BF16_BWD = _BN_BWD + ["tmf_conv3d_wgrad_bf16_workspace_bytes", "tmf_conv3d_wgrad_bf16_t", "tmf_conv3d_fwd_bf16_t"]
_C1_GRAM_FWD = ["tmf_c1_blocks", "tmf_c1_gram_bytes", "tmf_c1_stats_g", "tmf_bn_finalize", "tmf_c1_bn_pool_fwd"]
_C1_TWO_PASS_BWD = ["tmf_c1_blocks", "tmf_c1_bwd_reduce", "tmf_bn_bwd_finalize", "tmf_c1_bwd_wgrad_workspace_bytes",
                    "tmf_c1_bwd_wgrad"]

# id: (settings, entries of the forward, entries of the backward).  Settings (defaults: fp32 precision and storage, conv_wino 0,
# c1_gram 1, cin 8, cout 16, k 3, training, a graph, x wants a gradient and is fp32, an fp32 output); B = 1, 8 x 8 x 8, max pool.
# tmf_conv3d_wino_ok wants cin % 8 == 0 and cout % 32 == 0 and tmf_conv3d_wgrad_wino_ok both % 32 == 0: (8, 16) is refused in
# every direction, (32, 32) is the smallest pair that takes the Winograd form in all three; (8, 32) takes it in the forward only
# and (32, 8) in the data gradient only — there the direct packer still runs first.
CASES = {
    "fp32-direct": (dict(),
                    [_ALGO, "tmf_pack_conv_weights"] + _DIRECT_FWD + _BN_FWD,
                    _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd"]),
    "fp32-winograd": (dict(wino=3, cin=32, cout=32),
                      [_ALGO] + _WINO_PACK + _WINO_FWD + _BN_FWD,
                      _BN_BWD + _WINO_WGRAD + ["tmf_conv3d_fwd_wino"]),
    "fp32-winograd-forward-only": (dict(wino=3, cin=8, cout=32),
                                   [_ALGO, "tmf_pack_conv_weights"] + _WINO_PACK + _WINO_FWD + _BN_FWD,
                                   _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd"]),
    "fp32-winograd-dgrad-only": (dict(wino=3, cin=32, cout=8),
                                 [_ALGO, "tmf_pack_conv_weights"] + _WINO_PACK + _DIRECT_FWD + _BN_FWD,
                                 _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd_wino"]),
    "bf16": (dict(conv="bf16"), _BF16_FWD, _BF16_BWD),
    # (the dispatcher asks bf16_conv_capable first: one more query of the rule)
    "bf16-storage": (dict(conv="bf16", storage="bf16", x16=True, out_bf16=True), [_ALGO] + _BF16_FWD, _BF16_BWD),
    "fp32x": (dict(conv="fp32x"),
              [_ALGO, "tmf_pack_conv_weights_split3", "tmf_conv3d_split_stat_blocks", "tmf_conv3d_fwd_split"] + _BN_FWD,
              _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd_split"]),
    "c1-gram": (dict(cin=1, cout=8, xgrad=False),
                _C1_GRAM_FWD,
                ["tmf_c1_bwd_fused_workspace_bytes", "tmf_c1_bwd_fused"]),
    "c1-two-pass": (dict(cin=1, cout=8, xgrad=False, c1_gram=0),
                    ["tmf_c1_blocks", "tmf_c1_gram_bytes", "tmf_c1_stats", "tmf_bn_finalize", "tmf_c1_bn_pool_fwd"],
                    _C1_TWO_PASS_BWD),
    "c1-input-gradient": (dict(cin=1, cout=8),
                          _C1_GRAM_FWD,
                          ["tmf_c1_bwd_fused_workspace_bytes", "tmf_c1_bwd_fused_coef", "tmf_c1_bwd_dgrad_workspace_bytes",
                           "tmf_c1_bwd_dgrad"]),
    "c1-eval-graph": (dict(cin=1, cout=8, xgrad=False, train=False),
                      ["tmf_bn_eval_coeffs", "tmf_c1_bn_pool_fwd"],
                      _C1_TWO_PASS_BWD),
    "k1": (dict(k=1),
           [_ALGO, "tmf_pack_conv_weights"] + _DIRECT_FWD + _BN_FWD,
           _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd"]),
    "no-input-gradient": (dict(xgrad=False),
                          [_ALGO, "tmf_pack_conv_weights"] + _DIRECT_FWD + _BN_FWD,
                          _BN_BWD + _DIRECT_WGRAD),
    "no-input-gradient-winograd": (dict(wino=3, cin=32, cout=32, xgrad=False),
                                   [_ALGO] + _WINO_PACK + _WINO_FWD + _BN_FWD,
                                   _BN_BWD + _WINO_WGRAD),
    "eval-graph": (dict(train=False),
                   [_ALGO, "tmf_pack_conv_weights", "tmf_conv3d_fwd", "tmf_bn_eval_coeffs", "tmf_bn_act_pool_fwd_t"],
                   _BN_BWD + _DIRECT_WGRAD + ["tmf_conv3d_fwd"]),
    "eval-fused-direct": (dict(train=False, graph=False),
                          ["tmf_bn_eval_coeffs", _ALGO, "tmf_conv3d_fwd_affine"], None),
    "eval-fused-winograd": (dict(wino=3, cin=32, cout=32, train=False, graph=False),
                            ["tmf_bn_eval_coeffs", _ALGO] + _WINO_PACK + ["tmf_conv3d_fwd_wino_affine"], None),
}


@contextlib.contextmanager
def _recorded(entries):
    """Every _lib.call and _lib.query inside the block, appended to `entries` as (name, arguments), in order."""
    lib = _lib()
    real = lib.call, lib.query
    lib.call = lambda name, *a: (entries.append((name, a)), real[0](name, *a))[1]
    lib.query = lambda name, *a: (entries.append((name, a)), real[1](name, *a))[1]
    try:
        yield
    finally:
        lib.call, lib.query = real


def _names(entries):
    return [name for name, _ in entries]


@pytest.mark.parametrize("case", list(CASES))
def test_block_route_calls_the_library_as_written(case, monkeypatch):
    ops, lib = _ops(), _lib()
    cfg, want_fwd, want_bwd = CASES[case]
    cin, cout, k = cfg.get("cin", 8), cfg.get("cout", 16), cfg.get("k", 3)
    train, graph, xgrad = cfg.get("train", True), cfg.get("graph", True), cfg.get("xgrad", True)
    out_bf16, wino = cfg.get("out_bf16", False), cfg.get("wino", 0)
    precision = ops.make_precision(cfg.get("conv", "fp32"), cfg.get("storage", "fp32"))
    x = _rand(1, 8, 8, 8, cin, seed=1).to(DEV)
    x = (x.bfloat16() if cfg.get("x16") else x).requires_grad_(graph and xgrad)
    w = _rand(cout, cin, k, k, k, seed=2, scale=(cin * k ** 3) ** -0.5).to(DEV).requires_grad_(graph)
    b, g, be = (_rand(cout, seed=3 + i, scale=0.1).to(DEV).requires_grad_(graph) for i in range(3))
    rm, rv = _rand(cout, seed=6, scale=0.1).to(DEV), (1 + _rand(cout, seed=7, scale=0.1).abs()).to(DEV)
    monkeypatch.setattr(ops, "FUSE_EVAL_BLOCKS", True)
    wino_before = ops.conv_wino_mode()
    lib.call("tmf_set_option", b"conv_wino", wino)
    lib.call("tmf_set_option", b"c1_gram", cfg.get("c1_gram", 1))
    try:
        if wino == 3 and (cin, cout) == (32, 32):
            assert ops.wino_ok(cin, cout) and ops.wino_ok(cout, cin) and ops.wgrad_wino_ok(cin, cout)
            assert not (ops.wino_ok(8, 16) or ops.wino_ok(16, 8) or ops.wgrad_wino_ok(8, 16))
        fwd, bwd = [], []
        with _recorded(fwd), (contextlib.nullcontext() if graph else torch.no_grad()):
            out = ops.conv_bn_act_pool(x, w, b, g, be, rm, rv, train, pool="max", out_bf16=out_bf16, precision=precision)
        assert _names(fwd) == want_fwd
        assert out.shape == (1, 4, 4, 4, cout) and out.dtype == (B16 if out_bf16 else F32)
        if not graph:
            assert not out.requires_grad
            return
        if not xgrad:                        # no data-gradient form may be packed: the packers' third pointer
            packs = [a for name, a in fwd if name.startswith("tmf_pack_conv_weights")]
            assert [a[2] for a in packs] == [None] * len(packs)
        leaves = ([x] if xgrad else []) + [w, b, g, be]
        with _recorded(bwd):
            grads = torch.autograd.grad(out, leaves, _rand(*out.shape, seed=8).to(DEV).to(out.dtype))
        torch.cuda.synchronize()
        assert _names(bwd) == want_bwd
        assert [(tuple(t.shape), t.dtype) for t in grads] == [(tuple(t.shape), t.dtype) for t in leaves]
        assert all(bool(torch.isfinite(t.float()).all()) for t in (out,) + tuple(grads))
    finally:
        lib.call("tmf_set_option", b"conv_wino", wino_before)
        lib.call("tmf_set_option", b"c1_gram", 1)
