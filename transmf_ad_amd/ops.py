"""torch.autograd.Functions over the C ABI of libtmf_hip.so.

PyTorch is plumbing here (device memory, the current HIP stream, autograd graph);
every numeric step of the hot path is a hand-written gfx950 kernel.  All tensors are
fp32, contiguous, on a HIP device; activations are channels-last (B, D, H, W, C).
"""
from __future__ import annotations

import collections
import ctypes
import math
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib

_f32 = torch.float32


def _stream():
    """Raw hipStream_t of torch's current stream (the private fast path: the public current_stream() builds a
    Stream object and costs ~10 us, ~0.7 ms per train step over ~75 calls)."""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _chk(t: torch.Tensor, name: str, allow_bf16: bool = False) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.TmfError(
            f"{name} is on {t.device}: transmf_ad_amd runs only on a HIP device (MI355X); there is no CPU fallback")
    if t.device.index != torch._C._cuda_getDevice():
        # the kernels are launched on the CURRENT device's current stream (_stream): pointers of another GPU there
        # would fault or race.  The module forwards install the guard themselves (networks.on_device_of).
        raise _lib.TmfError(
            f"{name} is on {t.device} but the current HIP device is cuda:{torch._C._cuda_getDevice()}: "
            f"call under `with torch.cuda.device({t.device.index}):`")
    if t.dtype != _f32 and not (allow_bf16 and t.dtype == torch.bfloat16):
        raise _lib.TmfError(f"{name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


# --------------------------------------------------------------------------------------
# conv3d (+ folded bias) -> BatchNorm3d -> LeakyReLU -> pool      (networks.py:21-53)
# --------------------------------------------------------------------------------------

def pack_weight(weight: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, k, k, k) reference layout -> tap-major [k^3][Cin][Cout]."""
    return weight.permute(2, 3, 4, 1, 0).contiguous()


def pack_weight_dgrad(weight: torch.Tensor) -> torch.Tensor:
    """Weights of the data-gradient convolution: w'[26-t][co][ci] = w[t][ci][co]."""
    return weight.flip(2, 3, 4).permute(2, 3, 4, 0, 1).contiguous()


def pack_weights_both(weight: torch.Tensor, want_dgrad: bool, want_fwd: bool = True):
    """Forward layout [k^3][Cin][Cout] and (optionally) data-gradient layout [k^3][Cout][Cin] in one launch."""
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    if not (want_fwd or want_dgrad):
        return None, None
    wf = torch.empty((k ** 3, cin, cout), device=weight.device, dtype=_f32) if want_fwd else None
    wd = torch.empty((k ** 3, cout, cin), device=weight.device, dtype=_f32) if want_dgrad else None
    _lib.call("tmf_pack_conv_weights", weight.data_ptr(), _ptr(wf), _ptr(wd), cout, cin, k ** 3, _stream())
    return wf, wd


def unpack_wgrad(dw: torch.Tensor, cout: int, cin: int, k: int) -> torch.Tensor:
    """tap-major [k^3][Cin][Cout] gradient -> reference (Cout, Cin, k, k, k)."""
    return dw.view(k, k, k, cin, cout).permute(4, 3, 0, 1, 2).contiguous()


# Precision of the convolution products is a property of the MODULE that runs them (sNet.set_precision / model.set_precision
# -> sNet.tmf_precision), handed down explicitly to every op and into tmf_snet_desc.precision / .storage_bf16; two models with
# different precisions live side by side in one process.  The two setters below only change the DEFAULT that modules
# without a setting of their own follow (the round-1 API: bench.py --precision, the parity tests).
_PRECISION = "fp32"
_ACT16 = False
_b16 = torch.bfloat16
_CONV_MODES = ("fp32", "fp32x", "bf16")


def set_conv_precision(precision: str) -> None:
    """Process DEFAULT for modules that have no precision of their own: "fp32" (exact-fp32 MFMA everywhere); "bf16": the
    forward, data-gradient and weight-gradient 3x3x3 convolutions round their operands to bf16 and run on the bf16 matrix
    cores with fp32 accumulation (tensors stay fp32); "fp32x": fp32-accurate 3-way bf16 split (six partial products)."""
    global _PRECISION
    if precision not in _CONV_MODES:
        raise ValueError(precision)
    _PRECISION = precision


def get_conv_precision() -> str:
    return _PRECISION


def set_activation_storage(dtype: str) -> None:
    """Process DEFAULT: "fp32" or "bf16" — with conv precision "bf16", keep the sNet activations BETWEEN the conv blocks
    (raw conv outputs z, block outputs, and their gradients) as bf16 tensors — BASELINE configs[2] "bf16 storage".  The
    network input, the BatchNorm statistics / parameters, the 1x1x1 layer and everything after the encoders stay fp32."""
    global _ACT16
    if dtype not in ("fp32", "bf16"):
        raise ValueError(dtype)
    _ACT16 = dtype == "bf16"


def make_precision(conv: str = "fp32", storage: str = "fp32"):
    """(conv mode, bf16 activation storage) as the ops take it; storage "bf16" only has an effect with conv "bf16"."""
    if conv not in _CONV_MODES or storage not in ("fp32", "bf16"):
        raise ValueError((conv, storage))
    return (conv, storage == "bf16" and conv == "bf16")


def resolve_precision(precision=None):
    """None -> the process default; else a make_precision() pair."""
    if precision is None:
        return (_PRECISION, _ACT16 and _PRECISION == "bf16")
    return precision


def activation_storage_bf16(precision=None) -> bool:
    return resolve_precision(precision)[1]


def conv_block_algo(mode: str, cin: int, cout: int, k: int):
    """(forward, data gradient, weight gradient) kernel family, each a _lib.CONV_* code, of one encoder block in conv precision
    `mode` under the options of the moment: the library's one rule (tmf_conv_block_algo), the same the whole-encoder path
    plans with — so the block-by-block path and the one-call path run the same kernels."""
    a = _lib.query("tmf_conv_block_algo", _lib.PRECISION[mode], cin, cout, k)
    return a & 15, (a >> 4) & 15, (a >> 8) & 15


def bf16_conv_capable(cin: int, k: int) -> bool:
    """the 3x3x3 bf16 matrix-core kernels need 8-channel input groups (the forward's family does not depend on cout)"""
    return conv_block_algo("bf16", cin, cin, k)[0] == _lib.CONV_BF16


def pack_weight_bf16(weight: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, 3,3,3) -> bf16 [27][Cout][Cin] (B operand rows: output channel, K = input channel contiguous)."""
    return weight.permute(2, 3, 4, 0, 1).contiguous().to(torch.bfloat16)


def pack_weights_both_bf16(weight: torch.Tensor, want_dgrad: bool):
    """pack_weight_bf16 and (optionally) pack_weight_dgrad_bf16 of one weight tensor in ONE launch."""
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wf = torch.empty((k ** 3, cout, cin), device=weight.device, dtype=torch.bfloat16)
    wd = torch.empty((k ** 3, cin, cout), device=weight.device, dtype=torch.bfloat16) if want_dgrad else None
    _lib.call("tmf_pack_conv_weights_bf16", weight.data_ptr(), wf.data_ptr(), _ptr(wd), cout, cin, k ** 3, _stream())
    return wf, wd


def pack_weight_dgrad_bf16(weight: torch.Tensor) -> torch.Tensor:
    """Data-gradient weights, bf16 [27][Cin][Cout]: w'[26-t][ci][co] = w[co][ci][t]."""
    return weight.flip(2, 3, 4).permute(2, 3, 4, 1, 0).contiguous().to(torch.bfloat16)


def split3_bf16(t: torch.Tensor) -> torch.Tensor:
    """Exact decomposition t = hi + mid + lo into three bf16 tensors, stacked on a new leading axis."""
    hi = t.to(torch.bfloat16)
    r1 = t - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    return torch.stack([hi, mid, lo]).contiguous()


def pack_weights_split3(weight: torch.Tensor, want_dgrad: bool):
    """split3_bf16 of the forward layout [27][cout][cin] and (optionally) of the data-gradient layout [27][cin][cout]
    (flipped taps) of one (cout, cin, 3, 3, 3) weight tensor in ONE launch: (3, 27, cout, cin), (3, 27, cin, cout) bf16."""
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    wf = torch.empty((3, k ** 3, cout, cin), device=weight.device, dtype=torch.bfloat16)
    wd = torch.empty((3, k ** 3, cin, cout), device=weight.device, dtype=torch.bfloat16) if want_dgrad else None
    _lib.call("tmf_pack_conv_weights_split3", weight.data_ptr(), wf.data_ptr(), _ptr(wd), cout, cin, k ** 3, _stream())
    return wf, wd


def conv_wino_mode() -> int:
    """tmf_set_option("conv_wino", v) / TMF_CONV_WINO: 0 = direct kernels, 1 = Winograd data gradients, 2 = Winograd forward
    and data gradients (layers with tmf_conv3d_wino_ok), 3 (default) = the weight gradients as well (tmf_conv3d_wgrad_wino_ok)."""
    return _lib.query("tmf_conv_wino_mode")


def wino_ok(cin: int, cout: int) -> bool:
    return bool(_lib.query("tmf_conv3d_wino_ok", cin, cout))


def pack_weights_wino(weight: torch.Tensor, want_fwd: bool = True, want_dgrad: bool = False):
    """Winograd-transformed weights of one (cout, cin, 3, 3, 3) tensor in ONE launch: u_fwd [64][cin/8][2][cout][4] and
    u_dgrad [64][cout/8][2][cin][4] (flipped filter, channel roles swapped); None for a form that is not asked for."""
    cout, cin = weight.shape[0], weight.shape[1]
    # (the library's buffer is the fp32 tensor plus, behind it, its exact 3-way bf16 split for conv3d_winox.hip: the returned
    #  tensors are views of the fp32 part, the storage carries both)
    n = 64 * cin * cout
    nb = _lib.query("tmf_conv3d_wino_weight_bytes", cin, cout) // 4
    uf = torch.empty((nb,), device=weight.device, dtype=_f32)[:n].view(64, cin // 8, 2, cout, 4) if want_fwd else None
    ud = torch.empty((nb,), device=weight.device, dtype=_f32)[:n].view(64, cout // 8, 2, cin, 4) if want_dgrad else None
    _lib.call("tmf_pack_conv_weights_wino", weight.data_ptr(), _ptr(uf), _ptr(ud), cout, cin, _stream())
    return uf, ud


def wino_p_mode() -> bool:
    """True when the Winograd entries run their persistent one-wave-per-SIMD kernels (the default; TMF_WINO_P=0 or
    tmf_set_option("wino_p", 0): the two-waves-per-SIMD kernels of round 4)."""
    return bool(_lib.query("tmf_wino_p_mode"))


def wgrad_wino_ok(cin: int, cout: int) -> bool:
    return bool(_lib.query("tmf_conv3d_wgrad_wino_ok", cin, cout))


# One row per kernel family of conv_block_algo.  pack(weight, want_fwd, want_dgrad) -> (forward form, data-gradient form) is the
# family's one-launch packer (the data gradient is the forward entry on the other form with the channel roles swapped; the
# bf16 and split packers always write the forward form); w16: the packed forms are bf16; io16: the entries read and write
# fp32 or bf16 activations and take an io word that says which (every other family: fp32 only).  An entry stands with the
# scalars it takes behind B, D, H, W; a weight gradient's workspace query takes the same ones.  affine: the forward with the
# eval-mode BatchNorm, LeakyReLU and pool in its epilogue (conv_bn_act_pool_eval_fused).
_ConvFamily = collections.namedtuple("_ConvFamily", "pack w16 io16 fwd blocks affine wgrad wbytes", defaults=(None, None, None))
_cck = lambda cin, cout, k: (cin, cout, k)
_cc = lambda cin, cout, k: (cin, cout)
_co = lambda cin, cout, k: (cout,)
_none = lambda cin, cout, k: ()
_pack_direct = lambda w, f, d: pack_weights_both(w, d, want_fwd=f)
_DIRECT = _ConvFamily(_pack_direct, False, False, ("tmf_conv3d_fwd", _cck), ("tmf_conv3d_stat_blocks", _cck),
                      "tmf_conv3d_fwd_affine", ("tmf_conv3d_wgrad", _cck), "tmf_conv3d_wgrad_workspace_bytes")
_DIRECT_C1 = _ConvFamily(_pack_direct, False, False, ("tmf_conv3d_c1_fwd", _co), ("tmf_conv3d_c1_stat_blocks", _co),
                         None, ("tmf_conv3d_c1_wgrad", _co), "tmf_conv3d_c1_wgrad_workspace_bytes")     # cin == 1, k == 3
_WINO = _ConvFamily(pack_weights_wino, False, False, ("tmf_conv3d_fwd_wino", _cc), ("tmf_conv3d_wino_stat_blocks", _none),
                    "tmf_conv3d_fwd_wino_affine", ("tmf_conv3d_wgrad_wino", _cc), "tmf_conv3d_wgrad_wino_workspace_bytes")
_BF16 = _ConvFamily(lambda w, f, d: pack_weights_both_bf16(w, d), True, True, ("tmf_conv3d_fwd_bf16_t", _cc),
                    ("tmf_conv3d_bf16_stat_blocks", _none), None, ("tmf_conv3d_wgrad_bf16_t", _cc),
                    "tmf_conv3d_wgrad_bf16_workspace_bytes")
_SPLIT = _ConvFamily(lambda w, f, d: pack_weights_split3(w, d), True, False, ("tmf_conv3d_fwd_split", _cc),
                     ("tmf_conv3d_split_stat_blocks", _none))                                # (no weight gradient of its own)
_CONV = {_lib.CONV_DIRECT: _DIRECT, _lib.CONV_WINO: _WINO, _lib.CONV_BF16: _BF16, _lib.CONV_SPLIT: _SPLIT}


def _conv_variant(fam, cin, k):
    return _DIRECT_C1 if (fam is _DIRECT and cin == 1 and k == 3) else fam


def _conv_forward(fam, x, w, cin, cout, k, want_stats, out_bf16=False):
    """z = conv(x, w) on NDHWC x by the entries of one _ConvFamily, w its packed forward form (or, for a data gradient, its
    dgrad form with cin and cout swapped); returns (z, stat_partial or None, nblk)."""
    fam = _conv_variant(fam, cin, k)
    if out_bf16 and not fam.io16:
        raise _lib.TmfError("only the bf16 convolution kernels write a bf16 tensor")
    B, D, H, W = x.shape[:4]
    z = torch.empty((B, D, H, W, cout), device=x.device, dtype=_b16 if out_bf16 else _f32)
    part, nblk = None, 0
    if want_stats:
        nblk = _lib.query(fam.blocks[0], B, D, H, W, *fam.blocks[1](cin, cout, k))
        part = torch.empty((nblk, 2, cout), device=x.device, dtype=_f32)
    io = ((1 if x.dtype == _b16 else 0) | (2 if out_bf16 else 0),) if fam.io16 else ()
    _lib.call(fam.fwd[0], x.data_ptr(), w.data_ptr(), z.data_ptr(), _ptr(part),
              B, D, H, W, *fam.fwd[1](cin, cout, k), *io, _stream())
    return z, part, nblk


def _conv_wgrad(fam, x, dz, cin, cout, k, reference_layout):
    """weight gradient by the entries of one _ConvFamily: tap-major [k^3][cin][cout], or (reference_layout) nn.Conv3d's
    (cout, cin, k, k, k) written directly by the final reduction."""
    fam = _conv_variant(fam, cin, k)
    if fam.wgrad is None:
        raise _lib.TmfError("this convolution family has no weight-gradient kernel")
    B, D, H, W = x.shape[:4]
    dw = torch.empty((cout, cin, k, k, k) if reference_layout else (k ** 3, cin, cout), device=x.device, dtype=_f32)
    tail = fam.wgrad[1](cin, cout, k)
    nbytes = _lib.query(fam.wbytes, B, D, H, W, *tail)
    ws = torch.empty((max(nbytes, 16) // 4,), device=x.device, dtype=_f32)
    io = ()
    if fam.io16:
        if x.dtype != dz.dtype:                  # mixed storage (not produced by sNet): widen the bf16 side
            x, dz = x.float(), dz.float()
        io = (1 if x.dtype == _b16 else 0,)
    _lib.call(fam.wgrad[0], x.data_ptr(), dz.data_ptr(), dw.data_ptr(), ws.data_ptr(), nbytes,
              B, D, H, W, *tail, *io, int(reference_layout), _stream())
    return dw


def _pack_conv_weights(weight, fam_f, fam_d, want_dgrad):
    """(forward form for fam_f, data-gradient form for fam_d or None), one launch per packer that has a form to write."""
    if fam_d is fam_f or not want_dgrad or fam_f.w16:
        # (a bf16 or split forward whose data gradient is direct, cout % 8 != 0, packs no form for it: backward's pack_weight_dgrad)
        return fam_f.pack(weight, True, want_dgrad and fam_d is fam_f)
    wf = wd = None                                # one direction direct, the other Winograd: the direct packer first
    for fam in (_DIRECT, _WINO):
        f, d = fam.pack(weight, fam is fam_f, fam is fam_d)
        wf, wd = f if fam is fam_f else wf, d if fam is fam_d else wd
    return wf, wd


def conv3d_raw(x, w_packed, cin, cout, ksize, want_stats):
    """z = conv(x, w) on NDHWC x; returns (z, stat_partial or None, nblk)."""
    return _conv_forward(_DIRECT, x, w_packed, cin, cout, ksize, want_stats)


def conv3d_bf16_raw(x, w_bf16, cin, cout, want_stats, out_bf16=False):
    """z = conv3x3x3(bf16(x), w_bf16) with fp32 accumulation; x may be an fp32 or a bf16 tensor, z is fp32 or
    (out_bf16) bf16; returns (z, stat_partial or None, nblk)."""
    return _conv_forward(_BF16, x, w_bf16, cin, cout, 3, want_stats, out_bf16)


def conv3d_split_raw(x, w3, cin, cout, want_stats):
    """fp32-accurate conv on the bf16 matrix cores; w3 = split3_bf16(packed [27][cout][cin] fp32 weights)."""
    return _conv_forward(_SPLIT, x, w3, cin, cout, 3, want_stats)


def conv3d_wino_raw(x, u, cin, cout, want_stats):
    """3x3x3 convolution in the Winograd form F(2x2x2, 3x3x3) (csrc/conv3d_wino.hip); u from pack_weights_wino."""
    return _conv_forward(_WINO, x, u, cin, cout, 3, want_stats)


def conv3d_wgrad(x, dz, cin, cout, ksize, reference_layout=False):
    """weight gradient: tap-major [k^3][cin][cout], or (reference_layout) nn.Conv3d's (cout, cin, k, k, k)."""
    return _conv_wgrad(_DIRECT, x, dz, cin, cout, ksize, reference_layout)


def conv3d_wgrad_bf16(x, dz, cin, cout, reference_layout=False):
    """weight gradient on the bf16 matrix cores (operands rounded to bf16): tap-major [27][cin][cout], or
    (reference_layout) the nn.Conv3d layout (cout, cin, 3, 3, 3) written directly by the final reduction."""
    return _conv_wgrad(_BF16, x, dz, cin, cout, 3, reference_layout)


def conv3d_wgrad_wino(x, dz, cin, cout, reference_layout=False):
    """3x3x3 weight gradient in the Winograd form (csrc/conv3d_wino.hip): tap-major [27][cin][cout] or nn.Conv3d's layout."""
    return _conv_wgrad(_WINO, x, dz, cin, cout, 3, reference_layout)


def _bn_eval_coeffs(gamma, beta, bias, running_mean, running_var, eps, cout, dev):
    """(scale, shift) of eval-mode BatchNorm with the conv bias folded into the shift."""
    scale = torch.empty(cout, device=dev, dtype=_f32)
    shift = torch.empty(cout, device=dev, dtype=_f32)
    _lib.call("tmf_bn_eval_coeffs", gamma.data_ptr(), beta.data_ptr(), _ptr(bias), running_mean.data_ptr(),
              running_var.data_ptr(), float(eps), cout, scale.data_ptr(), shift.data_ptr(), _stream())
    return scale, shift


def _bn_coeffs(training, part, rows, count, gamma, beta, bias, running_mean, running_var, momentum, eps, cout, dev):
    """(mean, invstd, scale, shift) of a block's BatchNorm: in training from the `rows` statistic partials of the conv over
    `count` voxels (and the running statistics move), in eval mode from the running statistics."""
    if not training:
        scale, shift = _bn_eval_coeffs(gamma, beta, bias, running_mean, running_var, eps, cout, dev)
        # xhat = (z + bias - running_mean) * invstd, written as (z - mean) * invstd
        invstd = torch.rsqrt(running_var + eps)
        mean = running_mean - bias if bias is not None else running_mean.clone()
        return mean, invstd, scale, shift
    mean, invstd, scale, shift = (torch.empty(cout, device=dev, dtype=_f32) for _ in range(4))
    _lib.call("tmf_bn_finalize", part.data_ptr(), rows, cout, count,
              gamma.data_ptr(), beta.data_ptr(), _ptr(bias), _ptr(running_mean), _ptr(running_var),
              float(momentum), float(eps), mean.data_ptr(), invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), _stream())
    return mean, invstd, scale, shift


def _bn_bwd_tail(part, nblk, cout, count, training, has_bias, scale, dev):
    """(dgamma, dbeta, coef, dbias) from the nblk partials of a backward-reduce pass; coef = (sum dy, sum dy xhat) / count."""
    dgamma = torch.empty(cout, device=dev, dtype=_f32)
    dbeta = torch.empty(cout, device=dev, dtype=_f32)
    coef = torch.empty((2, cout), device=dev, dtype=_f32)
    _lib.call("tmf_bn_bwd_finalize", part.data_ptr(), nblk, cout, count,
              dgamma.data_ptr(), dbeta.data_ptr(), coef.data_ptr(), _stream())
    if training:
        dbias = torch.zeros(cout, device=dev, dtype=_f32) if has_bias else None
    else:
        coef.zero_()                      # eval-mode BN is affine: dz = scale * dy
        dbias = scale * dbeta if has_bias else None
    return dgamma, dbeta, coef, dbias


class ConvBnActPool(torch.autograd.Function):
    """One sNet block: Conv3d(k, same padding) -> BatchNorm3d -> LeakyReLU -> {none,max,avg} 2x2x2 pool.

    The conv bias is never added to the activations: ahead of BatchNorm it only shifts the
    batch mean, so it is folded into running_mean (train) or into the BN shift (eval).
    Its train-mode gradient is exactly zero in exact arithmetic (the reference returns
    rounding noise there); we return zeros.
    """

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var,
                training, momentum, eps, slope, pool, out_bf16=False, precision=None):
        mode, act16 = resolve_precision(precision)
        x = _chk(x, "x", allow_bf16=True)
        cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
        B, D, H, W, C = x.shape
        if C != cin:
            raise _lib.TmfError(f"conv expects {cin} input channels, got {C}")
        weight = _chk(weight, "weight")
        # the kernel family per direction: the same choice as the whole-encoder path (snet_path.hip make_plan asks the same
        # query), so the two stay bit-identical
        fam_f, fam_d, fam_w = ctx.fam = tuple(_CONV[a] for a in conv_block_algo(mode, cin, cout, k))
        z16 = fam_f.io16 and act16               # raw conv output (and dz) stored as bf16
        if x.dtype == _b16 and not fam_f.io16:
            x = x.float()                         # only the bf16 kernels read bf16 tensors
        if out_bf16 and not z16:
            raise _lib.TmfError("a bf16 block output needs conv precision 'bf16' with bf16 activation storage")
        wf, wd = _pack_conv_weights(weight, fam_f, fam_d, ctx.needs_input_grad[0])      # the dgrad form is kept for backward
        dev = x.device
        s = _stream()
        pc = _lib.pool_code(pool)
        z, part, nblk = _conv_forward(fam_f, x, wf, cin, cout, k, training, z16)
        mean, invstd, scale, shift = _bn_coeffs(training, part, nblk, float(B * D * H * W), gamma, beta, bias,
                                                running_mean, running_var, momentum, eps, cout, dev)
        odt = _b16 if out_bf16 else _f32
        if pc == _lib.POOL_NONE:
            out = torch.empty((B, D, H, W, cout), device=dev, dtype=odt)
        else:
            out = torch.empty((B, D // 2, H // 2, W // 2, cout), device=dev, dtype=odt)
        io = (1 if z16 else 0) | (2 if out_bf16 else 0)
        if out.numel() > 0:
            _lib.call("tmf_bn_act_pool_fwd_t", z.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
                      B, D, H, W, cout, pc, float(slope), io, s)
        ctx.save_for_backward(x, weight if wd is None else wd, z, scale, shift, mean, invstd)
        ctx.cfg = (training, float(slope), pc, cin, cout, k, bias is not None)
        ctx.packed_dgrad = wd is not None
        ctx.io = io
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, z, scale, shift, mean, invstd = ctx.saved_tensors
        training, slope, pc, cin, cout, k, has_bias = ctx.cfg
        B, D, H, W, _ = x.shape
        dev = x.device
        s = _stream()
        io = ctx.io
        dout = _chk(dout, "grad_output", allow_bf16=True)
        if (dout.dtype == _b16) != bool(io & 2):
            dout = dout.to(_b16 if io & 2 else _f32)
        nblk = _lib.query("tmf_bn_act_pool_bwd_blocks", B, D, H, W, cout, pc)
        part = torch.empty((nblk, 2, cout), device=dev, dtype=_f32)
        _lib.call("tmf_bn_act_pool_bwd_reduce_t", z.data_ptr(), dout.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                  mean.data_ptr(), invstd.data_ptr(), part.data_ptr(), B, D, H, W, cout, pc, slope, io, s)
        dgamma, dbeta, coef, dbias = _bn_bwd_tail(part, nblk, cout, float(B * D * H * W), training, has_bias, scale, dev)
        dz = torch.empty_like(z)
        _lib.call("tmf_bn_act_pool_bwd_apply_t", z.data_ptr(), dout.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                  mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), dz.data_ptr(), B, D, H, W, cout, pc, slope, io, s)
        _fam_f, fam_d, fam_w = ctx.fam
        dweight = _conv_wgrad(fam_w, x, dz, cin, cout, k, True) if ctx.needs_input_grad[1] else None
        dx = None
        if ctx.needs_input_grad[0]:
            wd = weight if ctx.packed_dgrad else pack_weight_dgrad(weight)         # (saved: the dgrad form packed in forward, else the weight)
            if dz.dtype != _f32 and not fam_d.io16:
                dz = dz.float()                   # bf16 storage with a direct data gradient
            dx, _, _ = _conv_forward(fam_d, dz, wd, cout, cin, k, False, fam_d.io16 and x.dtype == _b16)
            if dx.dtype != x.dtype:
                dx = dx.to(x.dtype)
        return (dx, dweight, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None, None)


class Conv1BnPool(torch.autograd.Function):
    """First sNet block (Cin = 1, 3x3x3, max pool) with the conv output never written to HBM: the statistics,
    forward, backward-reduce, weight-gradient and data-gradient passes each recompute it from the input volume."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, running_mean, running_var, training, momentum, eps, slope,
                out_bf16=False, precision=None):
        mode, _act16 = resolve_precision(precision)
        x = _chk(x, "x")
        B, D, H, W, _ = x.shape
        C = weight.shape[0]
        wp = pack_weight(_chk(weight, "weight")).view(27, C)
        dev = x.device
        s = _stream()
        sfx = "_bf16" if mode == "bf16" else ""            # both products on the bf16 matrix cores (opt-in mode)
        gram = part = rows = None
        if training:
            nblk = _lib.query("tmf_c1_blocks", B, D, H, W, C)
            part = torch.empty((nblk, 2, C), device=dev, dtype=_f32)
            gbytes = _lib.query("tmf_c1_gram_bytes" + sfx, B, D, H, W, C) if mode in ("fp32", "bf16") else 0   # (bf16: "c1_gram" 2 only)
            if gbytes:                 # pair sums + the tap Gram matrix of the volume: backward then needs one pass
                gram = torch.empty(gbytes // 8, device=dev, dtype=torch.float64)   # (bf16: of the volume rounded to bf16)
                _lib.call("tmf_c1_stats_g" + sfx, x.data_ptr(), wp.data_ptr(), part.data_ptr(), gram.data_ptr(), gbytes, B, D, H, W, C, s)
                rows = 2
            else:                      # the recomputing pass (bf16: its own; fp32x keeps it: DESIGN 3.16)
                _lib.call("tmf_c1_stats" + sfx, x.data_ptr(), wp.data_ptr(), part.data_ptr(), B, D, H, W, C, s)
                rows = nblk
        mean, invstd, scale, shift = _bn_coeffs(training, part, rows, float(B * D * H * W), gamma, beta, bias,
                                                running_mean, running_var, momentum, eps, C, dev)
        if out_bf16 and not sfx:
            raise _lib.TmfError("a bf16 block output needs conv precision 'bf16'")
        out = torch.empty((B, D // 2, H // 2, W // 2, C), device=dev, dtype=_b16 if out_bf16 else _f32)
        p16 = (int(out_bf16),) if sfx else ()
        if out.numel() > 0:
            _lib.call("tmf_c1_bn_pool_fwd" + sfx, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                      out.data_ptr(), B, D, H, W, C, float(slope), *p16, s)
        ctx.save_for_backward(x, wp, scale, shift, mean, invstd)
        ctx.cfg = (training, float(slope), C, bias is not None, sfx, p16)
        ctx.gram = gram
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, wp, scale, shift, mean, invstd = ctx.saved_tensors
        training, slope, C, has_bias, sfx, p16 = ctx.cfg
        if ctx.needs_input_grad[0] and sfx:
            raise _lib.TmfError("the fused first block has no data gradient in the bf16 precision")
        B, D, H, W, _ = x.shape
        dev = x.device
        s = _stream()
        dout = _chk(dout, "grad_output", allow_bf16=True)
        want16 = bool(p16 and p16[0])
        if (dout.dtype == _b16) != want16:
            dout = dout.to(_b16 if want16 else _f32)
        def dgrad(coef):       # the data gradient from coef = (sum dy, sum dy xhat) / count (zeros: eval mode), conv1_dgrad.hip
            nb = _lib.query("tmf_c1_bwd_dgrad_workspace_bytes", B, D, H, W, C)
            dws = torch.empty((max(nb, 16) // 4,), device=dev, dtype=_f32)
            dx = torch.empty(x.shape, device=dev, dtype=_f32)
            _lib.call("tmf_c1_bwd_dgrad", x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                      invstd.data_ptr(), coef.data_ptr(), dout.data_ptr() if dout.numel() else None, dx.data_ptr(), dws.data_ptr(), nb,
                      B, D, H, W, C, slope, s)
            return dx

        if ctx.gram is not None and training and ctx.needs_input_grad[1]:
            # one pass over the volume: BatchNorm sums and D = x (*) dy together, dw from the forward's Gram data
            nbytes = _lib.query("tmf_c1_bwd_fused_workspace_bytes", B, D, H, W, C)
            ws = torch.empty((max(nbytes, 16) // 4,), device=dev, dtype=_f32)
            dweight = torch.empty((C, 1, 3, 3, 3), device=dev, dtype=_f32)
            dgamma = torch.empty(C, device=dev, dtype=_f32)
            dbeta = torch.empty(C, device=dev, dtype=_f32)
            dx = None
            if ctx.needs_input_grad[0]:    # the same pass also hands out coef (from the finish kernel's doubles); dw, dgamma, dbeta unchanged
                coef = torch.empty((2, C), device=dev, dtype=_f32)
                _lib.call("tmf_c1_bwd_fused_coef", x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                          invstd.data_ptr(), dout.data_ptr(), None, None, ctx.gram.data_ptr(), dweight.data_ptr(), dgamma.data_ptr(),
                          dbeta.data_ptr(), coef.data_ptr(), ws.data_ptr(), nbytes, B, D, H, W, C, slope, _lib.DW_REFERENCE, s)
                dx = dgrad(coef)
            else:
                _lib.call("tmf_c1_bwd_fused" + sfx, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(), mean.data_ptr(),
                          invstd.data_ptr(), dout.data_ptr(), ctx.gram.data_ptr(), dweight.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                          ws.data_ptr(), nbytes, B, D, H, W, C, slope, *p16, _lib.DW_REFERENCE, s)
            dbias = torch.zeros(C, device=dev, dtype=_f32) if has_bias else None
            return (dx, dweight, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None)
        nblk = _lib.query("tmf_c1_blocks", B, D, H, W, C)
        part = torch.empty((nblk, 2, C), device=dev, dtype=_f32)
        _lib.call("tmf_c1_bwd_reduce" + sfx, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                  mean.data_ptr(), invstd.data_ptr(), dout.data_ptr(), part.data_ptr(), B, D, H, W, C, slope, *p16, s)
        dgamma, dbeta, coef, dbias = _bn_bwd_tail(part, nblk, C, float(B * D * H * W), training, has_bias, scale, dev)
        dweight = None
        if ctx.needs_input_grad[1]:
            nbytes = _lib.query("tmf_c1_bwd_wgrad_workspace_bytes", B, D, H, W, C)
            ws = torch.empty((max(nbytes, 16) // 4,), device=dev, dtype=_f32)
            dweight = torch.empty((C, 1, 3, 3, 3), device=dev, dtype=_f32)       # written in the reference layout
            _lib.call("tmf_c1_bwd_wgrad" + sfx, x.data_ptr(), wp.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                      mean.data_ptr(), invstd.data_ptr(), coef.data_ptr(), dout.data_ptr(), dweight.data_ptr(),
                      ws.data_ptr(), nbytes, B, D, H, W, C, slope, *p16, _lib.DW_REFERENCE, s)
        dx = dgrad(coef) if ctx.needs_input_grad[0] else None
        return (dx, dweight, dbias, dgamma, dbeta, None, None, None, None, None, None, None, None)


def conv_bn_act_pool_eval_fused(x, weight, bias, gamma, beta, running_mean, running_var, eps, slope, pool):
    """Inference form of a block (no autograd graph): conv + folded BatchNorm + LeakyReLU + pool in ONE kernel."""
    x, weight = _chk(x, "x"), _chk(weight, "weight")
    cout, cin, k = weight.shape[0], weight.shape[1], weight.shape[2]
    B, D, H, W, C = x.shape
    if C != cin:
        raise _lib.TmfError(f"conv expects {cin} input channels, got {C}")
    dev = x.device
    scale, shift = _bn_eval_coeffs(gamma, beta, bias, running_mean, running_var, eps, cout, dev)
    pc = _lib.pool_code(pool)
    shape = (B, D, H, W, cout) if pc == _lib.POOL_NONE else (B, D // 2, H // 2, W // 2, cout)
    out = torch.empty(shape, device=dev, dtype=_f32)
    if out.numel() > 0:
        fam = _CONV[conv_block_algo("fp32", cin, cout, k)[0]]
        if pool == "avg":                                   # as tmf_snet_eval_fwd chooses: only the direct form averages
            fam = _DIRECT
        w = pack_weight(weight) if fam is _DIRECT else fam.pack(weight, True, False)[0]
        _lib.call(fam.affine, x.data_ptr(), w.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(),
                  B, D, H, W, *fam.fwd[1](cin, cout, k), pc, float(slope), _stream())
    return out


FUSE_EVAL_BLOCKS = os.environ.get("TMF_FUSE_EVAL", "1") != "0"


def conv_bn_act_pool(x, weight, bias, gamma, beta, running_mean, running_var, training,
                     momentum=0.1, eps=1e-5, slope=0.01, pool=None, out_bf16=False, precision=None):
    """precision: make_precision(conv, storage) of the calling module, None = the process default."""
    precision = resolve_precision(precision)
    mode, act16 = precision
    needs_graph = torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad or gamma.requires_grad)
    if (FUSE_EVAL_BLOCKS and not training and not needs_graph and mode == "fp32" and weight.shape[1] > 1
            and weight.shape[1] % 4 == 0 and weight.shape[0] % 4 == 0):
        return conv_bn_act_pool_eval_fused(x, weight, bias, gamma, beta, running_mean, running_var, eps, slope, pool)
    # (an input that wants a gradient: the fused block has the data-gradient pass in the fp32 precisions; the bf16 precision, and a
    # bf16 output asked of an fp32 block, keep the generic route)
    if (weight.shape[1] == 1 and weight.shape[2] == 3 and pool == "max"
            and (not x.requires_grad or (mode != "bf16" and not out_bf16))):
        if out_bf16 and mode != "bf16":
            raise _lib.TmfError("a bf16 block output needs conv precision 'bf16'")
        return Conv1BnPool.apply(x, weight, bias, gamma, beta, running_mean, running_var,
                                 training, momentum, eps, slope, out_bf16 and mode == "bf16", precision)
    can16 = out_bf16 and act16 and bf16_conv_capable(weight.shape[1], weight.shape[2])
    y = ConvBnActPool.apply(x, weight, bias, gamma, beta, running_mean, running_var,
                            training, momentum, eps, slope, pool, can16, precision)
    return y.to(_b16) if (out_bf16 and not can16) else y


# --------------------------------------------------------------------------------------
# whole encoder in one call per pass                                   (networks.py:55-61)
# --------------------------------------------------------------------------------------

# False / TMF_SNET_C=0: every block is its own autograd.Function issued from Python (kept for A/B runs and tests)
SNET_ONE_CALL = os.environ.get("TMF_SNET_C", "1") != "0"


def snet_one_call_supported(B, D, H, W, dim, precision=None):
    return (SNET_ONE_CALL and resolve_precision(precision)[0] in ("fp32", "bf16", "fp32x") and dim >= 32 and dim % 32 == 0
            and min(D, H, W) >= 16 and B > 0)


def snet_eval_one_call(vol, dim, eps, slope, blocks, precision=None, algo=None):
    """Eval-mode sNet forward as ONE library call (tmf_snet_eval_fwd): no autograd graph (val_step runs under no_grad).
    blocks: 7 x (conv weight, conv bias | None, bn weight, bn bias, running_mean, running_var); precision: fp32 (a block is
    one kernel) or bf16 [+ bf16 storage] (the block-by-block launches, enqueued by one call)."""
    import ctypes as C
    vol = _chk(vol, "vol")
    B, _, D, H, W = vol.shape
    mode, act16 = resolve_precision(precision)
    desc = _lib.SnetDesc(B=B, D=D, H=H, W=W, dim=dim, precision=_lib.PRECISION[mode], storage_bf16=int(act16),
                         flags=snet_algo_flags(algo))
    prm = _lib.SnetParams()
    for l, (w, b, g, be, rm, rv) in enumerate(blocks):
        desc.eps[l], desc.slope[l], desc.momentum[l] = eps[l], slope[l], 0.0
        prm.weight[l], prm.bias[l], prm.gamma[l], prm.beta[l] = w.data_ptr(), _ptr(b), g.data_ptr(), be.data_ptr()
        prm.running_mean[l], prm.running_var[l] = rm.data_ptr(), rv.data_ptr()
    nws = _lib.query("tmf_snet_eval_workspace_bytes", C.byref(desc))
    ws = torch.empty(nws, device=vol.device, dtype=torch.uint8)
    out = torch.empty((B, D // 16, H // 16, W // 16, dim), device=vol.device, dtype=_f32)
    _lib.call("tmf_snet_eval_fwd", C.byref(desc), vol.data_ptr(), C.byref(prm), ws.data_ptr(), nws, out.data_ptr(), _stream())
    return out


# Every whole-pass autograd node below (SNetTrain, FusionTrain, HeadsAD, HeadsCNN) writes ALL of its parameter gradients
# into ONE flat buffer and hands autograd views of it.  A data-parallel wrapper (parallel.GradAllReduce) registers itself
# here as a consumer and is told, at the end of each node's backward, about that buffer: it then all-reduces the buffer IN
# PLACE on its own stream (no per-parameter hooks, no pack copies; `param.grad` ends up as a view of the reduced buffer).
# A segment (start, stop, event, when) says that elements [start, stop) are final behind `event` (None: behind everything
# the CURRENT stream has been handed so far) and when their collective should be handed to RCCL: "now" (an encoder's deep
# blocks: the event is recorded in the middle of its backward, conv2 / conv1 still run behind it), "next" (heads, fusion:
# they report in during the launch-bound start of backward, where the host time of an enqueue is idle GPU — they go out
# together with the next "now" range) or "end" (an encoder's shallow blocks: the end of backward).  The set holds consumers WEAKLY: with no
# wrapper alive nothing is published and nothing is kept (k-fold training builds and drops one model per fold).
import weakref

_FLAT_GRAD_CONSUMERS = weakref.WeakSet()


def add_flat_grad_consumer(consumer) -> None:
    """consumer.tmf_flat_grads(flat, param_ptrs, views, segments) is called at the end of every whole-pass backward."""
    _FLAT_GRAD_CONSUMERS.add(consumer)


def remove_flat_grad_consumer(consumer) -> None:
    _FLAT_GRAD_CONSUMERS.discard(consumer)


def _publish_flat_grads(flat, param_ptrs, views, segments) -> None:
    """param_ptrs[i]: data pointer of the parameter whose gradient is views[i] (None: that input got no gradient).
    A consumer must not KEEP a reference to a view: autograd adopts an incoming gradient as ``.grad`` without a copy only
    while it holds the last reference."""
    for c in list(_FLAT_GRAD_CONSUMERS):
        c.tmf_flat_grads(flat, param_ptrs, views, segments)


def snet_algo_flags(algo=None) -> int:
    """The algorithm word of a tmf_snet_desc (include/tmf_hip.h: TMF_SNET_ALGO | ...).  algo None: the process options of the
    moment (tmf_set_option / TMF_* environment), pinned for the call — a backward then runs the plan its forward laid out whatever
    happens to the options in between; a dict {conv_wino: 0..3, wino_p: 0|1, wino_x: 0|1, c1_gram: 0|1|2, c1_split: 0|1, pool_recompute: 0..3} (missing keys: the process
    option) is ONE module's own choice (sNet.set_algorithm): two models with different settings live side by side."""
    f = _lib.query("tmf_snet_algo_flags")
    if algo:
        bad = set(algo) - {"conv_wino", "wino_p", "wino_x", "c1_gram", "c1_split", "pool_recompute"}
        if bad:
            raise ValueError(f"unknown algorithm option(s) {sorted(bad)}")
        if "conv_wino" in algo:
            if algo["conv_wino"] not in (0, 1, 2, 3):
                raise ValueError("conv_wino must be 0, 1, 2 or 3")
            f = (f & ~_lib.snet_algo_wino(3)) | _lib.snet_algo_wino(int(algo["conv_wino"]))
        for key, bit in (("wino_p", _lib.SNET_ALGO_WINO_P), ("wino_x", _lib.SNET_ALGO_WINO_X), ("c1_gram", _lib.SNET_ALGO_C1_GRAM),
                         ("c1_split", _lib.SNET_ALGO_C1_SPLIT)):
            if key in algo:
                f = (f | bit) if algo[key] else (f & ~bit)
        if "c1_gram" in algo:                            # 2: the bf16 mode's first block through the Gram matrix as well
            f = (f | _lib.SNET_ALGO_C1_GRAM_BF16) if algo["c1_gram"] == 2 else (f & ~_lib.SNET_ALGO_C1_GRAM_BF16)
        if "pool_recompute" in algo:                     # 1: the pool routing recomputed in backward; 2 / 3: in block 0 / blocks 2, 4 only
            if algo["pool_recompute"] not in (0, 1, 2, 3):
                raise ValueError("pool_recompute must be 0, 1, 2 or 3")
            c1, bn = _lib.SNET_ALGO_POOL_REC_C1, _lib.SNET_ALGO_POOL_REC_BN
            f = (f & ~(c1 | bn)) | {0: 0, 1: c1 | bn, 2: c1, 3: bn}[int(algo["pool_recompute"])]
    return f


class SNetTrain(torch.autograd.Function):
    """Train-mode sNet forward / backward as ONE library call each (tmf_snet_train_fwd / _bwd: csrc/snet_path.hip): the
    same kernels in the same order as the block-by-block path, every intermediate tensor inside one workspace tensor,
    weight gradients written in the reference layout.  forward(vol (B,1,D,H,W), cfg, buffers, *params) with params =
    7 x (conv weight, conv bias | None, bn weight, bn bias) -> (B, d, h, w, dim) channels-last."""

    @staticmethod
    def forward(ctx, vol, cfg, buffers, *params):
        import ctypes as C
        vol = _chk(vol, "vol")
        dim, momentum, eps, slope = cfg[:4]
        mode, act16 = resolve_precision(cfg[4] if len(cfg) > 4 else None)
        B, _, D, H, W = vol.shape
        desc = _lib.SnetDesc(B=B, D=D, H=H, W=W, dim=dim, precision=_lib.PRECISION[mode], storage_bf16=int(act16),
                             flags=(_lib.SNET_ALONE if (len(cfg) > 5 and cfg[5]) else 0) | snet_algo_flags(cfg[6] if len(cfg) > 6 else None))
        if not any(ctx.needs_input_grad):
            desc.flags |= _lib.SNET_ALGO_POOL_REC_C1 | _lib.SNET_ALGO_POOL_REC_BN   # no backward will follow (no_grad, frozen encoder): keep no pool routing in `saved`
        prm = _lib.SnetParams()
        for l in range(7):
            desc.momentum[l], desc.eps[l], desc.slope[l] = momentum[l], eps[l], slope[l]
            w, b, g, be = params[4 * l:4 * l + 4]
            rm, rv = buffers[l]
            for t, name in ((w, "conv weight"), (g, "BatchNorm weight"), (be, "BatchNorm bias")):
                if not (t.is_cuda and t.dtype == _f32 and t.is_contiguous()):
                    raise _lib.TmfError(f"sNet block {l}: {name} must be a contiguous float32 tensor on the HIP device")
            prm.weight[l], prm.bias[l], prm.gamma[l], prm.beta[l] = w.data_ptr(), _ptr(b), g.data_ptr(), be.data_ptr()
            prm.running_mean[l], prm.running_var[l] = _ptr(rm), _ptr(rv)
        nsaved = _lib.query("tmf_snet_saved_bytes", C.byref(desc))
        if nsaved == 0:
            raise _lib.TmfError("tmf_snet_saved_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
        saved = torch.empty(nsaved, device=vol.device, dtype=torch.uint8)
        out = torch.empty((B, D // 16, H // 16, W // 16, dim), device=vol.device, dtype=_f32)
        _lib.call("tmf_snet_train_fwd", C.byref(desc), vol.data_ptr(), C.byref(prm), saved.data_ptr(), nsaved,
                  out.data_ptr(), _stream())
        ctx.save_for_backward(vol, saved)
        ctx.desc = desc
        ctx.shapes = [None if p is None else p.shape for p in params]
        ctx.param_ptrs = [None if p is None else p.data_ptr() for p in params]
        # the gradient buffer, its views and the gradient table of backward, set up while the GPU is busy (see FusionTrain)
        ctx.bwd = SNetTrain._prepare_backward(ctx.shapes, ctx.needs_input_grad, vol.device) if any(ctx.needs_input_grad[3:]) else None
        return out

    @staticmethod
    def _prepare_backward(shapes, need, dev):
        sizes = [0 if s is None else s.numel() for s in shapes]
        flat = torch.empty(sum(sizes), device=dev, dtype=_f32)        # all 28 gradients in one allocation
        # layout [shallow blocks 0 .. DEEP_FROM-1 | deep blocks DEEP_FROM .. 6 | the seven conv-bias gradients]: the bias
        # gradients (exact zeros) sit back to back at the end — the library fills them with ONE memset at the START of
        # backward — so [deep | biases] is one contiguous range that is final at `deep_event`
        shallow = [i for i in range(4 * _lib.SNET_DEEP_FROM) if i % 4 != 1]
        order = shallow + [i for i in range(4 * _lib.SNET_DEEP_FROM, len(sizes)) if i % 4 != 1] + \
            [i for i in range(len(sizes)) if i % 4 == 1]
        parts = dict(zip(order, flat.split([sizes[i] for i in order])))
        o_deep = sum(sizes[i] for i in shallow)
        grads = [None if s is None else (parts[i] if len(s) == 1 else parts[i].view(s)) for i, s in enumerate(shapes)]
        ptr = [parts[i].data_ptr() for i in range(len(sizes))]
        g = _lib.SnetGrads()
        for l in range(7):
            g.dweight[l] = ptr[4 * l] if need[3 + 4 * l] else None
            g.dbias[l] = None if shapes[4 * l + 1] is None else ptr[4 * l + 1]
            g.dgamma[l], g.dbeta[l] = ptr[4 * l + 2], ptr[4 * l + 3]
        # an event behind the last kernel of the deep blocks (conv3.0 .. conv4.3): a data-parallel wrapper starts the
        # all-reduce of their gradients there, under the backward of conv2 / conv1, instead of after this call
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))               # (creates the handle; the library re-records it in backward)
        g.deep_event = ev.cuda_event
        return flat, grads, g, ev, o_deep

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        import ctypes as C
        vol, saved = ctx.saved_tensors
        desc = ctx.desc
        dout = _chk(dout, "grad_output")
        prep = ctx.bwd if ctx.bwd is not None else SNetTrain._prepare_backward(ctx.shapes, ctx.needs_input_grad, vol.device)
        ctx.bwd = None
        flat, grads, g, ev, o_deep = prep
        nscr = _lib.query("tmf_snet_bwd_scratch_bytes", C.byref(desc))
        scratch = torch.empty(nscr, device=vol.device, dtype=torch.uint8)
        dvol = None
        if ctx.needs_input_grad[0]:        # block 0 also runs the data-gradient pass (fp32 / fp32x; the library refuses bf16)
            dvol = torch.empty_like(vol)
            _lib.call("tmf_snet_train_bwd_input", C.byref(desc), vol.data_ptr(), saved.data_ptr(), saved.numel(), dout.data_ptr(),
                      C.byref(g), scratch.data_ptr(), nscr, _stream(), dvol.data_ptr())
        else:
            _lib.call("tmf_snet_train_bwd", C.byref(desc), vol.data_ptr(), saved.data_ptr(), saved.numel(), dout.data_ptr(),
                      C.byref(g), scratch.data_ptr(), nscr, _stream())
        out = [dvol, None, None]
        for i, gr in enumerate(grads):
            out.append(gr if (gr is not None and ctx.needs_input_grad[3 + i]) else None)
        if _FLAT_GRAD_CONSUMERS and all(ctx.needs_input_grad[3 + i] for i, gr in enumerate(grads) if gr is not None):
            # shallow blocks: final when this call's last kernel is; deep blocks + bias zeros: final at the event
            _publish_flat_grads(flat, ctx.param_ptrs, grads, [(o_deep, flat.numel(), ev, "now"), (0, o_deep, None, "end")])
        return tuple(out)


# --------------------------------------------------------------------------------------
# fused cross attention                                               (networks.py:166-174)
# --------------------------------------------------------------------------------------

class CrossAttention(torch.autograd.Function):
    """out[b, n, (h d)] = softmax(q k^T * scale) v with q: (B, N, h*d), kv: (B, M, 2*h*d)
    (the raw to_q / to_kv outputs: no rearrange, no chunk copy)."""

    @staticmethod
    def forward(ctx, q, kv, heads, scale):
        q, kv = _chk(q, "q"), _chk(kv, "kv")
        B, N, inner = q.shape
        M = kv.shape[1]
        if kv.shape[2] != 2 * inner or inner % heads:
            raise _lib.TmfError(f"attention shapes: q {tuple(q.shape)} kv {tuple(kv.shape)} heads {heads}")
        dh = inner // heads
        out = torch.empty((B, N, inner), device=q.device, dtype=_f32)
        lse = torch.empty((B, heads, N), device=q.device, dtype=_f32)
        _lib.call("tmf_xattn_fwd", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, out.data_ptr(),
                  lse.data_ptr(), B, heads, N, M, dh, inner, 2 * inner, float(scale), _stream())
        ctx.save_for_backward(q, kv, out, lse)
        ctx.cfg = (heads, float(scale))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, kv, out, lse = ctx.saved_tensors
        heads, scale = ctx.cfg
        B, N, inner = q.shape
        M = kv.shape[1]
        dh = inner // heads
        dout = _chk(dout, "grad_output")
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        _lib.call("tmf_xattn_bwd", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, out.data_ptr(),
                  lse.data_ptr(), dout.data_ptr(), dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + inner * 4,
                  B, heads, N, M, dh, inner, 2 * inner, 2 * inner, scale, _stream())
        return dq, dkv, None, None


def cross_attention(q, kv, heads, scale):
    return CrossAttention.apply(q, kv, heads, scale)


# --------------------------------------------------------------------------------------
# LayerNorm                                                          (networks.py:117,219)
# --------------------------------------------------------------------------------------

class LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, residual):
        x = _chk(x, "x")
        dim = x.shape[-1]
        rows = x.numel() // dim
        y = torch.empty_like(x)
        mean = torch.empty(rows, device=x.device, dtype=_f32)
        rstd = torch.empty(rows, device=x.device, dtype=_f32)
        res = _chk(residual, "residual") if residual is not None else None
        _lib.call("tmf_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(res), y.data_ptr(),
                  mean.data_ptr(), rstd.data_ptr(), rows, dim, float(eps), _stream())
        ctx.save_for_backward(x, gamma, mean, rstd)
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dim = x.shape[-1]
        rows = x.numel() // dim
        dy = _chk(dy, "grad_output")
        dx = torch.empty_like(x)
        nblk = _lib.query("tmf_layernorm_bwd_blocks", rows, dim)
        part = torch.empty((nblk, 2, dim), device=x.device, dtype=_f32)
        s = _stream()
        _lib.call("tmf_layernorm_bwd", x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                  dy.data_ptr(), dx.data_ptr(), part.data_ptr(), rows, dim, s)
        gb = torch.empty((2, dim), device=x.device, dtype=_f32)
        _lib.call("tmf_colsum_finalize", part.data_ptr(), nblk, 2 * dim, gb.data_ptr(), s)
        return dx, gb[0], gb[1], None, (dy if ctx.has_res else None)


def layer_norm(x, gamma, beta, eps=1e-5, residual=None):
    """LayerNorm(x) * gamma + beta (+ residual, fused into the same pass)."""
    return LayerNorm.apply(x, gamma, beta, eps, residual)


# --------------------------------------------------------------------------------------
# fused transformer block: every nn.Linear is one launch that also does the LayerNorm / bias / GELU /
# residual around it (csrc/token_gemm.hip).                         (networks.py:114-175, 215-230)
# --------------------------------------------------------------------------------------

def tok_linear_fwd(x, w, bias=None, residual=None, ln=None, gelu=False, keep_ln_out=False, mask=None):
    """y = [GELU](LayerNorm?(x) @ w.T + bias) + residual on 2-D row-major fp32 tensors.
    ln = (gamma, beta, eps).  mask: a scaled Dropout keep-mask (R, Nout) applied before the residual / after the GELU
    (tmf_tok_linear_fwd_masked; `pre` stays unmasked).  Returns (y, ln_saved, pre): ln_saved = (mean, rstd, normalised
    rows | None)."""
    R, K = x.shape
    nout = w.shape[0]
    y = torch.empty((R, nout), device=x.device, dtype=_f32)
    mean = rstd = ln_out = pre = None
    g = b = None
    eps = 0.0
    if ln is not None:
        g, b, eps = ln
        mean = torch.empty(R, device=x.device, dtype=_f32)
        rstd = torch.empty(R, device=x.device, dtype=_f32)
        if keep_ln_out:
            ln_out = torch.empty((R, K), device=x.device, dtype=_f32)
    if gelu:
        pre = torch.empty((R, nout), device=x.device, dtype=_f32)
    args = (x.data_ptr(), w.data_ptr(), _ptr(bias), _ptr(residual), y.data_ptr(), R, K, nout, _ptr(g), _ptr(b), float(eps),
            _ptr(mean), _ptr(rstd), _ptr(ln_out), _ptr(pre))
    if mask is None:
        _lib.call("tmf_tok_linear_fwd", *args, _stream())
    else:
        _lib.call("tmf_tok_linear_fwd_masked", *args, _chk(mask, "mask").data_ptr(), _stream())
    return y, (mean, rstd, ln_out), pre


def tok_linear_bwd_input(dy, w, gelu_pre=None, ln=None, add1=None, add2=None, ln_partial=None, bias_partial=None,
                         partial_stride=0, mask=None, mask_out=None):
    """dx = E(dy @ w); ln = (x, mean, rstd, gamma) selects the LayerNorm-backward epilogue.  ln_partial /
    bias_partial are (tensor, column offset) pairs into one [row blocks][partial_stride] workspace.  mask: a scaled
    Dropout keep-mask (R, K) (tmf_tok_linear_bwd_input_masked): with gelu_pre it multiplies the GELU gradient, with ln
    the epilogue also writes mask * dx to `mask_out`."""
    R, nout = dy.shape
    K = w.shape[1]
    dx = torch.empty((R, K), device=dy.device, dtype=_f32)
    lx = lm = lr = lg = None
    if ln is not None:
        lx, lm, lr, lg = ln

    def off(pair):
        return None if pair is None else pair[0].data_ptr() + 4 * pair[1]
    args = (dy.data_ptr(), w.data_ptr(), dx.data_ptr(), R, nout, K, _ptr(gelu_pre), _ptr(lx), _ptr(lm), _ptr(lr), _ptr(lg),
            _ptr(add1), _ptr(add2), off(ln_partial), off(bias_partial), partial_stride)
    if mask is None:
        _lib.call("tmf_tok_linear_bwd_input", *args, _stream())
    else:
        _lib.call("tmf_tok_linear_bwd_input_masked", *args, _chk(mask, "mask").data_ptr(), _ptr(mask_out), _stream())
    return dx


def mask_mul(x, mask):
    """x * mask (a scaled Dropout keep-mask of x's shape) in one launch (tmf_mask_mul)."""
    x, mask = _chk(x, "x"), _chk(mask, "mask")
    if mask.shape != x.shape:
        raise _lib.TmfError(f"mask_mul: mask {tuple(mask.shape)} vs x {tuple(x.shape)}")
    y = torch.empty_like(x)
    _lib.call("tmf_mask_mul", x.data_ptr(), mask.data_ptr(), y.data_ptr(), x.numel(), _stream())
    return y


# False / TMF_FUSE_TOKENS=0: every op of the block is its own launch (kept for A/B measurements and tests)
FUSE_TOKEN_LINEARS = os.environ.get("TMF_FUSE_TOKENS", "1") != "0"


def tok_wgrad_multi(pairs):
    """[dy_p^T @ x_p for (dy_p, x_p) in pairs] — all weight gradients of a block in one launch (+ one reduction)."""
    import ctypes as C
    n = len(pairs)
    Rs = (C.c_int * n)(*[dy.shape[0] for dy, _ in pairs])
    Ns = (C.c_int * n)(*[dy.shape[1] for dy, _ in pairs])
    Ks = (C.c_int * n)(*[x.shape[1] for _, x in pairs])
    dev = pairs[0][0].device
    flat = torch.empty(sum(dy.shape[1] * x.shape[1] for dy, x in pairs), device=dev, dtype=_f32)
    outs, o = [], 0
    for dy, x in pairs:
        m = dy.shape[1] * x.shape[1]
        outs.append(flat[o:o + m].view(dy.shape[1], x.shape[1]))
        o += m
    dys = (C.c_void_p * n)(*[dy.data_ptr() for dy, _ in pairs])
    xs = (C.c_void_p * n)(*[x.data_ptr() for _, x in pairs])
    dws = (C.c_void_p * n)(*[t.data_ptr() for t in outs])
    nbytes = _lib.query("tmf_tok_wgrad_multi_workspace_bytes", n, Ns, Ks)
    ws = torch.empty(nbytes // 4, device=dev, dtype=_f32)
    _lib.call("tmf_tok_wgrad_multi", n, dys, xs, dws, Rs, Ns, Ks, ws.data_ptr(), nbytes, _stream())
    return outs


# the block widths token_gemm.hip's LayerNorm prologue / LayerNorm-backward epilogue take
TOKEN_GEMM_DIMS = (64, 128, 256)


def fused_block_supported(dim, inner, mlp):
    return FUSE_TOKEN_LINEARS and dim in TOKEN_GEMM_DIMS and inner % 64 == 0 and mlp % 64 == 0


class TransformerLayer(torch.autograd.Function):
    """x <- Attention(LayerNorm(x), context) + x ; x <- FeedForward(LayerNorm(x)) + x   as 6 launches forward
    (to_q with LayerNorm prologue, to_kv, attention, to_out + bias + x, Linear + bias + GELU with LayerNorm
    prologue, Linear + bias + x) and 7 + 1 (all five weight gradients) + 2 reductions backward.  masks = the scaled
    Dropout keep-masks (m_o (R, dim), m_g (R, mlp), m_f (R, dim); any may be None) of networks.py:153, :131, :133, applied
    in the Linears' epilogues; backward multiplies its incoming gradient by m_f in one extra launch (tmf_mask_mul).
    context2 (optional): the second part of a two-part context [context ; context2] (CrossTransformer, networks.py:250-251),
    never concatenated: one to_kv launch per part, tmf_xattn_fwd_cat / _bwd_cat read and write both in place."""

    @staticmethod
    def forward(ctx, x, context, g1, b1n, wq, wkv, wo, bo, g2, b2n, w1, b1, w2, b2, heads, scale, eps1, eps2, masks=None,
                context2=None):
        mo, mg, mf = masks if masks is not None else (None, None, None)
        x, context = _chk(x, "x"), _chk(context, "context")
        B, N, dim = x.shape
        M = context.shape[1]
        inner = wq.shape[0]
        x2d, c2d = x.view(B * N, dim), context.view(B * M, dim)
        q, (mean1, rstd1, a), _ = tok_linear_fwd(x2d, wq, ln=(g1, b1n, eps1), keep_ln_out=True)
        kv, _, _ = tok_linear_fwd(c2d, wkv)
        dh = inner // heads
        out = torch.empty((B * N, inner), device=x.device, dtype=_f32)
        lse = torch.empty((B, heads, N), device=x.device, dtype=_f32)
        c22d = kv2 = None
        M2 = 0
        if context2 is None:
            _lib.call("tmf_xattn_fwd", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, out.data_ptr(),
                      lse.data_ptr(), B, heads, N, M, dh, inner, 2 * inner, float(scale), _stream())
        else:
            context2 = _chk(context2, "context2")
            M2 = context2.shape[1]
            if context2.shape[0] != B or context2.shape[2] != dim:
                raise _lib.TmfError(f"context parts {tuple(context.shape)} and {tuple(context2.shape)}")
            c22d = context2.view(B * M2, dim)
            kv2, _, _ = tok_linear_fwd(c22d, wkv)
            _lib.call("tmf_xattn_fwd_cat", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, kv2.data_ptr(),
                      kv2.data_ptr() + inner * 4, out.data_ptr(), lse.data_ptr(), B, heads, N, M, M2, dh, inner, 2 * inner,
                      float(scale), _stream())
        x1, _, _ = tok_linear_fwd(out, wo, bias=bo, residual=x2d, mask=mo)
        g, (mean2, rstd2, f), h = tok_linear_fwd(x1, w1, bias=b1, ln=(g2, b2n, eps2), gelu=True, keep_ln_out=True, mask=mg)
        x2, _, _ = tok_linear_fwd(g, w2, bias=b2, residual=x1, mask=mf)
        ctx.save_for_backward(x2d, c2d, g1, wq, wkv, wo, g2, w1, w2, mean1, rstd1, a, q, kv, out, lse, x1, mean2,
                              rstd2, f, h, g, c22d, kv2)
        ctx.cfg = (B, N, M, dim, inner, heads, float(scale), M2)
        ctx.masks = (mo, mg, mf)
        return x2.view(B, N, dim)

    @staticmethod
    def backward(ctx, dx2):
        (x2d, c2d, g1, wq, wkv, wo, g2, w1, w2, mean1, rstd1, a, q, kv, out, lse, x1, mean2, rstd2, f, h,
         g, c22d, kv2) = ctx.saved_tensors
        B, N, M, dim, inner, heads, scale, M2 = ctx.cfg
        mlp = w1.shape[0]
        R = B * N
        dx2 = _chk(dx2, "grad_output").view(R, dim)
        nblk = _lib.query("tmf_tok_row_blocks", R)
        # one [row blocks][stride] workspace for every bias / LayerNorm parameter gradient of the block
        o_b2, o_b1, o_bo, o_ln2, o_ln1 = 0, dim, dim + mlp, 2 * dim + mlp, 4 * dim + mlp
        stride = 6 * dim + mlp
        part = torch.empty((nblk, stride), device=dx2.device, dtype=_f32)
        # Dropout: e_f = m_f dx2 and e_o = m_o dx1 are the dy of the second FeedForward Linear and of to_out; the residual
        # paths carry the unmasked dx2 / dx1
        mo, mg, mf = ctx.masks
        ef = dx2 if mf is None else mask_mul(dx2, mf)
        dh_ = tok_linear_bwd_input(ef, w2, gelu_pre=h, bias_partial=(part, o_b2), partial_stride=stride, mask=mg)
        eo = None if mo is None else torch.empty((R, dim), device=dx2.device, dtype=_f32)
        dx1 = tok_linear_bwd_input(dh_, w1, ln=(x1, mean2, rstd2, g2), add1=dx2, ln_partial=(part, o_ln2),
                                   bias_partial=(part, o_b1), partial_stride=stride, mask=mo, mask_out=eo)
        if eo is None:
            eo = dx1
        dout = tok_linear_bwd_input(eo, wo, bias_partial=(part, o_bo), partial_stride=stride)
        dq = torch.empty_like(q)
        dkv = torch.empty_like(kv)
        dhd = inner // heads
        dkv2 = dctx2 = None
        if kv2 is None:
            _lib.call("tmf_xattn_bwd", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, out.data_ptr(),
                      lse.data_ptr(), dout.data_ptr(), dq.data_ptr(), dkv.data_ptr(), dkv.data_ptr() + inner * 4,
                      B, heads, N, M, dhd, inner, 2 * inner, 2 * inner, scale, _stream())
        else:
            dkv2 = torch.empty_like(kv2)
            _lib.call("tmf_xattn_bwd_cat", q.data_ptr(), kv.data_ptr(), kv.data_ptr() + inner * 4, kv2.data_ptr(),
                      kv2.data_ptr() + inner * 4, out.data_ptr(), lse.data_ptr(), dout.data_ptr(), dq.data_ptr(),
                      dkv.data_ptr(), dkv.data_ptr() + inner * 4, dkv2.data_ptr(), dkv2.data_ptr() + inner * 4,
                      B, heads, N, M, M2, dhd, inner, 2 * inner, 2 * inner, scale, _stream())
            if ctx.needs_input_grad[19]:
                dctx2 = tok_linear_bwd_input(dkv2, wkv).view(B, M2, dim)
        dctx = tok_linear_bwd_input(dkv, wkv) if ctx.needs_input_grad[1] else None
        dx = tok_linear_bwd_input(dq, wq, ln=(x2d, mean1, rstd1, g1), add1=dx1, ln_partial=(part, o_ln1),
                                  partial_stride=stride)
        sums = torch.empty(stride, device=dx2.device, dtype=_f32)
        _lib.call("tmf_colsum_finalize", part.data_ptr(), nblk, stride, sums.data_ptr(), _stream())
        pairs = [(ef, g), (dh_, f), (eo, out), (dkv, c2d), (dq, a)] + ([] if kv2 is None else [(dkv2, c22d)])
        dws = tok_wgrad_multi(pairs)
        dw2, dw1, dwo, dwkv, dwq = dws[:5]
        if kv2 is not None:
            dwkv = dwkv + dws[5]                    # to_kv saw both context parts
        return (dx.view(B, N, dim), None if dctx is None else dctx.view(B, M, dim),
                sums[o_ln1:o_ln1 + dim], sums[o_ln1 + dim:o_ln1 + 2 * dim], dwq, dwkv, dwo, sums[o_bo:o_bo + dim],
                sums[o_ln2:o_ln2 + dim], sums[o_ln2 + dim:o_ln2 + 2 * dim], dw1, sums[o_b1:o_b1 + mlp], dw2,
                sums[o_b2:o_b2 + dim], None, None, None, None, None, dctx2)


def transformer_layer(x, context, ln1, attn, ln2, ff, masks=None, context2=None):
    """ln1 / ln2: nn.LayerNorm; attn: networks.Attention; ff: networks.FeedForward (parameter containers); masks: the
    layer's scaled Dropout keep-masks (to_out, after GELU, after the second Linear) or None; context2: the second part of
    a two-part context [context ; context2] or None."""
    if masks is not None and all(m is None for m in masks):
        masks = None
    return TransformerLayer.apply(x, context, ln1.weight, ln1.bias, attn.to_q.weight, attn.to_kv.weight,
                                  attn.to_out[0].weight, attn.to_out[0].bias, ln2.weight, ln2.bias,
                                  ff.net[0].weight, ff.net[0].bias, ff.net[3].weight, ff.net[3].bias,
                                  attn.heads, attn.scale, ln1.eps, ln2.eps, masks, context2)


# --------------------------------------------------------------------------------------
# whole fusion transformer in one call per pass                      (networks.py:255-281)
# --------------------------------------------------------------------------------------

FUSION_ONE_CALL = os.environ.get("TMF_FUSION_C", "1") != "0"
# the fused per-instance kernels (csrc/xformer_fused.hip) inside the one-call path; "0" keeps one launch per Linear
FUSION_FUSED_KERNELS = os.environ.get("TMF_FUSION_FUSED", "1") != "0"


def fusion_fused_supported(N, dim, heads, dim_head, mlp):
    """Shapes the fused per-instance kernels take (tmf_xf_supported, csrc/xformer_fused.hip)."""
    return (FUSION_ONE_CALL and FUSION_FUSED_KERNELS and dim == 128 and (heads, dim_head) in ((4, 32), (8, 16)) and mlp == 512
            and 1 <= N <= 512)


def dropout_keep_mask(drop, shape, device):
    """Scaled keep-mask of an nn.Dropout in train mode (None when inactive).  A module that provides
    ``tmf_keep_mask(training)`` (tests: fixed masks captured from the reference) supplies its own."""
    if hasattr(drop, "tmf_keep_mask"):
        m = drop.tmf_keep_mask(drop.training)
        return None if m is None else m.to(device=device, dtype=_f32).reshape(shape).contiguous()
    p = float(getattr(drop, "p", 0.0))
    if not drop.training or p <= 0.0:
        return None
    if p >= 1.0:
        return torch.zeros(shape, device=device, dtype=_f32)
    return torch.empty(shape, device=device, dtype=_f32).bernoulli_(1.0 - p).div_(1.0 - p)


_MASK_CALLS = 0          # fallback call counter (a generator without an offset API)


def _mask_stream(device):
    """(seed, offset) of the next tmf_dropout_keep_masks call, taken from torch's OWN device generator — the Philox stream
    position torch's dropout kernels consume — and advanced past it: `torch.manual_seed(s)` therefore reproduces the masks
    of a run exactly as it reproduces nn.Dropout's (seed and offset are host-side integers: no synchronisation)."""
    global _MASK_CALLS
    try:
        gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
        off = gen.get_offset()
        gen.set_offset(off + 4)                              # (torch's offsets move in multiples of 4)
        return gen.initial_seed() & 0xFFFFFFFFFFFFFFFF, off
    except Exception:                                        # pragma: no cover
        _MASK_CALLS += 1
        return torch.initial_seed() & 0xFFFFFFFFFFFFFFFF, (1 << 40) + _MASK_CALLS


def dropout_keep_masks(requests, device):
    """Scaled keep-masks for MANY Dropout modules in ONE launch (tmf_dropout_keep_masks: a counter-based Philox generator
    keyed by the seed and stream offset of torch's device generator, so torch.manual_seed makes a run reproducible): requests = [(drop, shape), ...] -> list
    of fp32 masks (None where the module is inactive).  The two Dropout(0.5) of fc_cls were 6 stock launches per step, the
    18 masks of a depth-3 fusion block with dropout 36; modules that bring their own mask (``tmf_keep_mask``: the tests'
    fixed masks) and p >= 1 are served as in dropout_keep_mask."""
    import ctypes as C
    out = [None] * len(requests)
    live = []
    for i, (drop, shape) in enumerate(requests):
        p = float(getattr(drop, "p", 0.0))
        if hasattr(drop, "tmf_keep_mask") or p >= 1.0 or p <= 0.0 or not drop.training:
            out[i] = dropout_keep_mask(drop, shape, device)
        else:
            live.append((i, 1.0 - p, int(torch.Size(shape).numel())))
    for s0 in range(0, len(live), _lib.MASK_SEGMENTS):
        part = live[s0:s0 + _lib.MASK_SEGMENTS]
        sizes = [(n + 3) & ~3 for _i, _k, n in part]                     # 16-byte aligned segments
        flat = torch.empty(sum(sizes), device=device, dtype=_f32)
        ptrs, off = [], 0
        for (i, _k, n), sz in zip(part, sizes):
            out[i] = flat[off:off + n].view(requests[i][1])
            ptrs.append(flat.data_ptr() + 4 * off)
            off += sz
        seed, offset = _mask_stream(device)
        _lib.call("tmf_dropout_keep_masks", len(part), (C.c_void_p * len(part))(*ptrs), (C.c_long * len(part))(*[n for _i, _k, n in part]),
                  (C.c_float * len(part))(*[k for _i, k, _n in part]), seed, offset, _stream())
    return out


def fusion_one_call_supported(dim, inner, mlp, dim_head, depth):
    return (FUSION_ONE_CALL and FUSE_TOKEN_LINEARS and dim in TOKEN_GEMM_DIMS and inner % 64 == 0 and mlp % 64 == 0
            and dim_head in (8, 16, 32, 64) and 0 < depth <= 16)


def fusion_takes_masks(dim, inner, mlp, dim_head):
    """Geometries whose one-call fusion entry takes Dropout keep-masks (tmf_fusion_takes_masks): every one it accepts —
    the fused per-instance kernels at dim 128 apply them, one launch per op (token_gemm.hip's masked epilogues) elsewhere."""
    return dim in TOKEN_GEMM_DIMS and inner % 64 == 0 and mlp % 64 == 0 and dim_head in (8, 16, 32, 64)


def _fusion_call_setup(mri, pet, cfg, params):
    """What both fusion entries take: checked tokens, the descriptor, the per-instance parameter table (tmf_xformer_params,
    pointers of `params` in _lib.XFORMER_PTRS order) and this call's Dropout keep-masks (kept alive by the returned list)."""
    mri, pet = _chk(mri, "mri_tokens"), _chk(pet, "pet_tokens")
    heads, dim_head, mlp, depth, eps = cfg[:5]
    drops = cfg[5] if len(cfg) > 5 else None      # per instance the three nn.Dropout modules (to_out, GELU, Linear 2)
    B, N, dim = mri.shape
    if pet.shape != mri.shape:
        raise _lib.TmfError(f"token shapes differ: {tuple(mri.shape)} vs {tuple(pet.shape)}")
    desc = _lib.FusionDesc(B=B, N=N, dim=dim, heads=heads, dim_head=dim_head, mlp=mlp, depth=depth,
                           flags=0 if FUSION_FUSED_KERNELS else _lib.FUSION_PER_OP)
    inst = (_lib.XformerParams * (2 * depth))()
    masks = []
    for i in range(2 * depth):
        for j, name in enumerate(_lib.XFORMER_PTRS):
            t = params[14 * i + j]
            if not (t.is_cuda and t.dtype == _f32 and t.is_contiguous()):
                raise _lib.TmfError(f"Transformer instance {i}: {name} must be a contiguous float32 HIP tensor")
            setattr(inst[i], name, t.data_ptr())
        inst[i].eps1, inst[i].eps2, inst[i].epsf = eps[i]
    if drops is not None:                    # every keep-mask of the step in one draw per distinct p
        req = [(drop, (B * N, width)) for i in range(2 * depth) for drop, width in zip(drops[i], (dim, mlp, dim))]
        for j, mk in enumerate(dropout_keep_masks(req, mri.device)):
            if mk is not None:
                masks.append(mk)
                setattr(inst[j // 3], ("mask_o", "mask_g", "mask_f")[j % 3], mk.data_ptr())
    return mri, pet, desc, inst, masks


FUSION_INFER_ONE_CALL = os.environ.get("TMF_FUSION_INFER_C", "1") != "0"


def fusion_infer_ok(mri_tokens):
    """The part of the forward-only route's predicate that does not depend on the module (networks.CrossTransformer_MOD_AVG
    adds its own geometry / hook checks): device tokens, grad mode off, the switch on."""
    return FUSION_INFER_ONE_CALL and mri_tokens.is_cuda and not torch.is_grad_enabled()


def fusion_infer(mri_tok, pet_tok, cfg, params):
    """CrossTransformer_MOD_AVG's forward under no_grad as ONE library call that keeps nothing (tmf_fusion_infer_fwd,
    csrc/fusion_path.hip): cfg and params as FusionTrain.forward takes them -> cls (B, 4*dim), bit-identical to
    FusionTrain's.  No autograd."""
    import ctypes as C
    mri, pet, desc, inst, masks = _fusion_call_setup(mri_tok, pet_tok, cfg, params)
    nws = _lib.query("tmf_fusion_infer_workspace_bytes", C.byref(desc))
    if nws == 0:
        raise _lib.TmfError("tmf_fusion_infer_workspace_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
    ws = torch.empty(nws, device=mri.device, dtype=torch.uint8)
    cls = torch.empty((mri.shape[0], 4 * mri.shape[2]), device=mri.device, dtype=_f32)
    _lib.call("tmf_fusion_infer_fwd", C.byref(desc), mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), nws,
              cls.data_ptr(), _stream())
    return cls


def xattn_probs(q, kv, lse, heads, scale, kv2=None, want_probs=True):
    """The attention probabilities of cross_attention(q, kv, ...) rebuilt from its base-2 log-sum-exp `lse` (B, heads, N)
    (tmf_xattn_probs, csrc/attention.hip): q (B, N, h*d), kv (B, M1, 2*h*d), kv2 (B, M2, 2*h*d) or None, the second part of a
    two-part context -> (probs (B, heads, N, M1 + M2) or None, recv (B, heads, M1 + M2) = the mean of probs over the queries)."""
    q, kv, lse = _chk(q, "q"), _chk(kv, "kv"), _chk(lse, "lse")
    B, N, inner = q.shape
    M1 = kv.shape[1]
    if kv.shape[0] != B or kv.shape[2] != 2 * inner or inner % heads or tuple(lse.shape) != (B, heads, N):
        raise _lib.TmfError(f"attention shapes: q {tuple(q.shape)} kv {tuple(kv.shape)} lse {tuple(lse.shape)} heads {heads}")
    M2 = 0
    if kv2 is not None:
        kv2 = _chk(kv2, "kv2")
        M2 = kv2.shape[1]
        if kv2.shape[0] != B or kv2.shape[2] != 2 * inner or M2 == 0:
            raise _lib.TmfError(f"attention shapes: kv2 {tuple(kv2.shape)} against kv {tuple(kv.shape)}")
    probs = torch.empty((B, heads, N, M1 + M2), device=q.device, dtype=_f32) if want_probs else None
    recv = torch.empty((B, heads, M1 + M2), device=q.device, dtype=_f32)
    _lib.call("tmf_xattn_probs", q.data_ptr(), kv.data_ptr(), _ptr(kv2), lse.data_ptr(), _ptr(probs), recv.data_ptr(),
              B, heads, N, M1, M2, inner // heads, inner, 2 * inner, float(scale), _stream())
    return probs, recv


def fusion_attn_maps(mri_tok, pet_tok, cfg, params, want_probs):
    """fusion_infer with the attention maps of every Transformer instance (tmf_fusion_attn_maps, csrc/fusion_path.hip; always
    one launch per op): -> (cls (B, 4*dim), recv (2*depth, B, heads, N), probs (2*depth, B, heads, N, N) or None).  Instance
    2l: layer l's mri encoder (queries mri, keys pet); 2l + 1: its pet encoder (queries pet, keys the new mri tokens)."""
    import ctypes as C
    mri, pet, desc, inst, masks = _fusion_call_setup(mri_tok, pet_tok, cfg, params)
    nws = _lib.query("tmf_fusion_attn_maps_workspace_bytes", C.byref(desc))
    if nws == 0:
        raise _lib.TmfError("tmf_fusion_attn_maps_workspace_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
    B, N, dim = mri.shape
    n_inst = 2 * desc.depth
    ws = torch.empty(nws, device=mri.device, dtype=torch.uint8)
    cls = torch.empty((B, 4 * dim), device=mri.device, dtype=_f32)
    recv = torch.empty((n_inst, B, desc.heads, N), device=mri.device, dtype=_f32)
    probs = torch.empty((n_inst, B, desc.heads, N, N), device=mri.device, dtype=_f32) if want_probs else None
    _lib.call("tmf_fusion_attn_maps", C.byref(desc), mri.data_ptr(), pet.data_ptr(), inst, ws.data_ptr(), nws,
              cls.data_ptr(), _ptr(probs), recv.data_ptr(), _stream())
    return cls, recv, probs


CAM_METHODS = {"gradcam": _lib.CAM_GRAD, "hirescam": _lib.CAM_HIRES}


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def _int(v, msg, lo, hi=None):
    """v if it is an int (no bool) in lo..hi (hi None: no upper end); ValueError(f"{msg}, got {v!r}") otherwise."""
    if not _is_int(v) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{msg}, got {v!r}")
    return v


def _kernel_takes(*pairs, contiguous=True):
    """The one device test of the explanation kernels.  pairs: (tensor, the dtype its entry reads - or a tuple of dtypes); all on
    one HIP device, each of its dtype, contiguous (unless `contiguous` is off) and not empty."""
    dev = pairs[0][0].device
    return all(t.is_cuda and t.device == dev and t.dtype in (d if isinstance(d, tuple) else (d,))
               and (t.is_contiguous() or not contiguous) and t.numel() > 0 for t, d in pairs)


def cam_ok(act, grad):
    """tmf_cam takes this pair: float32 tensors on one HIP device, a channel count tmf_cam_ok accepts, at least one voxel."""
    return _kernel_takes((act, _f32), (grad, _f32), contiguous=False) and bool(_lib.query("tmf_cam_ok", int(act.shape[-1])))


def cam(act, grad, method="gradcam", relu=True, normalize=True):
    """Class activation map of a channels-last activation act (B, ..., C) and the score's gradient by it, same shape
    (tmf_cam, csrc/cam.hip) -> (cam (B, ...), weights (B, C) or None for "hirescam", peak (B,) = each sample's maximum before
    the division).  "gradcam": weights = the mean of grad over the voxels, cam = sum_c weights * act; "hirescam": cam =
    sum_c grad * act.  relu clamps at 0; normalize divides each sample by its maximum (zeros where that is <= 0)."""
    if method not in CAM_METHODS:
        raise ValueError(f"method must be one of {sorted(CAM_METHODS)}, got {method!r}")
    act, grad = _chk(act, "act"), _chk(grad, "grad")
    if act.shape != grad.shape or act.dim() < 3:
        raise _lib.TmfError(f"cam shapes: act {tuple(act.shape)} grad {tuple(grad.shape)}")
    B, C = act.shape[0], act.shape[-1]
    V = act.numel() // (B * C) if B * C else 0
    code = CAM_METHODS[method]
    nws = _lib.query("tmf_cam_workspace_bytes", B, V, C, code)
    if nws == 0:
        raise _lib.TmfError(f"tmf_cam takes no activation of shape {tuple(act.shape)} (C a multiple of 4 in 8..512)")
    ws = torch.empty(nws, device=act.device, dtype=torch.uint8)
    out = torch.empty(act.shape[:-1], device=act.device, dtype=_f32)
    weights = torch.empty((B, C), device=act.device, dtype=_f32) if code == _lib.CAM_GRAD else None
    peak = torch.empty((B,), device=act.device, dtype=_f32)
    flags = (_lib.CAM_RELU if relu else 0) | (_lib.CAM_NORMALIZE if normalize else 0)
    _lib.call("tmf_cam", act.data_ptr(), grad.data_ptr(), out.data_ptr(), _ptr(weights), peak.data_ptr(), ws.data_ptr(), nws,
              B, V, C, code, flags, _stream())
    return out, weights, peak


# --------------------------------------------------------------------------------------
# occlusion sensitivity (csrc/occlusion.hip; include/tmf_hip.h states the window grid, the jobs and the voxel map)
# --------------------------------------------------------------------------------------

def occlusion_grid(size, patch, stride):
    """(nd, nh, nw): per axis n = ceil(max(S - p, 0) / s) + 1 windows; ValueError unless 1 <= s <= p and S >= 1."""
    size, patch, stride = tuple(size), tuple(patch), tuple(stride)
    if not (len(size) == len(patch) == len(stride) == 3):
        raise ValueError(f"size, patch and stride are three numbers each, got {size}, {patch}, {stride}")
    for S, p, s in zip(size, patch, stride):
        if not all(_is_int(v) for v in (S, p, s)) or S < 1 or p < 1:
            raise ValueError(f"extents and patches are positive integers, got size {size}, patch {patch}, stride {stride}")
        if not 1 <= s <= p:
            raise ValueError(f"stride {stride} must lie in 1..patch {patch} on every axis: voxels would lie in no window")
    return tuple(-(-max(S - p, 0) // s) + 1 for S, p, s in zip(size, patch, stride))


def occlusion_window(size, patch, stride, w):
    """The three slices of window w = (id*nh + ih)*nw + iw: [i*s, min(i*s + p, S)) per axis."""
    _nd, nh, nw = occlusion_grid(size, patch, stride)
    idx = (w // (nh * nw), w // nw % nh, w % nw)
    return tuple(slice(i * s, min(i * s + p, S)) for i, S, p, s in zip(idx, size, patch, stride))


def occlusion_ok(*tensors):
    """The occlusion kernels take these: contiguous float32 (int32 for labels) tensors on one HIP device, none empty."""
    return _kernel_takes(*((t, (_f32, torch.int32)) for t in tensors))


def _job_buffer(vol, K, out):
    """The (K, ...) buffer a chunk of K jobs on the rows of vol (B, ...) is written to: `out` if it fits, a new one for None."""
    shape = (K,) + tuple(vol.shape[1:])
    if out is None:
        return torch.empty(shape, device=vol.device, dtype=vol.dtype)
    if tuple(out.shape) != shape or out.dtype != vol.dtype or out.device != vol.device:
        raise ValueError(f"out must be {shape} {vol.dtype} on {vol.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    return out


def _job_range(B, nW, j0, K):
    """Jobs j0 .. j0+K-1 lie among the B * nW jobs, or ValueError."""
    if not (K >= 1 and j0 >= 0 and j0 + K <= B * nW):
        raise ValueError(f"jobs {j0} .. {j0 + K - 1} of {B * nW}")


def _occlude_args(vol, fill, nW, j0, K, out, labels=None):
    """The checks of occlude_windows and occlude_labels (nW = R) -> the (K, ...) buffer to write."""
    B, size = vol.shape[0], tuple(vol.shape[-3:])
    if labels is not None and (tuple(labels.shape) != size or labels.dtype.is_floating_point or nW < 1):
        raise ValueError(f"labels must be integers of shape {size} and R >= 1, got {tuple(labels.shape)} {labels.dtype}, R = {nW}")
    _job_range(B, nW, j0, K)
    out = _job_buffer(vol, K, out)
    if tuple(fill.shape) != (B,):
        raise ValueError(f"fill must be ({B},), got {tuple(fill.shape)}")
    return out


def _occlude_windows_rows(vol, fill, patch, stride, nW, j0, K, out):
    size = tuple(vol.shape[-3:])
    jobs = torch.arange(j0, j0 + K, device=vol.device)
    out.copy_(vol.index_select(0, jobs // nW))
    for k in range(K):
        b, w = divmod(j0 + k, nW)
        out[k][(..., *occlusion_window(size, patch, stride, w))] = fill[b]
    return out


def occlude_windows_torch(vol, fill, patch, stride, j0, K, out=None):
    """occlude_windows in plain torch ops on whatever device and dtype vol has: the samples' rows copied, then one slice
    assignment of fill[b], cast to vol's dtype, per job."""
    nW = math.prod(occlusion_grid(tuple(vol.shape[-3:]), patch, stride))
    return _occlude_windows_rows(vol, fill, patch, stride, nW, j0, K, _occlude_args(vol, fill, nW, j0, K, out))


def occlude_windows(vol, fill, patch, stride, j0, K, out=None):
    """out[k] = vol[(j0+k) // nW] with window (j0+k) % nW of its last three axes set to fill[(j0+k) // nW]: vol (B, ..., D, H, W),
    fill (B,) -> (K, ..., D, H, W), the bits of clone() plus slice assignment.  Contiguous float32 HIP tensors: ONE launch
    (tmf_occlude_windows); anything else: occlude_windows_torch.  out: a buffer to write into (contiguous for the kernel)."""
    B, size = vol.shape[0], tuple(vol.shape[-3:])
    nW = math.prod(occlusion_grid(size, patch, stride))
    out = _occlude_args(vol, fill, nW, j0, K, out)
    if not (_kernel_takes((vol, _f32), (fill, _f32), (out, _f32))
            and vol.numel() == B * size[0] * size[1] * size[2]):           # one channel: (B, 1, D, H, W) or (B, D, H, W)
        return _occlude_windows_rows(vol, fill, patch, stride, nW, j0, K, out)
    _chk(vol, "vol")
    _lib.call("tmf_occlude_windows", vol.data_ptr(), fill.data_ptr(), out.data_ptr(), B, *size, *patch, *stride, j0, K, _stream())
    return out


def _occlude_labels_rows(vol, labels, fill, R, j0, K, out):
    labels = labels.to(vol.device)
    for k in range(K):
        b, r = divmod(j0 + k, R)
        out[k] = torch.where(labels == r + 1, fill[b], vol[b])
    return out


def occlude_labels_torch(vol, labels, fill, R, j0, K, out=None):
    """occlude_labels in plain torch ops on whatever device and dtype vol has: one torch.where per job, fill[b] cast to vol's
    dtype."""
    return _occlude_labels_rows(vol, labels, fill, R, j0, K, _occlude_args(vol, fill, R, j0, K, out, labels))


def occlude_labels(vol, labels, fill, R, j0, K, out=None):
    """occlude_windows with regions: job (j0+k) = b*R + (r-1) sets the voxels of sample b whose label (labels (D, H, W),
    integers) is r to fill[b]; label 0 and labels outside 0..R occlude nothing.  Kernel: tmf_occlude_labels (int32 labels);
    anything else: occlude_labels_torch."""
    out = _occlude_args(vol, fill, R, j0, K, out, labels)
    B = vol.shape[0]
    if not (_kernel_takes((vol, _f32), (fill, _f32), (out, _f32), (labels, torch.int32)) and vol.numel() == B * labels.numel()):
        return _occlude_labels_rows(vol, labels, fill, R, j0, K, out)
    _chk(vol, "vol")
    _lib.call("tmf_occlude_labels", vol.data_ptr(), labels.data_ptr(), fill.data_ptr(), out.data_ptr(), B, *labels.shape, R, j0, K,
              _stream())
    return out


def occlusion_volume_torch(drops, size, patch=None, stride=None, labels=None):
    """occlusion_volume in plain torch ops on whatever device and dtype the drops have: a scatter-add per window in ascending w
    and one division by the count; labels: a lookup."""
    size = tuple(size)
    B, nW = drops.shape
    if labels is not None:
        lab = labels.to(drops.device).long()
        picked = drops[:, (lab - 1).clamp(0, nW - 1).reshape(-1)].view((B,) + size)
        return torch.where((lab >= 1) & (lab <= nW), picked, torch.zeros((), device=drops.device, dtype=drops.dtype))
    acc = torch.zeros((B,) + size, device=drops.device, dtype=drops.dtype)
    cnt = torch.zeros(size, device=drops.device, dtype=drops.dtype)
    for w in range(nW):
        win = occlusion_window(size, patch, stride, w)
        acc[(slice(None), *win)] += drops[:, w].view(B, 1, 1, 1)
        cnt[win] += 1
    return acc / cnt


def occlusion_volume(drops, size, patch=None, stride=None, labels=None):
    """The drops back on the voxel grid -> (B, D, H, W).  Grid (drops (B, nW), patch, stride): the mean of drops[b, w] over the
    windows that contain the voxel, summed in ascending w, one division by the count.  labels (D, H, W) (drops (B, R)):
    drops[b, label - 1], 0 on background and on labels outside 1..R.  Contiguous float32 HIP drops (int32 labels): ONE launch
    (tmf_occlusion_volume / tmf_occlusion_volume_labels), a gather without atomics; anything else: torch ops in the same order."""
    size = tuple(size)
    B, nW = drops.shape
    if labels is None:
        grid = occlusion_grid(size, patch, stride)
        if nW != grid[0] * grid[1] * grid[2]:
            raise ValueError(f"drops {tuple(drops.shape)} do not belong to the {grid} windows of {size}")
        if _kernel_takes((drops, _f32)):
            _chk(drops, "drops")
            vmap = torch.empty((B,) + size, device=drops.device, dtype=_f32)
            _lib.call("tmf_occlusion_volume", drops.data_ptr(), vmap.data_ptr(), B, *size, *patch, *stride, _stream())
            return vmap
        return occlusion_volume_torch(drops, size, patch, stride)
    if tuple(labels.shape) != size or labels.dtype.is_floating_point:
        raise ValueError(f"labels must be integers of shape {size}, got {tuple(labels.shape)} {labels.dtype}")
    if _kernel_takes((drops, _f32), (labels, torch.int32)):
        _chk(drops, "drops")
        vmap = torch.empty((B,) + size, device=drops.device, dtype=_f32)
        _lib.call("tmf_occlusion_volume_labels", drops.data_ptr(), labels.data_ptr(), vmap.data_ptr(), B, *size, nW, _stream())
        return vmap
    return occlusion_volume_torch(drops, size, labels=labels)


# --------------------------------------------------------------------------------------
# RISE saliency maps (csrc/rise.hip; include/tmf_hip.h states the geometry, the mask value, the nodes and shifts, the jobs and the map)
# --------------------------------------------------------------------------------------

RISE_KEY = (0x52495345, 0x6D61736B)      # XORed into the two halves of the seed


def _cells3(cells):
    c = (cells,) * 3 if _is_int(cells) else tuple(cells) if isinstance(cells, (tuple, list)) else None
    if c is None or len(c) != 3 or any(not _is_int(x) for x in c):
        raise ValueError(f"cells must be an int or three of them, got {cells!r}")
    return c


def rise_geometry(size, cells):
    """-> (cell (c_d, c_h, c_w), nodes (n_d, n_h, n_w), the bytes of one node grid): per axis c = ceil(S / s), n = s + 2
    (tmf_rise_geometry computes the same); ValueError unless 1 <= s <= S on every axis."""
    size, cells = tuple(int(s) for s in size), _cells3(cells)
    if len(size) != 3 or any(S < 1 for S in size):
        raise ValueError(f"size must be three positive extents, got {size}")
    if any(not 1 <= s <= S for S, s in zip(size, cells)):
        raise ValueError(f"cells {cells} must lie in 1..extent {size} on every axis")
    nodes = tuple(s + 2 for s in cells)
    return tuple(-(-S // s) for S, s in zip(size, cells)), nodes, nodes[0] * nodes[1] * nodes[2]


def rise_ok(*tensors):
    """The RISE kernels take these: contiguous float32 (uint8 nodes, int32 shifts) tensors on one HIP device, none empty."""
    return _kernel_takes(*((t, (_f32, torch.uint8, torch.int32)) for t in tensors))


def _rise_mask_args(size, cells, p, seed, m0, N):
    geom = rise_geometry(size, cells)
    if not isinstance(p, (int, float)) or isinstance(p, bool) or not 0.0 < float(p) < 1.0:
        raise ValueError(f"p must lie in (0, 1), got {p!r}")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    if not (_is_int(m0) and _is_int(N) and N >= 1 and m0 >= 0 and m0 + N < 1 << 31):
        raise ValueError(f"masks m0 = {m0!r}, N = {N!r}")
    return geom


def _rise_masks_host(cell, nodes, G, p, seed, m0, N):
    """The node bytes and shifts as the header defines them, in numpy on the host: what rise_masks_torch falls back to where
    no HIP device can run tmf_rise_masks."""
    import numpy as np
    u64, mask32 = np.uint64, np.uint64(0xFFFFFFFF)

    def philox(c0, c1, c2, c3):
        c0, c1, c2, c3 = (np.asarray(c, dtype=u64) for c in np.broadcast_arrays(c0, c1, c2, c3))
        k0, k1 = u64((seed & 0xFFFFFFFF) ^ RISE_KEY[0]), u64((seed >> 32) ^ RISE_KEY[1])
        for _ in range(10):
            p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2
            c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & mask32, (p0 >> u64(32)) ^ c3 ^ k1, p0 & mask32
            k0, k1 = (k0 + u64(0x9E3779B9)) & mask32, (k1 + u64(0xBB67AE85)) & mask32
        return np.stack([c0, c1, c2, c3], -1)

    m = np.arange(m0, m0 + N, dtype=u64)
    nq = (G + 3) // 4
    words = philox(np.arange(nq, dtype=u64)[None, :], m[:, None], 0, 0).reshape(N, nq * 4)[:, :G]
    thr = np.float32(p) * np.float32(16777216.0)
    grid = ((words >> u64(8)).astype(np.float32) < thr).astype(np.uint8).reshape((N,) + tuple(nodes))
    sw = philox(0, m, 1, 0)[:, :3]
    shifts = ((sw * np.asarray(cell, dtype=u64)) >> u64(32)).astype(np.int32)
    return torch.from_numpy(grid), torch.from_numpy(shifts)


def rise_masks(size, cells, p, seed, m0, N, device):
    """nodes (N, n_d, n_h, n_w) uint8 and shifts (N, 3) int32 of masks m0 .. m0+N-1 on `device`: a pure function of (seed, m,
    geometry, p).  A HIP device: ONE launch (tmf_rise_masks); anything else: rise_masks_torch."""
    device = torch.device(device)
    if device.type != "cuda":
        return rise_masks_torch(size, cells, p, seed, m0, N, device)
    _cell, nn, _G = _rise_mask_args(size, cells, p, seed, m0, N)
    with torch.cuda.device(device):
        nodes = torch.empty((N,) + nn, device=device, dtype=torch.uint8)
        shifts = torch.empty((N, 3), device=device, dtype=torch.int32)
        _lib.call("tmf_rise_masks", nodes.data_ptr(), shifts.data_ptr(), *tuple(size), *_cells3(cells), float(p), seed, m0, N,
                  _stream())
    return nodes, shifts


def rise_masks_torch(size, cells, p, seed, m0, N, device=None):
    """rise_masks for any device: the nodes and shifts come from the library where a HIP device can run it (then copied to
    `device`), else from the same Philox4x32-10 restated in numpy on the host - the same bytes either way."""
    device = torch.device("cpu" if device is None else device)
    if torch.cuda.is_available():
        nodes, shifts = rise_masks(size, cells, p, seed, m0, N, device if device.type == "cuda" else torch.device("cuda"))
        return nodes.to(device), shifts.to(device)
    cell, nn, G = _rise_mask_args(size, cells, p, seed, m0, N)
    nodes, shifts = _rise_masks_host(cell, nn, G, p, seed, m0, N)
    return nodes.to(device), shifts.to(device)


def _rise_args(nodes, shifts, size, cells):
    cell, nn, _G = rise_geometry(size, cells)
    N = nodes.shape[0]
    if nodes.dtype != torch.uint8 or tuple(nodes.shape) != (N,) + nn or N < 1:
        raise ValueError(f"nodes must be uint8 (N, {nn[0]}, {nn[1]}, {nn[2]}), got {tuple(nodes.shape)} {nodes.dtype}")
    if shifts.dtype != torch.int32 or tuple(shifts.shape) != (N, 3):
        raise ValueError(f"shifts must be int32 ({N}, 3), got {tuple(shifts.shape)} {shifts.dtype}")
    return cell, N


def rise_mask_values(nodes, shifts, size, cells, dtype=_f32):
    """M of every mask in nodes / shifts on the voxel grid -> (n, D, H, W): THE formula of the header, op by op - W first, then
    H, then D, every product and sum a torch op of its own.  float32: w1 = float(r) * (1.0f / float(c)), the kernels' bits;
    float64: w1 = r / c, M_exact.  Any other floating dtype: the float32 values cast."""
    import numpy as np
    cell, _N = _rise_args(nodes, shifts, size, cells)
    exact = dtype == torch.float64
    ct = torch.float64 if exact else _f32
    dev = nodes.device
    idx, w0, w1 = [], [], []
    for a in range(3):
        q = torch.arange(size[a], device=dev).view(1, -1) + shifts[:, a:a + 1].to(device=dev, dtype=torch.long)     # (n, S)
        i = q // cell[a]
        r = (q - i * cell[a]).to(ct)
        w = r / cell[a] if exact else r * float(np.float32(1.0) / np.float32(cell[a]))
        shape = [-1, 1, 1, 1]
        shape[a + 1] = size[a]
        idx.append(i.view(shape))
        w1.append(w.view(shape))
        w0.append((1.0 - w).view(shape))
    m = torch.arange(nodes.shape[0], device=dev).view(-1, 1, 1, 1)
    g = lambda a, b, c: nodes[m, idx[0] + a, idx[1] + b, idx[2] + c].to(ct)
    x = [[g(a, b, 0) * w0[2] + g(a, b, 1) * w1[2] for b in (0, 1)] for a in (0, 1)]
    y = [x[a][0] * w0[1] + x[a][1] * w1[1] for a in (0, 1)]
    M = y[0] * w0[0] + y[1] * w1[0]
    return M if M.dtype == dtype else M.to(dtype)


def _rise_apply_args(vol, nodes, shifts, fill, size, cells, j0, K, base, out):
    _cell, N = _rise_args(nodes, shifts, size, cells)
    B = vol.shape[0]
    if tuple(vol.shape[-3:]) != tuple(size) or vol.numel() != B * size[0] * size[1] * size[2]:
        raise ValueError(f"vol must be a one-channel volume (B, 1, D, H, W) or (B, D, H, W) of {tuple(size)} voxels, got {tuple(vol.shape)}")
    if base is not None and tuple(base.shape) != tuple(vol.shape):
        raise ValueError(f"base must have vol's shape {tuple(vol.shape)}, got {tuple(base.shape)}")
    if base is None and (fill is None or tuple(fill.shape) != (B,)):
        raise ValueError(f"fill must be ({B},), got {None if fill is None else tuple(fill.shape)}")
    _job_range(B, N, j0, K)
    return _job_buffer(vol, K, out), N


def _rise_apply_rows(vol, nodes, shifts, fill, size, cells, N, j0, K, base, out):
    jobs = torch.arange(j0, j0 + K, device=vol.device)
    b, m = jobs // N, (jobs % N).to(nodes.device)
    dtype = torch.float64 if vol.dtype == torch.float64 else _f32
    M = rise_mask_values(nodes.index_select(0, m), shifts.index_select(0, m), size, cells, dtype).to(vol.device)
    M = M.view((K,) + (1,) * (vol.dim() - 4) + tuple(size))
    v = vol.index_select(0, b).to(dtype)
    f = base.index_select(0, b).to(dtype) if base is not None else fill.index_select(0, b).to(dtype).view((K,) + (1,) * (vol.dim() - 1))
    out.copy_(f + M * (v - f))
    return out


def rise_apply_torch(vol, nodes, shifts, fill, size, cells, j0, K, base=None, out=None):
    """rise_apply in plain torch ops on whatever device and floating dtype vol has: f + M * (vol - f) with rise_mask_values
    (float32, or float64 for a float64 vol), three torch ops."""
    out, N = _rise_apply_args(vol, nodes, shifts, fill, size, cells, j0, K, base, out)
    return _rise_apply_rows(vol, nodes, shifts, fill, size, cells, N, j0, K, base, out)


def rise_apply(vol, nodes, shifts, fill, size, cells, j0, K, base=None, out=None):
    """out[k] = f + M_m * (vol[b] - f) for job j0 + k = b*N + m: vol (B, 1, D, H, W) or (B, D, H, W), nodes / shifts of masks
    0..N-1, f = base[b] (a tensor of vol's shape) where given, else fill[b] (fill (B,)) -> (K, ...) of vol's shape.  Contiguous
    float32 HIP tensors: ONE launch (tmf_rise_apply); anything else: rise_apply_torch, the same bits in float32."""
    out, N = _rise_apply_args(vol, nodes, shifts, fill, size, cells, j0, K, base, out)
    if not (rise_ok(vol, nodes, shifts, base if base is not None else fill, out) and vol.dtype == _f32 and out.dtype == _f32
            and (base if base is not None else fill).dtype == _f32):
        return _rise_apply_rows(vol, nodes, shifts, fill, size, cells, N, j0, K, base, out)
    _chk(vol, "vol")
    _lib.call("tmf_rise_apply", vol.data_ptr(), nodes.data_ptr(), shifts.data_ptr(), _ptr(None if base is not None else fill),
              _ptr(base), out.data_ptr(), vol.shape[0], *tuple(size), *_cells3(cells), N, j0, K, _stream())
    return out


def _rise_accumulate_args(scores, nodes, shifts, size, cells, m_first, m_step):
    _cell, N = _rise_args(nodes, shifts, size, cells)
    if scores.dim() != 2 or scores.shape[1] != N or scores.shape[0] < 1 or not scores.dtype.is_floating_point:
        raise ValueError(f"scores must be floating-point (B, {N}), got {tuple(scores.shape)} {scores.dtype}")
    if not (_is_int(m_first) and _is_int(m_step) and m_step >= 1 and 0 <= m_first < N):
        raise ValueError(f"masks m_first = {m_first!r}, m_step = {m_step!r} of {N}")
    return N


def rise_accumulate_torch(scores, nodes, shifts, size, cells, scale=1.0, m_first=0, m_step=1, chunk=64):
    """rise_accumulate in plain torch ops on whatever device and floating dtype the scores have: a matmul of the scores with
    rise_mask_values, `chunk` rebuilt masks at a time, then one multiplication by scale.  float64 scores: M_exact and fp64 sums,
    the reference of the bound."""
    N = _rise_accumulate_args(scores, nodes, shifts, size, cells, m_first, m_step)
    B, size = scores.shape[0], tuple(size)
    dtype = torch.float64 if scores.dtype == torch.float64 else _f32
    ms = torch.arange(m_first, N, m_step, device=nodes.device)
    acc = torch.zeros((B, size[0] * size[1] * size[2]), device=scores.device, dtype=dtype)
    for lo in range(0, ms.numel(), chunk):
        m = ms[lo:lo + chunk]
        M = rise_mask_values(nodes.index_select(0, m), shifts.index_select(0, m), size, cells, dtype).to(scores.device)
        acc += scores.index_select(1, m.to(scores.device)).to(dtype) @ M.view(m.numel(), -1)
    return (acc * scale).to(scores.dtype).view((B,) + size)


def rise_accumulate(scores, nodes, shifts, size, cells, scale=1.0, m_first=0, m_step=1):
    """sal[b] = scale * sum_m scores[b, m] * M_m over m = m_first, m_first + m_step, ... < N: scores (B, N) -> (B, D, H, W), an
    fp32 chain in ascending m and one multiplication by scale.  Contiguous float32 HIP scores: ONE launch (tmf_rise_accumulate),
    every mask rebuilt in registers, no atomics, two calls give the same bits; anything else: rise_accumulate_torch."""
    N = _rise_accumulate_args(scores, nodes, shifts, size, cells, m_first, m_step)
    if not (rise_ok(scores, nodes, shifts) and scores.dtype == _f32):
        return rise_accumulate_torch(scores, nodes, shifts, size, cells, scale, m_first, m_step)
    _chk(scores, "scores")
    B, size = scores.shape[0], tuple(size)
    sal = torch.empty((B,) + size, device=scores.device, dtype=_f32)
    _lib.call("tmf_rise_accumulate", scores.data_ptr(), nodes.data_ptr(), shifts.data_ptr(), sal.data_ptr(), float(scale), B, *size,
              *_cells3(cells), N, m_first, m_step, _stream())
    return sal


# --------------------------------------------------------------------------------------
# atlas-region Shapley values (csrc/shap.hip; include/tmf_hip.h states the players, the coalitions, the jobs, the fit and the solve)
# --------------------------------------------------------------------------------------

SHAP_KEY = (0x53484150, 0x636F616C)      # XORed into the two halves of the seed
SHAP_MAX_PLAYERS = _lib.SHAP_MAX_PLAYERS


def shap_ok(*tensors):
    """The Shapley kernels take these: contiguous float32 (int32 labels, coalitions and A, float64 rhs and delta) tensors on one
    HIP device, none empty."""
    return _kernel_takes(*((t, (_f32, torch.int32, torch.float64)) for t in tensors))


def _shap_players(P):
    return _int(P, f"P must be an integer in 2..{SHAP_MAX_PLAYERS} players", 2, SHAP_MAX_PLAYERS)


def shap_size_table_torch(P):
    """thr (max(P - 2, 0),) int64 with values in 0..2^32-1, restated in numpy: w_r = 1 / (r (P - r)), F_s the ascending fp64
    partial sum over the ascending total, thr[t] = min(2^32 - 1, floor(2^32 F_{t+1}))."""
    import numpy as np
    P = _shap_players(P)
    total = part = np.float64(0.0)
    for r in range(1, P):
        total = total + np.float64(1.0) / (np.float64(r) * np.float64(P - r))
    thr = np.empty(max(P - 2, 0), np.int64)
    for t in range(P - 2):
        part = part + np.float64(1.0) / (np.float64(t + 1) * np.float64(P - t - 1))
        thr[t] = min(2 ** 32 - 1, int(np.floor(np.float64(4294967296.0) * (part / total))))
    return torch.from_numpy(thr)


def shap_size_table(P):
    """thr (max(P - 2, 0),) int64 with values in 0..2^32-1 from the library's host entry tmf_shap_size_table."""
    P = _shap_players(P)
    thr = (ctypes.c_uint32 * max(P - 2, 1))()
    _lib.call("tmf_shap_size_table", P, thr)
    return torch.tensor(list(thr)[:P - 2], dtype=torch.int64)


def _shap_coalition_args(P, paired, seed, m0, N):
    _shap_players(P)
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"seed must be an integer in 0..2^64-1, got {seed!r}")
    if not (_is_int(m0) and _is_int(N) and N >= 1 and m0 >= 0 and m0 + N < 1 << 31):
        raise ValueError(f"coalitions m0 = {m0!r}, N = {N!r}")
    return (P + 31) // 32


def _shap_bits32(words):
    """uint32 values held in an int64 tensor / array -> the int32 tensor with the same bits."""
    import numpy as np
    return torch.from_numpy(np.asarray(words, dtype=np.int64).astype(np.uint32).view(np.int32))


def _shap_coalitions_host(P, paired, seed, m0, N):
    """The rows as the header defines them, in numpy on the host -> (N, Wd) int32 (the bits of the uint32 words)."""
    import numpy as np
    u64, mask32 = np.uint64, np.uint64(0xFFFFFFFF)

    def philox(c0, c1, c2, c3):
        c0, c1, c2, c3 = (np.asarray(c, dtype=u64) for c in np.broadcast_arrays(c0, c1, c2, c3))
        k0, k1 = u64((seed & 0xFFFFFFFF) ^ SHAP_KEY[0]), u64((seed >> 32) ^ SHAP_KEY[1])
        for _ in range(10):
            p0, p1 = u64(0xD2511F53) * c0, u64(0xCD9E8D57) * c2
            c0, c1, c2, c3 = (p1 >> u64(32)) ^ c1 ^ k0, p1 & mask32, (p0 >> u64(32)) ^ c3 ^ k1, p0 & mask32
            k0, k1 = (k0 + u64(0x9E3779B9)) & mask32, (k1 + u64(0xBB67AE85)) & mask32
        return np.stack([c0, c1, c2, c3], -1)

    Wd = (P + 31) // 32
    m = np.arange(m0, m0 + N)
    k = m >> 1 if paired else m
    ks = np.arange(k[0], k[-1] + 1, dtype=u64)
    u = philox(0, ks, 1, 0)[:, 0]
    s = 1 + np.searchsorted(shap_size_table_torch(P).numpy().astype(u64), u, side="right")     # #{t : thr[t] <= u}
    nq = (P + 3) // 4
    keys = philox(np.arange(nq, dtype=u64)[None, :], ks[:, None], 0, 0).reshape(len(ks), nq * 4)[:, :P]
    order = np.argsort(keys, axis=1, kind="stable")                                              # ties by index
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(P), order.shape), 1)
    z = (rank < s[:, None])[k - k[0]]
    if paired:
        z = np.where((m & 1)[:, None] == 1, ~z, z)
    bits = np.zeros((N, Wd * 32), np.int64)
    bits[:, :P] = z
    words = (bits.reshape(N, Wd, 32) << np.arange(32, dtype=np.int64)).sum(2)
    return _shap_bits32(words)


def shap_coalitions_torch(P, paired, seed, m0, N, device=None):
    """shap_coalitions restated in numpy on the host (Philox4x32-10, the size table, ranks by a stable sort), then moved to
    `device`: the same bits as the kernel's."""
    _shap_coalition_args(P, paired, seed, m0, N)
    return _shap_coalitions_host(P, bool(paired), seed, m0, N).to(torch.device("cpu" if device is None else device))


def shap_coalitions(P, paired, seed, m0, N, device):
    """(N, Wd) int32, the bits of rows m0 .. m0+N-1 of the coalition sampler: player i is bit i & 31 of word i >> 5.  A pure
    function of (seed, m, P, paired).  A HIP device: ONE launch (tmf_shap_coalitions); anything else: shap_coalitions_torch."""
    device = torch.device(device)
    if device.type != "cuda":
        return shap_coalitions_torch(P, paired, seed, m0, N, device)
    Wd = _shap_coalition_args(P, paired, seed, m0, N)
    with torch.cuda.device(device):
        thr = _shap_bits32(shap_size_table(P).numpy()).to(device) if P > 2 else None
        coal = torch.empty((N, Wd), device=device, dtype=torch.int32)
        _lib.call("tmf_shap_coalitions", coal.data_ptr(), _ptr(thr), P, 1 if paired else 0, seed, m0, N, _stream())
    return coal


def shap_unpack(coal, P):
    """(N, Wd) int32 rows -> (N, P) bool: z[m, i] = player i is in coalition m."""
    i = torch.arange(P, device=coal.device)
    return ((coal.long()[:, i >> 5] >> (i & 31)) & 1).bool()


def _shap_apply_args(vol, labels, coal, fill, R, p0, P, j0, K, base, out):
    B, size = vol.shape[0], tuple(vol.shape[-3:])
    _shap_players(P)
    if tuple(labels.shape) != size or labels.dtype.is_floating_point:
        raise ValueError(f"labels must be integers of shape {size}, got {tuple(labels.shape)} {labels.dtype}")
    if not (_is_int(R) and _is_int(p0) and R >= 1 and p0 >= 0 and p0 + R <= P):
        raise ValueError(f"players p0 = {p0!r}, R = {R!r} of {P}")
    if coal.dim() != 2 or coal.dtype != torch.int32 or coal.shape[0] < 1 or coal.shape[1] != (P + 31) // 32:
        raise ValueError(f"coalitions must be (N, {(P + 31) // 32}) int32, got {tuple(coal.shape)} {coal.dtype}")
    N = coal.shape[0]
    _job_range(B, N, j0, K)
    out = _job_buffer(vol, K, out)
    if base is None and (fill is None or tuple(fill.shape) != (B,)):
        raise ValueError(f"fill must be ({B},), got {None if fill is None else tuple(fill.shape)}")
    if base is not None and tuple(base.shape) != tuple(vol.shape):
        raise ValueError(f"base must be {tuple(vol.shape)}, got {tuple(base.shape)}")
    return out, N


def _shap_apply_rows(vol, labels, coal, fill, R, p0, N, j0, K, base, out):
    lab = labels.to(vol.device).long()
    coal = coal.to(vol.device).long()
    has = (lab >= 1) & (lab <= R)
    player = torch.where(has, p0 + lab - 1, torch.zeros_like(lab))
    word, bit = player >> 5, player & 31
    for k in range(K):
        b, m = divmod(j0 + k, N)
        keep = ~has | ((coal[m][word] >> bit) & 1).bool()
        out[k] = torch.where(keep, vol[b], base[b] if base is not None else fill[b])
    return out


def shap_apply_torch(vol, labels, coal, fill, R, p0, P, j0, K, base=None, out=None):
    """shap_apply in plain torch ops on whatever device and dtype vol has: one torch.where per job."""
    out, N = _shap_apply_args(vol, labels, coal, fill, R, p0, P, j0, K, base, out)
    return _shap_apply_rows(vol, labels, coal, fill, R, p0, N, j0, K, base, out)


def shap_apply(vol, labels, coal, fill, R, p0, P, j0, K, base=None, out=None):
    """out[k] = sample b of vol (B, ..., D, H, W) under coalition row m of coal (N, Wd), job j0 + k = b*N + m: a voxel with
    label l in 1..R keeps its value where bit p0 + l - 1 of the row is set and takes base[b] (where given, else fill[b])
    otherwise; background and labels outside 1..R are never replaced -> (K, ..., D, H, W).  Contiguous float32 HIP tensors
    (int32 labels and coalitions): ONE launch (tmf_shap_apply); anything else: shap_apply_torch, the same bits."""
    out, N = _shap_apply_args(vol, labels, coal, fill, R, p0, P, j0, K, base, out)
    B = vol.shape[0]
    if not (shap_ok(vol, labels, coal, base if base is not None else fill, out) and vol.dtype == _f32 and out.dtype == _f32
            and labels.dtype == torch.int32 and (base if base is not None else fill).dtype == _f32
            and vol.numel() == B * labels.numel()):
        return _shap_apply_rows(vol, labels, coal, fill, R, p0, N, j0, K, base, out)
    _chk(vol, "vol")
    _lib.call("tmf_shap_apply", vol.data_ptr(), labels.data_ptr(), coal.data_ptr(), _ptr(None if base is not None else fill),
              _ptr(base), out.data_ptr(), B, *labels.shape, R, p0, P, N, j0, K, _stream())
    return out


def _shap_gram_args(coal, scores, offset, P):
    _shap_players(P)
    if coal.dim() != 2 or coal.dtype != torch.int32 or coal.shape[0] < 1 or coal.shape[1] != (P + 31) // 32:
        raise ValueError(f"coalitions must be (N, {(P + 31) // 32}) int32, got {tuple(coal.shape)} {coal.dtype}")
    N = coal.shape[0]
    if scores.dim() != 2 or scores.shape[1] != N or scores.shape[0] < 1 or tuple(offset.shape) != (scores.shape[0],):
        raise ValueError(f"scores must be (B, {N}) and offset (B,), got {tuple(scores.shape)} and {tuple(offset.shape)}")
    return scores.shape[0], N


def shap_gram_torch(coal, scores, offset, P):
    """shap_gram in plain torch ops on whatever device the scores have: the unpacked bits, two fp64 matrix products (A is exact:
    its entries are counts below 2^31)."""
    _shap_gram_args(coal, scores, offset, P)
    z = shap_unpack(coal.to(scores.device), P).double()
    y = scores.double() - offset.double().view(-1, 1)
    return (z.t() @ z).to(torch.int32), y @ z


def shap_gram(coal, scores, offset, P):
    """The normal equations of the fit: coal (N, Wd), scores (B, N), offset (B,) -> (A (P, P) int32 = sum_m z_m z_m^T, exact;
    rhs (B, P) float64 = sum_m z_mi (scores[b, m] - offset[b]), an ascending chain).  Contiguous float32 HIP scores: two
    launches (tmf_shap_gram), no atomics; anything else: shap_gram_torch."""
    B, N = _shap_gram_args(coal, scores, offset, P)
    if not (shap_ok(coal, scores, offset) and scores.dtype == _f32 and offset.dtype == _f32):
        return shap_gram_torch(coal, scores, offset, P)
    A = torch.empty((P, P), device=scores.device, dtype=torch.int32)
    rhs = torch.empty((B, P), device=scores.device, dtype=torch.float64)
    _lib.call("tmf_shap_gram", coal.data_ptr(), scores.data_ptr(), offset.data_ptr(), A.data_ptr(), rhs.data_ptr(), B, P, N, _stream())
    return A, rhs


def _shap_solve_args(A, rhs, delta, ridge):
    P = A.shape[-1]
    _shap_players(P)
    if tuple(A.shape) != (P, P) or A.dtype.is_floating_point or rhs.dim() != 2 or rhs.shape[1] != P or rhs.shape[0] < 1 \
            or tuple(delta.shape) != (rhs.shape[0],):
        raise ValueError(f"A must be integers ({P}, {P}), rhs (B, {P}) and delta (B,), got {tuple(A.shape)}, {tuple(rhs.shape)} "
                         f"and {tuple(delta.shape)}")
    if not isinstance(ridge, (int, float)) or isinstance(ridge, bool) or not (0.0 <= float(ridge) < math.inf):
        raise ValueError(f"ridge must be a finite number >= 0, got {ridge!r}")
    return rhs.shape[0], P


def shap_solve_torch(A, rhs, delta, ridge=0.0):
    """shap_solve with torch.linalg in float64 on whatever device A has: cholesky_ex, cholesky_solve, the closed form."""
    _B, P = _shap_solve_args(A, rhs, delta, ridge)
    M = A.double() + float(ridge) * torch.eye(P, device=A.device, dtype=torch.float64)
    L, info = torch.linalg.cholesky_ex(M)
    X = torch.cholesky_solve(torch.cat([rhs.double(), torch.ones((1, P), device=A.device, dtype=torch.float64)]).t(), L).t()
    xb, x1 = X[:-1], X[-1]
    phi = xb - x1 * ((xb.sum(1) - delta.double()) / x1.sum()).view(-1, 1)
    info = info.to(torch.int32).view(1)
    return torch.where(info == 0, phi, torch.full_like(phi, math.nan)), info


def shap_solve(A, rhs, delta, ridge=0.0):
    """The fit under the efficiency constraint: with M = A + ridge I, X = M^-1 [rhs_1 .. rhs_B, 1],
    phi_b = x_b - x_1 (sum x_b - delta_b) / sum x_1 -> (phi (B, P) float64, info (1,) int32: 0, or the 1-based index of the first
    pivot <= 0 of the Cholesky factorisation - A is singular - and phi all NaN).  Contiguous HIP tensors (int32 A, float64 rhs
    and delta): a fixed sequence of launches (tmf_shap_solve), no host read; anything else: shap_solve_torch."""
    B, P = _shap_solve_args(A, rhs, delta, ridge)
    if not (_kernel_takes((A, torch.int32), (rhs, torch.float64), (delta, torch.float64))):
        return shap_solve_torch(A, rhs, delta, ridge)
    nbytes = _lib.query("tmf_shap_solve_workspace", B, P)
    ws = torch.empty((nbytes,), device=A.device, dtype=torch.uint8)
    phi = torch.empty((B, P), device=A.device, dtype=torch.float64)
    info = torch.empty((1,), device=A.device, dtype=torch.int32)
    _lib.call("tmf_shap_solve", A.data_ptr(), rhs.data_ptr(), delta.data_ptr(), float(ridge), phi.data_ptr(), info.data_ptr(),
              ws.data_ptr(), nbytes, B, P, _stream())
    return phi, info


# --------------------------------------------------------------------------------------
# deletion / insertion curves (csrc/faithfulness.hip; include/tmf_hip.h states the ordering, the thresholds and the jobs)
# --------------------------------------------------------------------------------------

RANK_MODES = {"deletion": _lib.RANK_DELETION, "insertion": _lib.RANK_INSERTION}


def rank_counts(V, steps):
    """[n_1 .. n_steps], n_k = ceil(k*V / steps): the number of voxels step k removes at least.  Non-decreasing, each in
    1..V, n_steps = V; repeated where V < steps."""
    if not (_is_int(V) and _is_int(steps)) or V < 1 or not 1 <= steps <= _lib.RANK_MAX_STEPS:
        raise ValueError(f"V must be a positive integer and steps one in 1..{_lib.RANK_MAX_STEPS}, got V = {V!r}, steps = {steps!r}")
    return [-(-k * V // steps) for k in range(1, steps + 1)]


def faithfulness_ok(*tensors):
    """The kernels of csrc/faithfulness.hip take these: contiguous float32 tensors on one HIP device, none empty."""
    return _kernel_takes(*((t, _f32) for t in tensors))


def _rank_counts_checked(V, counts):
    counts = [int(c) for c in counts]
    S = len(counts)
    if not 1 <= S <= _lib.RANK_MAX_STEPS or counts[0] < 1 or counts[-1] > V or any(a > b for a, b in zip(counts, counts[1:])):
        raise ValueError(f"counts must be 1..{_lib.RANK_MAX_STEPS} non-decreasing numbers in 1..{V}, got {counts}")
    return counts


def _rank_args(attr, counts):
    B = attr.shape[0]
    V = attr.numel() // B if B else 0
    if B < 1 or V < 1:
        raise ValueError(f"attr must hold samples with voxels, got {tuple(attr.shape)}")
    return B, V, _rank_counts_checked(V, counts)


def _rank_thresholds_sorted(attr, B, counts):
    S = len(counts)
    a = attr.reshape(B, -1) + 0.0
    srt = a.sort(1, descending=True).values
    thr = srt.gather(1, torch.tensor(counts, device=a.device).view(1, S).expand(B, S) - 1)
    removed = torch.stack([(a >= thr[:, k:k + 1]).sum(1) for k in range(S)], 1).to(torch.int32)
    return thr, removed


def rank_thresholds_torch(attr, counts):
    """rank_thresholds in plain torch ops on whatever device and dtype attr has: sort(descending=True), a gather and >=."""
    B, _V, counts = _rank_args(attr, counts)
    return _rank_thresholds_sorted(attr, B, counts)


def rank_thresholds(attr, counts):
    """attr (B, ...) with V elements per sample, counts [S] (rank_counts) -> (thr (B, S) of attr's dtype, removed (B, S) int32):
    thr[b, k] = the counts[k]-th largest a = attr + 0.0 of sample b, removed[b, k] = the number of its voxels with a >= thr[b, k]
    (ties go together).  Contiguous float32 HIP tensors: a radix select without a sort (tmf_rank_thresholds); anything else:
    rank_thresholds_torch."""
    B, V, counts = _rank_args(attr, counts)
    if not _kernel_takes((attr, _f32)):
        return _rank_thresholds_sorted(attr, B, counts)
    _chk(attr, "attr")
    S = len(counts)
    thr = torch.empty((B, S), device=attr.device, dtype=_f32)
    removed = torch.empty((B, S), device=attr.device, dtype=torch.int32)
    nws = _lib.query("tmf_rank_workspace_bytes", B, V, S)
    ws = torch.empty((nws,), device=attr.device, dtype=torch.uint8)            # the entry zeroes it
    _lib.call("tmf_rank_thresholds", attr.data_ptr(), (ctypes.c_int * S)(*counts), thr.data_ptr(), removed.data_ptr(),
              ws.data_ptr(), nws, B, V, S, _stream())
    return thr, removed


def _mask_args(vol, attr, thr, fill, mode, j0, K, base, out):
    if mode not in RANK_MODES:
        raise ValueError(f"mode must be one of {tuple(RANK_MODES)}, got {mode!r}")
    B = vol.shape[0]
    if thr.dim() != 2 or thr.shape[0] != B or not 1 <= thr.shape[1] <= _lib.RANK_MAX_STEPS:
        raise ValueError(f"thr must be ({B}, S) with S in 1..{_lib.RANK_MAX_STEPS}, got {tuple(thr.shape)}")
    if attr.shape[0] != B or attr.numel() != vol.numel():
        raise ValueError(f"attr {tuple(attr.shape)} does not hold one value per voxel of vol {tuple(vol.shape)}")
    if base is not None and tuple(base.shape) != tuple(vol.shape):
        raise ValueError(f"base must have vol's shape {tuple(vol.shape)}, got {tuple(base.shape)}")
    if base is None and (fill is None or tuple(fill.shape) != (B,)):
        raise ValueError(f"fill must be ({B},), got {None if fill is None else tuple(fill.shape)}")
    _job_range(B, thr.shape[1] + 1, j0, K)
    return _job_buffer(vol, K, out)


def _mask_rows(vol, attr, thr, fill, mode, j0, K, base, out):
    S = thr.shape[1]
    a = attr.reshape(vol.shape) + 0.0
    for k in range(K):
        b, s = divmod(j0 + k, S + 1)
        m = a[b] >= thr[b, s - 1] if s else torch.zeros_like(a[b], dtype=torch.bool)
        g = base[b] if base is not None else fill[b].to(vol.dtype)
        out[k] = torch.where(m, g, vol[b]) if mode == "deletion" else torch.where(m, vol[b], g)
    return out


def mask_by_rank_torch(vol, attr, thr, fill, mode, j0, K, base=None, out=None):
    """mask_by_rank in plain torch ops on whatever device and dtype the tensors have: >= and one torch.where per job, fill[b]
    cast to vol's dtype."""
    return _mask_rows(vol, attr, thr, fill, mode, j0, K, base, _mask_args(vol, attr, thr, fill, mode, j0, K, base, out))


def mask_by_rank(vol, attr, thr, fill, mode, j0, K, base=None, out=None):
    """Job j0 + k = b*(S+1) + s, s in 0..S: m = (s > 0) & (attr[b] + 0.0 >= thr[b, s-1]); out[k] = where(m, f, vol[b]) for mode
    "deletion", where(m, vol[b], f) for "insertion", f = base[b] (a tensor of vol's shape) where given, else fill[b] (fill (B,)).
    vol, attr (B, ...) with the same number of elements, thr (B, S) -> (K, ...) of vol's shape.  Contiguous float32 HIP
    tensors: ONE launch (tmf_mask_by_rank); anything else: mask_by_rank_torch.  out: a buffer to write into."""
    out = _mask_args(vol, attr, thr, fill, mode, j0, K, base, out)
    if not faithfulness_ok(vol, attr, thr, base if base is not None else fill, out):
        return _mask_rows(vol, attr, thr, fill, mode, j0, K, base, out)
    _chk(vol, "vol")
    B = vol.shape[0]
    _lib.call("tmf_mask_by_rank", vol.data_ptr(), attr.data_ptr(), thr.data_ptr(), _ptr(None if base is not None else fill),
              _ptr(base), out.data_ptr(), B, vol.numel() // B, thr.shape[1], RANK_MODES[mode], j0, K, _stream())
    return out


# --------------------------------------------------------------------------------------
# atlas region statistics (csrc/region_stats.hip; include/tmf_hip.h states the bins, the outputs and the accuracy of the sums)
# --------------------------------------------------------------------------------------

REGION_MAX = _lib.REGION_MAX
REGION_MAX_CLASSES = _lib.REGION_MAX_CLASSES
REGION_FIELDS = ("count", "sum", "abs_sum", "pos_sum", "max", "argmax")


def region_ok(*tensors):
    """The kernels of csrc/region_stats.hip take these: contiguous float32 (int32 labels, int64 classes, float64 state) tensors
    on one HIP device, none empty."""
    return _kernel_takes(*((t, (_f32, torch.int32, torch.int64, torch.float64)) for t in tensors))


def _region_args(a, labels, R):
    if a.dim() != 2 or a.shape[0] < 1 or a.shape[1] < 1 or not a.dtype.is_floating_point:
        raise ValueError(f"a must be a floating-point tensor (B, V) with samples and voxels, got {tuple(a.shape)} {a.dtype}")
    if labels.dim() != 1 or labels.shape[0] != a.shape[1] or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must be integers ({a.shape[1]},), got {tuple(labels.shape)} {labels.dtype}")
    _int(R, "R must be an integer >= 1", 1)


def region_stats_torch(a, labels, R):
    """region_stats in stock torch ops on whatever device and dtype `a` has: bincount, index_add_, scatter_reduce("amax") and, for
    argmax, the minimum index among the voxels equal to the bin's max.  The sums of a dtype narrower than float32 are added up
    in float32 and rounded once."""
    _region_args(a, labels, R)
    B, V = a.shape
    lab = labels.to(a.device).long()
    bins = torch.where((lab >= 0) & (lab <= R), lab, torch.zeros_like(lab))
    count = torch.bincount(bins, minlength=R + 1).to(torch.int32)
    wide = a if a.dtype in (_f32, torch.float64) else a.float()
    add = lambda x: torch.zeros((B, R + 1), device=a.device, dtype=wide.dtype).index_add_(1, bins, x).to(a.dtype)
    rows = bins.view(1, V).expand(B, V)
    a0 = wide + 0.0
    mx = torch.full((B, R + 1), float("-inf"), device=a.device, dtype=wide.dtype).scatter_reduce(1, rows, a0, "amax")
    at = torch.arange(V, device=a.device).view(1, V).expand(B, V)
    cand = torch.where(a0 == mx.gather(1, rows), at, torch.full_like(at, V))
    arg = torch.full((B, R + 1), V, device=a.device, dtype=at.dtype).scatter_reduce(1, rows, cand, "amin")
    arg = torch.where(arg < V, arg, torch.full_like(arg, -1)).to(torch.int32)
    return count, add(wide), add(wide.abs()), add(wide.clamp(min=0)), mx.to(a.dtype), arg


def region_stats(a, labels, R):
    """a (B, V), labels (V,) integers, R >= 1 -> (count (R+1,) int32, sum, abs_sum, pos_sum, max (B, R+1) of a's dtype, argmax
    (B, R+1) int32): bin r in 1..R holds the voxels with label r, bin 0 every other voxel; an empty bin has max -inf and argmax -1.
    Contiguous float32 HIP `a`, int32 labels and R <= REGION_MAX: tmf_region_stats (integer sums: the same bits on every call,
    no host read); anything else: region_stats_torch."""
    _region_args(a, labels, R)
    if not (R <= REGION_MAX and _kernel_takes((a, _f32), (labels, torch.int32))):
        return region_stats_torch(a, labels, R)
    _chk(a, "a")
    B, V = a.shape
    count = torch.empty((R + 1,), device=a.device, dtype=torch.int32)
    outs = [torch.empty((B, R + 1), device=a.device, dtype=_f32) for _ in range(4)]
    arg = torch.empty((B, R + 1), device=a.device, dtype=torch.int32)
    nws = _lib.query("tmf_region_workspace_bytes", B, V, R)
    ws = torch.empty((nws,), device=a.device, dtype=torch.uint8)               # the entry zeroes it
    _lib.call("tmf_region_stats", a.data_ptr(), labels.data_ptr(), count.data_ptr(), *(t.data_ptr() for t in outs), arg.data_ptr(),
              ws.data_ptr(), nws, B, V, R, _stream())
    return (count, *outs, arg)


def region_group_update(state, values, cls):
    """state (C, R+1, 3) float64 = (n, sum x, sum x^2) per class and region += the samples of values by class cls (B,), in
    ascending b; a class outside 0..C-1 is skipped.  values (B, R+1), or (B, R) for the regions 1..R alone (column 0 of the state
    is then not touched).  In place.  float32 values, int64 classes and a float64 state, contiguous on one HIP device,
    C <= REGION_MAX_CLASSES, R <= REGION_MAX: ONE launch (tmf_region_group_update), no atomics; anything else: the same sums
    by index_add_ in float64."""
    if state.dim() != 3 or state.shape[2] != 3 or state.dtype != torch.float64 or state.shape[1] < 2:
        raise ValueError(f"state must be float64 (C, R+1, 3), got {tuple(state.shape)} {state.dtype}")
    C, R = state.shape[0], state.shape[1] - 1
    if values.dim() != 2 or values.shape[1] not in (R, R + 1) or values.shape[0] < 1 or tuple(cls.shape) != (values.shape[0],) \
            or cls.dtype.is_floating_point:
        raise ValueError(f"values must be (B, {R + 1}) or (B, {R}) and cls integers (B,), got {tuple(values.shape)} and "
                         f"{tuple(cls.shape)} {cls.dtype}")
    B, first = values.shape[0], R + 1 - values.shape[1]
    if C <= REGION_MAX_CLASSES and R <= REGION_MAX and B <= 65536 \
            and _kernel_takes((state, torch.float64), (values, _f32), (cls, torch.int64)):
        _chk(values, "values")
        _lib.call("tmf_region_group_update", values.data_ptr(), cls.data_ptr(), state.data_ptr(), B, R, C, first, _stream())
        return state
    x = values.detach().to(device=state.device, dtype=torch.float64)
    c = cls.to(state.device).long()
    keep = (c >= 0) & (c < C)
    x, c = x[keep], c[keep]
    state[:, first:].index_add_(0, c, torch.stack([torch.ones_like(x), x, x * x], 2))
    return state


# --------------------------------------------------------------------------------------
# connected clusters and the cluster table (csrc/clusters.hip; include/tmf_hip.h states the foreground, the neighbourhoods, the
# numbering and the outputs)
# --------------------------------------------------------------------------------------

CLUSTER_MODES = {"pos": _lib.CLUSTER_POS, "neg": _lib.CLUSTER_NEG, "abs": _lib.CLUSTER_ABS}
CLUSTER_CONNECTIVITIES = (6, 18, 26)


def cluster_ok(*tensors):
    """The kernels of csrc/clusters.hip take these: contiguous float32 (int32 labels) tensors on one HIP device, none empty."""
    return _kernel_takes(*((t, (_f32, torch.int32)) for t in tensors))


def _cluster_score(a, mode):
    return a if mode == "pos" else -a if mode == "neg" else a.abs()


def _cluster_label_args(a, thr, mode, connectivity, min_size):
    if a.dim() != 4 or a.numel() == 0 or not a.dtype.is_floating_point:
        raise ValueError(f"a must be a floating-point tensor (B, D, H, W) with voxels, got {tuple(a.shape)} {a.dtype}")
    if tuple(thr.shape) != (a.shape[0],) or not thr.dtype.is_floating_point:
        raise ValueError(f"thr must be a floating-point tensor ({a.shape[0]},), got {tuple(thr.shape)} {thr.dtype}")
    if mode not in CLUSTER_MODES:
        raise ValueError(f"mode must be one of {tuple(CLUSTER_MODES)}, got {mode!r}")
    if connectivity not in CLUSTER_CONNECTIVITIES:
        raise ValueError(f"connectivity must be one of {CLUSTER_CONNECTIVITIES}, got {connectivity!r}")
    _int(min_size, "min_size must be an integer >= 1", 1)


def _shifted(x, dim, step, fill):
    """x moved by `step` (+1 / -1) along dim, `fill` where nothing moves in."""
    n = x.shape[dim]
    out = torch.full_like(x, fill)
    if n > 1:
        out.narrow(dim, max(step, 0), n - 1).copy_(x.narrow(dim, max(-step, 0), n - 1))
    return out


def _min3(x, dim, fill):
    return torch.minimum(x, torch.minimum(_shifted(x, dim, 1, fill), _shifted(x, dim, -1, fill)))


def cluster_label_torch(a, thr, mode="pos", connectivity=26, min_size=1):
    """cluster_label in stock torch ops on whatever device and dtype `a` has: every foreground voxel starts with its own linear
    index, takes the minimum over its neighbourhood (shifted copies: the 3 x 3 x 3 cube for 26, the cube without its corners for
    18, the faces for 6) and jumps to its pointer's pointer, until nothing changes (one host read per round); a root is a voxel
    that kept its own index, sizes are a scatter_add at the roots, the numbers a cumsum over the surviving roots."""
    _cluster_label_args(a, thr, mode, connectivity, min_size)
    B, D, H, W = a.shape
    V = D * H * W
    fg = _cluster_score(a, mode) >= thr.to(device=a.device, dtype=a.dtype).view(B, 1, 1, 1)
    idx = torch.arange(V, device=a.device).view(1, D, H, W).expand(B, D, H, W)
    big = torch.full_like(idx, V)
    lab = torch.where(fg, idx, big)
    flat_fg = fg.reshape(B, V)
    while True:
        row = _min3(lab, 3, V)                                          # dw in -1..1
        plus = torch.minimum(row, torch.minimum(_shifted(lab, 2, 1, V), _shifted(lab, 2, -1, V)))     # |dh| + |dw| <= 1
        if connectivity == 26:
            new = _min3(_min3(row, 2, V), 1, V)
        elif connectivity == 18:
            new = torch.minimum(_min3(row, 2, V), torch.minimum(_shifted(plus, 1, 1, V), _shifted(plus, 1, -1, V)))
        else:
            new = torch.minimum(plus, torch.minimum(_shifted(lab, 1, 1, V), _shifted(lab, 1, -1, V)))
        new = torch.where(fg, new, big).reshape(B, V)
        for _ in range(4):                                              # a voxel's pointer lies in its own cluster
            new = torch.where(flat_fg, new.gather(1, torch.where(flat_fg, new, torch.zeros_like(new))), new)
        new = new.view(B, D, H, W)
        if torch.equal(new, lab):
            break
        lab = new
    lab = lab.reshape(B, V)
    at = torch.where(flat_fg, lab, torch.zeros_like(lab))
    size = torch.zeros((B, V), device=a.device, dtype=torch.int64).scatter_add_(1, at, flat_fg.long())
    keep = flat_fg & (lab == idx.reshape(B, V)) & (size >= min_size)
    number = torch.where(keep, keep.long().cumsum(1), torch.zeros_like(lab))
    labels = torch.where(flat_fg, number.gather(1, at), torch.zeros_like(lab))
    return labels.to(torch.int32).view(B, D, H, W), keep.sum(1).to(torch.int32)


def cluster_label(a, thr, mode="pos", connectivity=26, min_size=1):
    """a (B, D, H, W), thr (B,) on a's device -> (labels (B, D, H, W) int32, n (B,) int32): the connected clusters of the voxels
    with s(a) >= thr[b] (s = a, -a, |a| for mode "pos", "neg", "abs"; NaN is never foreground), neighbours by `connectivity` (6,
    18, 26), the clusters of at least min_size voxels numbered 1, 2, ... per sample in ascending order of their lowest linear
    index, everything else 0; n = their number (-1: the kernels hit an internal bound, which a correct build never does).
    Contiguous float32 HIP tensors: tmf_cluster_label (eight stream operations whatever the data, no host read); anything else:
    cluster_label_torch."""
    _cluster_label_args(a, thr, mode, connectivity, min_size)
    if not (_kernel_takes((a, _f32), (thr, _f32)) and a.shape[0] <= 65536):
        return cluster_label_torch(a, thr, mode, connectivity, min_size)
    _chk(a, "a")
    B, D, H, W = a.shape
    labels = torch.empty((B, D, H, W), device=a.device, dtype=torch.int32)
    n = torch.empty((B,), device=a.device, dtype=torch.int32)
    nws = _lib.query("tmf_cluster_workspace_bytes", B, D, H, W)
    ws = torch.empty((nws,), device=a.device, dtype=torch.uint8)               # the entry zeroes what needs it
    _lib.call("tmf_cluster_label", a.data_ptr(), thr.data_ptr(), labels.data_ptr(), n.data_ptr(), ws.data_ptr(), nws, B, D, H, W,
              CLUSTER_MODES[mode], connectivity, min_size, _stream())
    return labels, n


def _cluster_table_args(a, labels, mode, K):
    if a.dim() != 4 or a.numel() == 0 or not a.dtype.is_floating_point:
        raise ValueError(f"a must be a floating-point tensor (B, D, H, W) with voxels, got {tuple(a.shape)} {a.dtype}")
    if tuple(labels.shape) != tuple(a.shape) or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError(f"labels must be integers {tuple(a.shape)}, got {tuple(labels.shape)} {labels.dtype}")
    if mode not in CLUSTER_MODES:
        raise ValueError(f"mode must be one of {tuple(CLUSTER_MODES)}, got {mode!r}")
    _int(K, f"K must be an integer in 1..{a[0].numel()} (the voxels of a sample)", 1, a[0].numel())


def cluster_table_torch(a, labels, mode="pos", K=1):
    """cluster_table in stock torch ops on whatever device and dtype `a` has: scatter_add for the sizes and the coordinate sums,
    scatter_reduce("amax" / "amin") for the largest s(a), the lowest index that attains it and the bounding box."""
    _cluster_table_args(a, labels, mode, K)
    B, D, H, W = a.shape
    V = D * H * W
    dev = a.device
    lab = labels.to(dev).reshape(B, V).long()
    valid = (lab >= 1) & (lab <= K)
    rows = torch.where(valid, lab - 1, torch.full_like(lab, K))                  # column K collects what is ignored
    flat = a.reshape(B, V)
    wide = flat if flat.dtype in (_f32, torch.float64) else flat.float()
    s = _cluster_score(wide, mode) + 0.0
    idx = torch.arange(V, device=dev).view(1, V).expand(B, V)
    size = torch.zeros((B, K + 1), device=dev, dtype=torch.int64).scatter_add_(1, rows, torch.ones_like(lab))
    mx = torch.full((B, K + 1), float("-inf"), device=dev, dtype=wide.dtype).scatter_reduce(1, rows, s, "amax")
    cand = torch.where(s == mx.gather(1, rows), idx, torch.full_like(idx, V))
    arg = torch.full((B, K + 1), V, device=dev, dtype=idx.dtype).scatter_reduce(1, rows, cand, "amin")[:, :K]
    found = arg < V
    peak = torch.where(found, flat.gather(1, arg.clamp(max=V - 1)), torch.full_like(flat[:, :1], float("nan")).expand(B, K))
    coords = torch.stack([idx // (H * W), idx // W % H, idx % W], 2)             # (B, V, 3)
    rows3 = rows.view(B, V, 1).expand(B, V, 3)
    coord_sum = torch.zeros((B, K + 1, 3), device=dev, dtype=torch.int64).scatter_add_(1, rows3, coords)[:, :K]
    start = torch.tensor([D, H, W], device=dev).view(1, 1, 3).expand(B, K + 1, 3).contiguous()
    lo = start.scatter_reduce(1, rows3, coords, "amin")[:, :K]
    hi = torch.full((B, K + 1, 3), -1, device=dev, dtype=torch.int64).scatter_reduce(1, rows3, coords, "amax")[:, :K]
    return (size[:, :K].to(torch.int32), peak.contiguous(), torch.where(found, arg, torch.full_like(arg, -1)).to(torch.int32),
            coord_sum.contiguous(), torch.cat([lo, hi], 2).to(torch.int32))


def cluster_table(a, labels, mode="pos", K=1):
    """a (B, D, H, W), labels (B, D, H, W) integers, K >= 1 -> (size (B, K) int32, peak (B, K) of a's dtype, argmax (B, K) int32,
    coord_sum (B, K, 3) int64, bbox (B, K, 6) int32): row k-1 describes the voxels with label k (a label outside 1..K is
    ignored) - their number, the value of the voxel whose s(a) is largest (NaN for an empty row), the lowest linear index of such
    a voxel (-1), the sums of d, h, w and (min d, min h, min w, max d, max h, max w) ((D, H, W, -1, -1, -1)).  Contiguous float32
    HIP `a` and int32 labels: tmf_cluster_table (three launches, integer atomics: the same bits on every call); anything else:
    cluster_table_torch."""
    _cluster_table_args(a, labels, mode, K)
    B = a.shape[0]
    if not (_kernel_takes((a, _f32), (labels, torch.int32)) and B <= 65536 and B * K < 1 << 31):
        return cluster_table_torch(a, labels, mode, K)
    _chk(a, "a")
    size, arg = (torch.empty((B, K), device=a.device, dtype=torch.int32) for _ in range(2))
    peak = torch.empty((B, K), device=a.device, dtype=_f32)
    coord_sum = torch.empty((B, K, 3), device=a.device, dtype=torch.int64)
    bbox = torch.empty((B, K, 6), device=a.device, dtype=torch.int32)
    _lib.call("tmf_cluster_table", a.data_ptr(), labels.data_ptr(), size.data_ptr(), peak.data_ptr(), arg.data_ptr(),
              coord_sum.data_ptr(), bbox.data_ptr(), B, *a.shape[1:], CLUSTER_MODES[mode], K, _stream())
    return size, peak, arg, coord_sum, bbox


# --------------------------------------------------------------------------------------
# Gaussian smoothing (csrc/smooth.hip; include/tmf_hip.h states the taps, the border modes, the mask and the error bound)
# --------------------------------------------------------------------------------------

SMOOTH_MODES = {"reflect": _lib.SMOOTH_REFLECT, "constant": _lib.SMOOTH_CONSTANT, "nearest": _lib.SMOOTH_NEAREST}
SMOOTH_MAX_RADIUS = _lib.SMOOTH_MAX_RADIUS


_smooth_scratch = (ctypes.c_float * (2 * SMOOTH_MAX_RADIUS + 1))()


def smooth_radius(sigma, truncate=4.0):
    """The radius r = (int)(truncate*sigma + 0.5) as tmf_gaussian_taps has it; ValueError, with the library's message, for what it
    refuses (a negative or non-finite sigma, a bad truncate, a radius above SMOOTH_MAX_RADIUS)."""
    try:
        r = _lib.query("tmf_gaussian_taps", float(sigma), float(truncate), ctypes.addressof(_smooth_scratch), len(_smooth_scratch))
    except (TypeError, ValueError):
        raise ValueError(f"sigma and truncate must be numbers, got {sigma!r} and {truncate!r}") from None
    if r < 0:
        raise ValueError(_lib.query("tmf_last_error_string").decode())
    return r


def gaussian_taps(sigma, truncate=4.0, dtype=_f32):
    """The 2r+1 taps of one axis as the library defines them -> a CPU tensor: float32 from tmf_gaussian_taps (what the kernels
    use), float64 from tmf_gaussian_taps_f64 (the taps before their one rounding).  sigma 0: the one tap 1.  ValueError, with
    the library's message, for what the entry refuses (a negative or non-finite sigma, a bad truncate, a radius above
    SMOOTH_MAX_RADIUS)."""
    if dtype not in (_f32, torch.float64):
        raise ValueError(f"taps are float32 or float64, got {dtype}")
    try:
        sigma, truncate = float(sigma), float(truncate)
    except (TypeError, ValueError):
        raise ValueError(f"sigma and truncate must be numbers, got {sigma!r} and {truncate!r}") from None
    n = 2 * SMOOTH_MAX_RADIUS + 1
    buf = ((ctypes.c_float if dtype == _f32 else ctypes.c_double) * n)()
    r = _lib.query("tmf_gaussian_taps" if dtype == _f32 else "tmf_gaussian_taps_f64", sigma, truncate, ctypes.addressof(buf), n)
    if r < 0:
        raise ValueError(_lib.query("tmf_last_error_string").decode())
    return torch.tensor(buf[:2 * r + 1], dtype=dtype)


def _smooth_args(a, sigma3, truncate, mode, mask):
    if a.dim() != 4 or a.numel() == 0 or not a.dtype.is_floating_point:
        raise ValueError(f"a must be a floating-point tensor (B, D, H, W) with voxels, got {tuple(a.shape)} {a.dtype}")
    if mode not in SMOOTH_MODES:
        raise ValueError(f"mode must be one of {tuple(SMOOTH_MODES)}, got {mode!r}")
    if len(sigma3) != 3:
        raise ValueError(f"sigma3 must hold the three sigmas (d, h, w), got {sigma3!r}")
    if mask is not None and (tuple(mask.shape) != tuple(a.shape[1:]) or mask.dtype.is_floating_point):
        raise ValueError(f"mask must be bool or integers {tuple(a.shape[1:])}, got {tuple(mask.shape)} {mask.dtype}")


def smooth_source_index(n, r, mode, device=None):
    """(n, 2r+1) int64: the source index of output o and tap i = -r..r on an axis of extent n under `mode`, -1 where the tap
    contributes 0 ("constant" outside 0..n-1) - the index formulas of include/tmf_hip.h."""
    j = torch.arange(n, device=device).view(n, 1) + torch.arange(-r, r + 1, device=device).view(1, 2 * r + 1)
    if mode == "reflect":
        p = j % (2 * n)                                                     # non-negative for a positive modulus
        return torch.where(p < n, p, 2 * n - 1 - p)
    if mode == "nearest":
        return j.clamp(0, n - 1)
    return torch.where((j >= 0) & (j < n), j, torch.full_like(j, -1))


def _smooth_axis(x, dim, taps, mode):
    """One 1-D pass along dim: the taps in ascending order, one index_select, one multiply and one add each."""
    r = (taps.numel() - 1) // 2
    src = smooth_source_index(x.shape[dim], r, mode, x.device)
    shape = [1] * x.dim()
    shape[dim] = x.shape[dim]
    acc = torch.zeros_like(x)
    for i, w in enumerate(taps.tolist()):
        col = src[:, i]
        term = x.index_select(dim, col.clamp(min=0))
        if mode == "constant":
            term = torch.where((col >= 0).view(shape), term, torch.zeros_like(term))
        acc = acc + w * term
    return acc


def gaussian_smooth_torch(a, sigma3, truncate=4.0, mode="reflect", mask=None):
    """gaussian_smooth in stock torch ops on whatever device and floating dtype `a` has: per filtered axis one index_select per
    tap through the index formulas of include/tmf_hip.h, accumulated in ascending tap order; with a mask G(a*m) / G(m) inside
    and 0 outside.  The taps are the library's (gaussian_taps): the float32 ones for float32 and narrower tensors, which are
    filtered in float32 and rounded once, the unrounded float64 ones for float64 tensors."""
    _smooth_args(a, sigma3, truncate, mode, mask)
    wide = a.dtype if a.dtype in (_f32, torch.float64) else _f32
    taps = [gaussian_taps(s, truncate, wide) for s in sigma3]
    x = a.to(wide)
    inside = None
    if mask is not None:
        inside = (mask.to(a.device) != 0).view(1, *a.shape[1:])
        x = torch.where(inside, x, torch.zeros_like(x))
        den = inside.to(wide)
    for dim in (3, 2, 1):                                                       # W, H, D: the order of the kernels
        t = taps[dim - 1]
        if t.numel() == 1:
            continue
        x = _smooth_axis(x, dim, t, mode)
        if inside is not None:
            den = _smooth_axis(den, dim, t, mode)
    if inside is not None:
        x = torch.where(inside, x / torch.where(inside, den, torch.ones_like(den)), torch.zeros_like(x))
    return x.to(a.dtype)


def smooth_ok(a, mask=None):
    """tmf_gaussian_smooth takes these: a contiguous float32 (B, D, H, W) on a HIP device with B <= 65536 and D*H*W < 2^31, the
    mask (if any) contiguous int32 on the same device."""
    pairs = [(a, _f32)] + ([(mask, torch.int32)] if mask is not None else [])
    return _kernel_takes(*pairs) and a.dim() == 4 and a.shape[0] <= 65536 and a[0].numel() < 1 << 31


def gaussian_smooth(a, sigma3, truncate=4.0, mode="reflect", mask=None, out=None):
    """a (B, D, H, W) float32 on a HIP device, sigma3 = (sigma_d, sigma_h, sigma_w) in voxels, mask None or (D, H, W) int32 ->
    the Gaussian-filtered maps (tmf_gaussian_smooth: two launches, no host read, the same bits on every call); with a mask
    G(a*m) / G(m) inside it and 0 outside.  The kernel path only: TmfError for tensors it does not take (see smooth_ok;
    gaussian_smooth_torch is the same function in stock ops), ValueError for arguments the entry refuses."""
    _smooth_args(a, sigma3, truncate, mode, mask)
    if not smooth_ok(a, mask):
        raise _lib.TmfError("gaussian_smooth takes a contiguous float32 (B, D, H, W) tensor (and an int32 mask) on one HIP device")
    for s in sigma3:
        smooth_radius(s, truncate)                          # the library's own refusal, as a ValueError, before anything is allocated
    _chk(a, "a")
    B, D, H, W = a.shape
    if out is None:
        out = torch.empty_like(a)
    elif out.shape != a.shape or not _kernel_takes((a, _f32), (out, _f32)):
        raise ValueError(f"out must be a contiguous float32 tensor {tuple(a.shape)} on a's device")
    nws = _lib.query("tmf_smooth_workspace_bytes", B, D, H, W, int(mask is not None))
    ws = torch.empty((nws,), device=a.device, dtype=torch.uint8)
    _lib.call("tmf_gaussian_smooth", a.data_ptr(), _ptr(mask), out.data_ptr(), *(float(s) for s in sigma3), float(truncate),
              SMOOTH_MODES[mode], ws.data_ptr(), nws, B, D, H, W, _stream())
    return out


class FusionTrain(torch.autograd.Function):
    """CrossTransformer_MOD_AVG forward / backward as ONE library call each (tmf_fusion_train_fwd / _bwd,
    csrc/fusion_path.hip).  forward(mri_tok, pet_tok, cfg, *params): params = per Transformer instance (mri enc of layer
    0, pet enc of layer 0, mri enc of layer 1, ...) the 14 tensors of _lib.XFORMER_PTRS order -> cls (B, 4*dim)."""

    @staticmethod
    def forward(ctx, mri, pet, cfg, *params):
        import ctypes as C
        mri, pet, desc, inst, masks = _fusion_call_setup(mri, pet, cfg, params)
        B, _N, dim = mri.shape
        nsaved = _lib.query("tmf_fusion_saved_bytes", C.byref(desc))
        if nsaved == 0:
            raise _lib.TmfError("tmf_fusion_saved_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
        saved = torch.empty(nsaved, device=mri.device, dtype=torch.uint8)
        cls = torch.empty((B, 4 * dim), device=mri.device, dtype=_f32)
        _lib.call("tmf_fusion_train_fwd", C.byref(desc), mri.data_ptr(), pet.data_ptr(), inst, saved.data_ptr(), nsaved,
                  cls.data_ptr(), _stream())
        ctx.save_for_backward(mri, pet, saved, *params)     # parameters too: autograd then rejects an in-place update
        ctx.desc, ctx.inst = desc, inst                     # between forward and backward; their pointers stay valid:
        ctx.masks = masks                                   # the ctypes structs are reused as they are
        ctx.param_ptrs = [t.data_ptr() for t in params]
        # Everything backward needs besides the incoming gradient is set up NOW, while the GPU is busy with the forward:
        # backward starts right behind the reference step's two loss.item() host syncs (kfold_train_adversarial.py:127-128),
        # where every microsecond of host preparation is a microsecond of idle GPU (measured: 140 us of gap in front of the
        # first fusion-backward kernel).
        ctx.bwd = FusionTrain._prepare_backward(desc, mri, pet) if any(ctx.needs_input_grad) else None
        return cls

    @staticmethod
    def _prepare_backward(desc, mri, pet):
        import ctypes as C
        depth, dim, mlp = desc.depth, desc.dim, desc.mlp
        inner = desc.heads * desc.dim_head
        n_inst = 2 * depth
        grads = (_lib.XformerGrads * n_inst)()
        # ONE flat gradient buffer for the whole fusion, cut by ONE split call; per instance
        # [b2 | b1 | bo | ln2 g | ln2 b | ln1 g | ln1 b | lnf g | lnf b | dwq | dwkv | dwo | dw1 | dw2]
        # (the first seven are the contiguous `small` region of tmf_xformer_grads, the next two its `lnf`)
        sizes = [dim, mlp, dim, dim, dim, dim, dim, dim, dim, inner * dim, 2 * inner * dim, dim * inner, mlp * dim, dim * mlp]
        per = sum(sizes)
        flat = torch.empty(n_inst * per, device=mri.device, dtype=_f32)
        parts = flat.split(sizes * n_inst)
        base = flat.data_ptr()
        o_lnf = 4 * (6 * dim + mlp)
        o_w = [o_lnf + 4 * 2 * dim]
        for n in sizes[9:13]:
            o_w.append(o_w[-1] + 4 * n)
        out = [None, None, None]
        for i in range(n_inst):
            g = grads[i]
            b0 = base + 4 * i * per
            g.small, g.lnf = b0, b0 + o_lnf
            g.dwq, g.dwkv, g.dwo, g.dw1, g.dw2 = (b0 + o for o in o_w)
            b2, b1, bo, g2, be2, g1, be1, gf, bf, dwq, dwkv, dwo, dw1, dw2 = parts[14 * i:14 * i + 14]
            # order of _lib.XFORMER_PTRS
            out += [g1, be1, dwq.view(inner, dim), dwkv.view(2 * inner, dim), dwo.view(dim, inner), bo, g2, be2,
                    dw1.view(mlp, dim), b1, dw2.view(dim, mlp), b2, gf, bf]
        dm = torch.empty_like(mri)
        dp = torch.empty_like(pet)
        nscr = _lib.query("tmf_fusion_bwd_scratch_bytes", C.byref(desc))
        scratch = torch.empty(nscr, device=mri.device, dtype=torch.uint8)
        out[0], out[1] = dm, dp
        return grads, flat, out, dm, dp, scratch, nscr

    @staticmethod
    def backward(ctx, dcls):
        import ctypes as C
        mri, pet, saved = ctx.saved_tensors[:3]
        desc, inst = ctx.desc, ctx.inst
        dcls = _chk(dcls, "grad_output")
        prep = ctx.bwd if ctx.bwd is not None else FusionTrain._prepare_backward(desc, mri, pet)
        ctx.bwd = None
        grads, flat, out, dm, dp, scratch, nscr = prep
        _lib.call("tmf_fusion_train_bwd", C.byref(desc), mri.data_ptr(), pet.data_ptr(), inst, saved.data_ptr(),
                  saved.numel(), dcls.data_ptr(), grads, dm.data_ptr(), dp.data_ptr(), scratch.data_ptr(), nscr, _stream())
        # (Round 4 measured the parameter-gradient launches of this pass — column sums, the weight-gradient launch: 0.08 ms
        #  of latency-bound work nothing in backward waits for — on a side stream beside the encoders' backward: per-step
        #  medians 14.54 / 14.60 / 14.60 ms against 14.64 / 14.56 / 14.55, and 7.41 / 7.44 / 7.41 against 7.42 / 7.44 / 7.39 at
        #  128^3 bf16: level — what leaves the serial token phase is paid back as CU time beside the encoders' kernels.  Dropped.
        #  A first, flawed version was 2-4 % SLOWER: its end-of-backward callback kept the gradient VIEWS alive, and autograd
        #  adopts a view as .grad only while it holds the last reference — a kept view is cloned: 84 copy launches.)
        if _FLAT_GRAD_CONSUMERS and all(ctx.needs_input_grad[3:]):
            _publish_flat_grads(flat, ctx.param_ptrs, out[3:], [(0, flat.numel(), None, "next")])
        return tuple(out)


# --------------------------------------------------------------------------------------
# the dense heads of model_ad in one launch per direction            (mymodel.py:190-194, 209-221)
# --------------------------------------------------------------------------------------

HEADS_ONE_CALL = os.environ.get("TMF_HEADS_C", "1") != "0"


class HeadsAD(torch.autograd.Function):
    """fc_cls(cls) and D(revgrad(mean_n mri_tok)), D(revgrad(mean_n pet_tok)) as ONE kernel forward and ONE backward
    (tmf_heads_fwd / _bwd, csrc/heads.hip).  forward(cls, mri_tok, pet_tok, mask1, mask2, cfg, buffers, *params) with
    params in _lib.HEADS_PARAMS order, buffers in _lib.HEADS_BUFFERS order (None = no running statistics), masks = scaled
    Dropout keep-masks or None, cfg = (training, (momentum x3), (eps x3), revgrad alpha) -> (logits, D_MRI, D_PET)."""

    @staticmethod
    def forward(ctx, cls, mri, pet, mask1, mask2, cfg, buffers, *params):
        import ctypes as C
        cls, mri, pet = _chk(cls, "cls"), _chk(mri, "mri_tokens"), _chk(pet, "pet_tokens")
        training, momentum, eps, alpha = cfg
        B, N, dim = mri.shape
        P = dict(zip(_lib.HEADS_PARAMS, params))
        desc = _lib.HeadsDesc(B=B, N=N, dim=dim, H1=P["fc0_w"].shape[0], H2=P["fc4_w"].shape[0], HD=P["d0_w"].shape[0],
                              NC=P["fc8_w"].shape[0], training=int(training))
        for i in range(3):
            desc.momentum[i], desc.eps[i] = momentum[i], eps[i]
        prm = _lib.HeadsParams()
        for name, t in P.items():
            if not (t.is_cuda and t.dtype == _f32 and t.is_contiguous()):
                raise _lib.TmfError(f"heads: {name} must be a contiguous float32 tensor on the HIP device")
            setattr(prm, name, t.data_ptr())
        for name, t in zip(_lib.HEADS_BUFFERS, buffers):
            setattr(prm, name, _ptr(t))
        m1 = None if mask1 is None else _chk(mask1, "mask1")
        m2 = None if mask2 is None else _chk(mask2, "mask2")
        nsaved = _lib.query("tmf_heads_saved_bytes", C.byref(desc))
        if nsaved == 0:
            raise _lib.TmfError("tmf_heads_saved_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
        saved = torch.empty(nsaved // 4, device=cls.device, dtype=_f32)
        outs = torch.empty((3, B, desc.NC), device=cls.device, dtype=_f32)
        _lib.call("tmf_heads_fwd", C.byref(desc), cls.data_ptr(), mri.data_ptr(), pet.data_ptr(), _ptr(m1), _ptr(m2),
                  C.byref(prm), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), saved.data_ptr(), nsaved, _stream())
        ctx.save_for_backward(cls, saved, *params)
        ctx.masks = (m1, m2)
        ctx.desc, ctx.prm, ctx.alpha = desc, prm, float(alpha)
        ctx.tok_shape = tuple(mri.shape)
        ctx.param_ptrs = [t.data_ptr() for t in params]
        # backward's buffers and gradient table, set up while the GPU is still busy with the forward (see FusionTrain)
        ctx.bwd = HeadsAD._prepare_backward(desc, cls, params, ctx.tok_shape) if any(ctx.needs_input_grad) else None
        return outs[0], outs[1], outs[2]

    @staticmethod
    def _prepare_backward(desc, cls, params, tok_shape):
        import ctypes as C
        dev = cls.device
        sizes = [p.numel() for p in params]
        flat = torch.empty(sum(sizes), device=dev, dtype=_f32)
        parts = flat.split(sizes)
        g = _lib.HeadsGrads()
        o = flat.data_ptr()
        for name, n in zip(_lib.HEADS_PARAMS, sizes):
            setattr(g, name, o)
            o += 4 * n
        d_cls = torch.empty_like(cls)
        d_tok = torch.empty((2,) + tok_shape, device=dev, dtype=_f32)
        nscr = _lib.query("tmf_heads_bwd_scratch_bytes", C.byref(desc))
        scratch = torch.empty(nscr // 4, device=dev, dtype=_f32)
        zero = torch.zeros((desc.B, desc.NC), device=dev, dtype=_f32)      # stands in for an output nobody differentiated
        grads = [t if p.dim() == 1 else t.view(p.shape) for t, p in zip(parts, params)]
        return g, flat, grads, d_cls, d_tok, scratch, nscr, zero

    @staticmethod
    def backward(ctx, dlo, ddm, ddp):
        import ctypes as C
        cls, saved = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        desc = ctx.desc
        prep = ctx.bwd if ctx.bwd is not None else HeadsAD._prepare_backward(desc, cls, params, ctx.tok_shape)
        ctx.bwd = None
        g, flat, grads, d_cls, d_tok, scratch, nscr, zero = prep
        # the three output gradients go to the library as they are (no stack / copy launch in front of the kernel)
        dl = [zero if t is None else (t if (t.dtype == _f32 and t.is_contiguous()) else t.to(_f32).contiguous())
              for t in (dlo, ddm, ddp)]
        m1, m2 = ctx.masks
        _lib.call("tmf_heads_bwd", C.byref(desc), cls.data_ptr(), _ptr(m1), _ptr(m2), C.byref(ctx.prm), saved.data_ptr(),
                  saved.numel() * 4, dl[0].data_ptr(), dl[1].data_ptr(), dl[2].data_ptr(), C.byref(g), d_cls.data_ptr(),
                  d_tok[0].data_ptr(), d_tok[1].data_ptr(), ctx.alpha, scratch.data_ptr(), nscr, _stream())
        if _FLAT_GRAD_CONSUMERS and all(ctx.needs_input_grad[7:]):
            _publish_flat_grads(flat, ctx.param_ptrs, grads, [(0, flat.numel(), None, "next")])
        return (d_cls, d_tok[0], d_tok[1], None, None, None, None, *grads)


class HeadsCNN(torch.autograd.Function):
    """The heads of the CNN-only models as ONE kernel per direction (tmf_heads_cnn_fwd / _bwd, csrc/heads.hip):
    model_CNN_ad: fc_cls(cat[mean_n mri, mean_n pet]), D(revgrad(mean_n mri)), D(revgrad(mean_n pet))   (mymodel.py:164-178)
    model_single: fc(mean_n tok)                                                                          (mymodel.py:33-39).
    forward(mri_tok, pet_tok | None, cfg, buffers, *params): params = fc0_w, fc0_b, fc2_w, fc2_b [, d0_w, d0_b, dbn_g, dbn_b,
    d3_w, d3_b]; buffers = (running_mean, running_var) of D's BatchNorm1d or (None, None); cfg = (training, momentum, eps,
    revgrad alpha) -> (logits, D_MRI, D_PET) or (logits,)."""

    @staticmethod
    def forward(ctx, mri, pet, cfg, buffers, *params):
        import ctypes as C
        mri = _chk(mri, "mri_tokens")
        M = 1 if pet is None else 2
        if M == 2:
            pet = _chk(pet, "pet_tokens")
            if pet.shape != mri.shape:
                raise _lib.TmfError(f"token shapes differ: {tuple(mri.shape)} vs {tuple(pet.shape)}")
        with_d = len(params) == len(_lib.HEADS_CNN_PARAMS)
        if not with_d and len(params) != 4:
            raise _lib.TmfError(f"heads_cnn: {len(params)} parameter tensors (4 without, 10 with the discriminator)")
        training, momentum, eps, alpha = cfg
        B, N, dim = mri.shape
        P = dict(zip(_lib.HEADS_CNN_PARAMS, params))
        desc = _lib.HeadsCnnDesc(B=B, N=N, dim=dim, M=M, H=P["fc0_w"].shape[0], HD=P["d0_w"].shape[0] if with_d else 0,
                                 NC=P["fc2_w"].shape[0], training=int(training), momentum=momentum, eps=eps)
        prm = _lib.HeadsCnnParams()
        for name, t in P.items():
            if not (t.is_cuda and t.dtype == _f32 and t.is_contiguous()):
                raise _lib.TmfError(f"heads_cnn: {name} must be a contiguous float32 tensor on the HIP device")
            setattr(prm, name, t.data_ptr())
        prm.dbn_rm, prm.dbn_rv = _ptr(buffers[0]), _ptr(buffers[1])
        nsaved = _lib.query("tmf_heads_cnn_saved_bytes", C.byref(desc))
        if nsaved == 0:
            raise _lib.TmfError("tmf_heads_cnn_saved_bytes: " + (_lib.load().tmf_last_error_string() or b"").decode())
        saved = torch.empty(nsaved // 4, device=mri.device, dtype=_f32)
        outs = torch.empty((3 if with_d else 1, B, desc.NC), device=mri.device, dtype=_f32)
        _lib.call("tmf_heads_cnn_fwd", C.byref(desc), mri.data_ptr(), _ptr(pet), C.byref(prm), outs[0].data_ptr(),
                  outs[1].data_ptr() if with_d else None, outs[2].data_ptr() if with_d else None, saved.data_ptr(), nsaved,
                  _stream())
        ctx.save_for_backward(saved, *params)
        ctx.desc, ctx.prm, ctx.alpha, ctx.with_d = desc, prm, float(alpha), with_d
        ctx.tok_shape = tuple(mri.shape)
        ctx.param_ptrs = [t.data_ptr() for t in params]
        ctx.bwd = HeadsCNN._prepare_backward(desc, mri.device, params, ctx.tok_shape) if any(ctx.needs_input_grad) else None
        return (outs[0], outs[1], outs[2]) if with_d else outs[0]

    @staticmethod
    def _prepare_backward(desc, dev, params, tok_shape):
        import ctypes as C
        sizes = [p.numel() for p in params]
        flat = torch.empty(sum(sizes), device=dev, dtype=_f32)
        parts = flat.split(sizes)
        g = _lib.HeadsCnnGrads()
        o = flat.data_ptr()
        for name, n in zip(_lib.HEADS_CNN_PARAMS, sizes):
            setattr(g, name, o)
            o += 4 * n
        d_tok = torch.empty((desc.M,) + tok_shape, device=dev, dtype=_f32)
        nscr = _lib.query("tmf_heads_cnn_bwd_scratch_bytes", C.byref(desc))
        scratch = torch.empty(nscr // 4, device=dev, dtype=_f32)
        zero = torch.zeros((desc.B, desc.NC), device=dev, dtype=_f32)      # stands in for an output nobody differentiated
        grads = [t if p.dim() == 1 else t.view(p.shape) for t, p in zip(parts, params)]
        return g, flat, grads, d_tok, scratch, nscr, zero

    @staticmethod
    def backward(ctx, dlo, ddm=None, ddp=None):
        import ctypes as C
        saved = ctx.saved_tensors[0]
        params = ctx.saved_tensors[1:]
        desc = ctx.desc
        prep = ctx.bwd if ctx.bwd is not None else HeadsCNN._prepare_backward(desc, saved.device, params, ctx.tok_shape)
        ctx.bwd = None
        g, flat, grads, d_tok, scratch, nscr, zero = prep
        dl = [zero if t is None else (t if (t.dtype == _f32 and t.is_contiguous()) else t.to(_f32).contiguous())
              for t in (dlo, ddm, ddp)]
        two = desc.M == 2
        _lib.call("tmf_heads_cnn_bwd", C.byref(desc), C.byref(ctx.prm), saved.data_ptr(), saved.numel() * 4, dl[0].data_ptr(),
                  dl[1].data_ptr() if ctx.with_d else None, dl[2].data_ptr() if ctx.with_d else None, C.byref(g),
                  d_tok[0].data_ptr(), d_tok[1].data_ptr() if two else None, ctx.alpha, scratch.data_ptr(), nscr, _stream())
        if _FLAT_GRAD_CONSUMERS and all(ctx.needs_input_grad[4:]):
            _publish_flat_grads(flat, ctx.param_ptrs, grads, [(0, flat.numel(), None, "next")])
        return (d_tok[0], d_tok[1] if two else None, None, None, *grads)


# --------------------------------------------------------------------------------------
# token pooling head                                                (networks.py:276-281)
# --------------------------------------------------------------------------------------

class TokenPool(torch.autograd.Function):
    """cat[mean_n mri, mean_n pet, max_n mri, max_n pet] -> (B, 4*dim)."""

    @staticmethod
    def forward(ctx, mri, pet):
        mri, pet = _chk(mri, "mri_tokens"), _chk(pet, "pet_tokens")
        B, N, dim = mri.shape
        if pet.shape != mri.shape:
            raise _lib.TmfError(f"token shapes differ: {tuple(mri.shape)} vs {tuple(pet.shape)}")
        cls = torch.empty((B, 4 * dim), device=mri.device, dtype=_f32)
        arg = torch.empty((B, 2, dim), device=mri.device, dtype=torch.int32)
        _lib.call("tmf_token_pool_fwd", mri.data_ptr(), pet.data_ptr(), cls.data_ptr(), arg.data_ptr(),
                  B, N, dim, _stream())
        ctx.save_for_backward(arg)
        ctx.shape = (B, N, dim)
        return cls

    @staticmethod
    def backward(ctx, dcls):
        (arg,) = ctx.saved_tensors
        B, N, dim = ctx.shape
        dcls = _chk(dcls, "grad_output")
        dm = torch.empty((B, N, dim), device=dcls.device, dtype=_f32)
        dp = torch.empty((B, N, dim), device=dcls.device, dtype=_f32)
        _lib.call("tmf_token_pool_bwd", dcls.data_ptr(), arg.data_ptr(), dm.data_ptr(), dp.data_ptr(),
                  B, N, dim, _stream())
        return dm, dp


def token_pool(mri, pet):
    return TokenPool.apply(mri, pet)


# --------------------------------------------------------------------------------------
# losses                                                          (losses.py:59-100, 122-128)
# --------------------------------------------------------------------------------------

class FALossFn(torch.autograd.Function):
    """sum |F1^T F1 - F2^T F2| (reduction 0: / (B N^2)) over two fp32 maps of one layout: (B, C, N) contiguous
    (channels_last False) or (B, N, C) contiguous (the storage behind sNet's output).  The forward of a call that wants a
    gradient also leaves the unscaled gradients (tmf_faloss_fwd); the backward scales them by grad_output."""

    @staticmethod
    def forward(ctx, f1, f2, B, C, N, channels_last, reduction):
        f1, f2 = _chk(f1, "feature_map1"), _chk(f2, "feature_map2")
        want = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss = torch.empty((), device=f1.device, dtype=_f32)
        ws = torch.empty(_lib.query("tmf_faloss_partial_rows", B, N), device=f1.device, dtype=torch.float64)
        g1 = torch.empty_like(f1) if want else None
        g2 = torch.empty_like(f2) if want else None
        _lib.call("tmf_faloss_fwd", f1.data_ptr(), f2.data_ptr(), loss.data_ptr(), _ptr(g1), _ptr(g2), ws.data_ptr(),
                  ws.numel() * 8, B, C, N, int(channels_last), reduction, _stream())
        if want:
            ctx.save_for_backward(g1, g2)
        ctx.cfg = (B, C, N, reduction)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        g1, g2 = ctx.saved_tensors
        B, C, N, reduction = ctx.cfg
        dloss = _chk(dloss, "grad_output")
        d1, d2 = torch.empty_like(g1), torch.empty_like(g2)
        _lib.call("tmf_faloss_bwd", g1.data_ptr(), g2.data_ptr(), dloss.data_ptr(), d1.data_ptr(), d2.data_ptr(),
                  B, C, N, reduction, _stream())
        return d1, d2, None, None, None, None, None


def faloss(f1, f2, B, C, N, channels_last, reduction):
    return FALossFn.apply(f1, f2, B, C, N, channels_last, reduction)


class SupConLossFn(torch.autograd.Function):
    """SupConLoss over contiguous fp32 features (bs, views, d); labels: int64 (bs,) or None; mask: fp32 (bs, bs) or None."""

    @staticmethod
    def forward(ctx, features, labels, mask, anchors_all, temperature, base_temperature):
        features = _chk(features, "features")
        bs, views, d = features.shape
        want = ctx.needs_input_grad[0]
        loss = torch.empty((), device=features.device, dtype=_f32)
        g = torch.empty_like(features) if want else None
        _lib.call("tmf_supcon_fwd", features.data_ptr(), _ptr(labels), _ptr(mask), loss.data_ptr(), _ptr(g), bs, views, d,
                  int(anchors_all), float(temperature), float(base_temperature), _stream())
        if want:
            ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (g,) = ctx.saved_tensors
        bs, views, d = g.shape
        dloss = _chk(dloss, "grad_output")
        df = torch.empty_like(g)
        _lib.call("tmf_supcon_bwd", g.data_ptr(), dloss.data_ptr(), df.data_ptr(), bs, views, d, _stream())
        return df, None, None, None, None, None


def supcon_loss(features, labels, mask, anchors_all, temperature, base_temperature):
    return SupConLossFn.apply(features, labels, mask, anchors_all, temperature, base_temperature)


# --------------------------------------------------------------------------------------
# criterion and epoch metrics                       (kfold_train_adversarial.py:119-131, 178-194)
# --------------------------------------------------------------------------------------

class CrossEntropyFn(torch.autograd.Function):
    """F.cross_entropy over fp32 (B, C) logits and int64 targets, reduction 0 mean | 1 sum (tmf_ce_fwd): one launch that
    also leaves dloss / dlogits when a gradient is wanted; the backward scales it by grad_output (tmf_ce_bwd)."""

    @staticmethod
    def forward(ctx, logits, target, weight, reduction):
        logits = _chk(logits, "input")
        B, C = logits.shape
        want = ctx.needs_input_grad[0]
        loss = torch.empty((), device=logits.device, dtype=_f32)
        g = torch.empty_like(logits) if want else None
        _lib.call("tmf_ce_fwd", logits.data_ptr(), target.data_ptr(), _ptr(weight), loss.data_ptr(), _ptr(g), B, C, reduction,
                  _stream())
        if want:
            ctx.save_for_backward(g)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        (g,) = ctx.saved_tensors
        dloss = _chk(dloss, "grad_output")
        d = torch.empty_like(g)
        _lib.call("tmf_ce_bwd", g.data_ptr(), dloss.data_ptr(), d.data_ptr(), g.shape[0], g.shape[1], _stream())
        return d, None, None, None


def cross_entropy(logits, target, weight, reduction):
    return CrossEntropyFn.apply(logits, target, weight, reduction)


class AdversarialCriterionFn(torch.autograd.Function):
    """(CE(logits, label), (CE(d_mri, 1) + CE(d_pet, 0)) / 2) as two 0-dim views of one 2-float tensor, in one launch
    (tmf_adv_criterion_fwd); the backward takes the two grads — either may be absent — and makes one launch."""

    @staticmethod
    def forward(ctx, logits, d_mri, d_pet, label, weight):
        logits, d_mri, d_pet = _chk(logits, "output_logits"), _chk(d_mri, "D_MRI_logits"), _chk(d_pet, "D_PET_logits")
        B, C = logits.shape
        want = any(ctx.needs_input_grad[:3])
        losses = torch.empty(2, device=logits.device, dtype=_f32)
        gs = (torch.empty_like(logits), torch.empty_like(d_mri), torch.empty_like(d_pet)) if want else (None, None, None)
        _lib.call("tmf_adv_criterion_fwd", logits.data_ptr(), d_mri.data_ptr(), d_pet.data_ptr(), label.data_ptr(), _ptr(weight),
                  losses.data_ptr(), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), B, C, _stream())
        if want:
            ctx.save_for_backward(*gs)
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, d_ce, d_ad):
        g0, g1, g2 = ctx.saved_tensors
        d_ce = None if d_ce is None else _chk(d_ce, "grad of ce_loss")
        d_ad = None if d_ad is None else _chk(d_ad, "grad of ad_loss")
        d0, d1, d2 = torch.empty_like(g0), torch.empty_like(g1), torch.empty_like(g2)
        _lib.call("tmf_adv_criterion_bwd", g0.data_ptr(), g1.data_ptr(), g2.data_ptr(), _ptr(d_ce), _ptr(d_ad), d0.data_ptr(),
                  d1.data_ptr(), d2.data_ptr(), g0.shape[0], g0.shape[1], _stream())
        return d0, d1, d2, None, None


def adversarial_criterion(logits, d_mri, d_pet, label, weight):
    return AdversarialCriterionFn.apply(logits, d_mri, d_pet, label, weight)


def train_metrics_update(state, losses, logits, d_mri, d_pet, label):
    """One read-add-write of the (8,) int64 device state (tmf_train_metrics_update); losses: the 2-float device tensor."""
    logits, d_mri, d_pet = _chk(logits, "output_logits"), _chk(d_mri, "D_MRI_logits"), _chk(d_pet, "D_PET_logits")
    _lib.call("tmf_train_metrics_update", state.data_ptr(), losses.data_ptr(), logits.data_ptr(), d_mri.data_ptr(),
              d_pet.data_ptr(), label.data_ptr(), logits.shape[0], logits.shape[1], _stream())


def eval_metrics_update(state, scores, labels, offset, logits, label):
    """tmf_eval_metrics_update: loss sum and confusion counts into `state`, scores / labels at `offset` of the epoch buffers."""
    logits = _chk(logits, "logits")
    _lib.call("tmf_eval_metrics_update", state.data_ptr(), scores.data_ptr(), labels.data_ptr(), int(offset), logits.data_ptr(),
              label.data_ptr(), logits.shape[0], logits.shape[1], _stream())


def auc_counts(scores, labels, n, workspace, out):
    """tmf_auc over the first n entries of the epoch buffers: T, P, N (uint64) into the three int64 words of `out`."""
    _lib.call("tmf_auc", scores.data_ptr(), labels.data_ptr(), int(n), workspace.data_ptr(), out.data_ptr(), _stream())
