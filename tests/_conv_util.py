"""What the convolution GPU tests share: the lazily imported package modules, seeded host tensors, the two activation
layouts and the relative maximum error against a wider reference."""
import numpy as np
import torch


def _ops():
    from transmf_ad_amd import ops
    return ops


def _lib():
    from transmf_ad_amd import _lib
    return _lib


def _rand(*shape, seed=0, scale=1.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def _ndhwc(x):      # (B,C,D,H,W) -> (B,D,H,W,C) contiguous
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _ncdhw(x):
    return x.permute(0, 4, 1, 2, 3).contiguous()


def _relerr(got, ref):
    ref = ref.double()
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
