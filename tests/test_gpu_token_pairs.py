"""One launch per op of the one-call fusion entry (csrc/fusion_path.hip: instance_fwd / instance_bwd) with every subset of
the three Dropout keep-masks of networks.py:153 (to_out), :131 (after GELU) and :133 (after the second Linear) present.
Each token GEMM and the block-final LayerNorm backward take their mask as it comes, NULL or not, and a NULL one must reach
the plain launch: the mixed subsets are the cases that decide it.  R = B N = 10 rows, below the 16-row tile.  Neither
geometry here (mlp 64, 4 heads of 16) is one the fused per-instance kernels take, so none of this reaches them."""
import itertools

import numpy as np
import pytest
import torch

from test_gpu_dims import linear_calls  # noqa: F401  (fixture)
from test_gpu_dropout_dims import _inputs, _keep, _max_rel, _names, _run
from test_gpu_kernels import _FixedMask
from test_gpu_model import DEV

pytestmark = pytest.mark.gpu

B, N, HEADS, DIM_HEAD, MLP = 2, 5, 4, 16, 64
SITES = ("mask_o", "mask_g", "mask_f")
SUBSETS = [tuple(s for s, on in zip(SITES, bits) if on) for bits in itertools.product((False, True), repeat=3)]


def _fusion(dim, subset):
    """CrossTransformer_MOD_AVG(dim, depth 1) with a fixed keep-mask at the Dropout sites named in `subset` of both
    instances; a site's mask is the same whatever the subset."""
    from transmf_ad_amd import networks
    torch.manual_seed(7)
    fz = networks.CrossTransformer_MOD_AVG(dim, 1, HEADS, DIM_HEAD, MLP, 0.).to(DEV).train()
    with torch.no_grad():
        for p in fz.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    rs = np.random.RandomState(3)
    for tr in fz.layers[0]:
        at, ff = tr.layers[0][0].fn, tr.layers[0][1].fn
        masks = dict(mask_o=_keep(rs, B * N, dim), mask_g=_keep(rs, B * N, MLP), mask_f=_keep(rs, B * N, dim))
        if "mask_o" in subset:
            at.to_out[1] = _FixedMask(masks["mask_o"])
        if "mask_g" in subset:
            ff.net[2] = _FixedMask(masks["mask_g"])
        if "mask_f" in subset:
            ff.net[4] = _FixedMask(masks["mask_f"])
        tr._drops = None
    return fz


@pytest.mark.parametrize("subset", SUBSETS, ids=["+".join(s) or "none" for s in SUBSETS])
@pytest.mark.parametrize("dim", [64, 128])
def test_every_mask_subset_on_one_launch_per_op(dim, subset, linear_calls, monkeypatch):
    """FusionTrain forward and backward on the one-launch-per-op path (dim 128: with ops.FUSION_FUSED_KERNELS off as well)
    against one ops.TransformerLayer per Transformer given the same masks — bitwise-equal cls, both token gradients and
    all 28 parameter gradients to fp32 round-off (1e-5 of each tensor's max), the comparison of
    test_gpu_dropout_dims.test_one_call_masks_match_per_transformer_path — and ops.fusion_infer's cls bit-identical to
    FusionTrain's."""
    from transmf_ad_amd import _lib, ops
    if dim == 128:
        monkeypatch.setattr(ops, "FUSION_FUSED_KERNELS", False)
    fz = _fusion(dim, subset)
    m0, p0, go = _inputs(B, N, dim)
    res = []
    for one_call in (True, False):
        monkeypatch.setattr(ops, "FUSION_ONE_CALL", one_call)
        node, used, out = _run(fz, m0, p0, go)
        assert node.startswith("FusionTrain") == one_call, node
        if one_call:
            assert used == 0
        res.append(out)
    monkeypatch.setattr(ops, "FUSION_ONE_CALL", True)
    assert linear_calls[0] == 0
    names = _names(fz)
    assert len(names) == len(res[0]) == len(res[1]) == 3 + 28
    assert torch.equal(res[0][0], res[1][0])
    for name, a, b in zip(names, res[0], res[1]):
        assert torch.isfinite(a).all(), name
        assert _max_rel(a, b) <= 1e-5, (name, _max_rel(a, b))

    calls, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with torch.no_grad():
        cls = fz(m0.to(DEV), p0.to(DEV))
    torch.cuda.synchronize()
    assert calls == ["tmf_fusion_infer_fwd"], calls
    assert torch.equal(cls.cpu(), res[0][0])
