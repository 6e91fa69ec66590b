"""Host-side checks (no GPU) of the fusion block at the reference's other `--dim` settings: the one-call fusion entries
and the per-Transformer token_gemm path take dim 64 and 256 in both head geometries of the reference's drivers, and
every other dim keeps its old path."""
import ctypes

import pytest

# (dim, heads): 4 heads of dim / 4 (kfold_train_adversarial.py:78-79) and 8 heads of dim / 8 (train_adversarial.py:30-31)
GEOMETRIES = [(64, 4), (64, 8), (256, 4), (256, 8)]


def _desc(dim, heads, N=216, B=2, depth=3):
    from transmf_ad_amd import _lib
    return _lib.FusionDesc(B=B, N=N, dim=dim, heads=heads, dim_head=dim // heads, mlp=4 * dim, depth=depth, flags=0)


@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_fusion_entries_take_dims_64_and_256(dim, heads):
    from transmf_ad_amd import _lib
    d = _desc(dim, heads)
    assert _lib.query("tmf_fusion_saved_bytes", ctypes.byref(d)) > 0
    assert _lib.query("tmf_fusion_bwd_scratch_bytes", ctypes.byref(d)) > 0
    # the fused per-instance kernels stay dim-128 only: these dims run one launch per op
    assert _lib.query("tmf_fusion_uses_fused", ctypes.byref(d)) == 0


def test_other_dims_keep_their_path():
    from transmf_ad_amd import _lib
    for dim, heads in ((96, 4), (32, 4), (192, 4)):
        d = _desc(dim, heads)
        assert _lib.query("tmf_fusion_saved_bytes", ctypes.byref(d)) == 0, dim
    # dim 128 keeps the fused per-instance kernels
    assert _lib.query("tmf_fusion_uses_fused", ctypes.byref(_desc(128, 4))) == 1


@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_ops_predicates_follow_the_library(dim, heads):
    from transmf_ad_amd import ops
    inner, mlp = dim, 4 * dim
    assert ops.fused_block_supported(dim, inner, mlp)
    assert ops.fusion_one_call_supported(dim, inner, mlp, dim // heads, 3)
    assert not ops.fusion_fused_supported(216, dim, heads, dim // heads, mlp)
    for other in (32, 96, 192):
        assert not ops.fused_block_supported(other, other, 4 * other)
        assert not ops.fusion_one_call_supported(other, other, 4 * other, other // 4, 3)


def test_token_linear_shape_checks_without_gpu():
    """The widths the token GEMMs take are checked on the host, before any launch (the pointers are never touched)."""
    from transmf_ad_amd import _lib
    p = 256
    with pytest.raises(_lib.TmfError, match="LayerNorm prologue"):
        _lib.call("tmf_tok_linear_fwd", p, p, None, None, p, 16, 96, 128, p, p, 1e-5, p, p, None, None, None)
    with pytest.raises(_lib.TmfError, match="multiple of 64"):
        _lib.call("tmf_tok_linear_fwd", p, p, None, None, p, 16, 64, 96, None, None, 0.0, None, None, None, None, None)
    with pytest.raises(_lib.TmfError, match="LayerNorm-backward"):
        _lib.call("tmf_tok_linear_bwd_input", p, p, p, 16, 64, 192, None, p, p, p, p, None, None, None, None, 0, None)
    with pytest.raises(_lib.TmfError, match="multiple of 64"):
        _lib.call("tmf_tok_linear_bwd_input", p, p, p, 16, 64, 96, None, None, None, None, None, None, None, None, None, 0,
                  None)
