"""Host-side checks (no GPU) of fusion-block Dropout at every dim the token GEMMs take: the one-call entry takes keep-masks
for each geometry it accepts, and the masked token-GEMM / LayerNorm-backward entries check their arguments on the host,
before any launch (the pointers are never touched)."""
import ctypes

import pytest

GEOMETRIES = [(64, 4), (64, 8), (128, 4), (128, 8), (256, 4), (256, 8)]


def _desc(dim, heads, N=216, B=2, depth=3, flags=0):
    from transmf_ad_amd import _lib
    return _lib.FusionDesc(B=B, N=N, dim=dim, heads=heads, dim_head=dim // heads, mlp=4 * dim, depth=depth, flags=flags)


@pytest.mark.parametrize("dim,heads", GEOMETRIES)
def test_fusion_takes_masks_at_every_token_gemm_dim(dim, heads):
    from transmf_ad_amd import _lib, ops
    for N in (5, 216, 729):                     # 729 > 512: beyond the fused per-instance kernels at dim 128
        for flags in (0, _lib.FUSION_PER_OP):
            d = _desc(dim, heads, N=N, flags=flags)
            assert _lib.query("tmf_fusion_takes_masks", ctypes.byref(d)) == 1, (N, flags)
            assert _lib.query("tmf_fusion_bwd_scratch_bytes", ctypes.byref(d)) > 0
    assert ops.fusion_takes_masks(dim, dim, 4 * dim, dim // heads)
    if dim != 128:              # masks do not move these dims onto the fused per-instance kernels
        assert _lib.query("tmf_fusion_uses_fused", ctypes.byref(_desc(dim, heads))) == 0
        assert not ops.fusion_fused_supported(216, dim, heads, dim // heads, 4 * dim)


def test_other_dims_take_no_masks():
    from transmf_ad_amd import _lib, ops
    for dim in (32, 96, 192, 512):
        assert _lib.query("tmf_fusion_takes_masks", ctypes.byref(_desc(dim, 4))) == 0, dim
        assert not ops.fusion_takes_masks(dim, dim, 4 * dim, dim // 4), dim
    assert not ops.fusion_takes_masks(128, 96, 512, 24)          # inner not a multiple of 64


def _rc(excinfo):
    return int(str(excinfo.value).split("rc=")[1].split(")")[0])


def test_masked_token_linear_checks_without_gpu():
    from transmf_ad_amd import _lib
    p = 256
    # forward: mask NULL, then the shape rules of tmf_tok_linear_fwd
    with pytest.raises(_lib.TmfError, match="'mask' is NULL") as e:
        _lib.call("tmf_tok_linear_fwd_masked", p, p, None, None, p, 16, 64, 64, None, None, 0.0, None, None, None, None, None,
                  None)
    assert _rc(e) == -1                                          # TMF_E_NULL
    with pytest.raises(_lib.TmfError, match="LayerNorm prologue") as e:
        _lib.call("tmf_tok_linear_fwd_masked", p, p, None, None, p, 16, 96, 128, p, p, 1e-5, p, p, None, p, p, None)
    assert _rc(e) == -2                                          # TMF_E_SHAPE
    with pytest.raises(_lib.TmfError, match="multiple of 64") as e:
        _lib.call("tmf_tok_linear_fwd_masked", p, p, None, None, p, 16, 64, 96, None, None, 0.0, None, None, None, None, p, None)
    assert _rc(e) == -2
    with pytest.raises(_lib.TmfError, match="takes no residual") as e:
        _lib.call("tmf_tok_linear_fwd_masked", p, p, None, p, p, 16, 64, 64, None, None, 0.0, None, None, None, p, p, None)
    assert _rc(e) == -2
    # backward: mask NULL, the LayerNorm-backward widths, exactly one epilogue, the masked copy of the LayerNorm epilogue
    with pytest.raises(_lib.TmfError, match="'mask' is NULL") as e:
        _lib.call("tmf_tok_linear_bwd_input_masked", p, p, p, 16, 64, 64, p, None, None, None, None, None, None, None, None, 0,
                  None, None, None)
    assert _rc(e) == -1
    with pytest.raises(_lib.TmfError, match="LayerNorm-backward epilogue needs K") as e:
        _lib.call("tmf_tok_linear_bwd_input_masked", p, p, p, 16, 64, 192, None, p, p, p, p, None, None, None, None, 0,
                  p, p, None)
    assert _rc(e) == -2
    with pytest.raises(_lib.TmfError, match="exactly one") as e:
        _lib.call("tmf_tok_linear_bwd_input_masked", p, p, p, 16, 64, 64, None, None, None, None, None, None, None, None, None,
                  0, p, None, None)
    assert _rc(e) == -2
    with pytest.raises(_lib.TmfError, match="'dx_masked' is NULL") as e:
        _lib.call("tmf_tok_linear_bwd_input_masked", p, p, p, 16, 64, 64, None, p, p, p, p, None, None, None, None, 0,
                  p, None, None)
    assert _rc(e) == -1
    with pytest.raises(_lib.TmfError, match="multiple of 64") as e:
        _lib.call("tmf_tok_linear_bwd_input_masked", p, p, p, 16, 64, 96, p, None, None, None, None, None, None, None, None, 0,
                  p, None, None)
    assert _rc(e) == -2


def test_masked_layernorm_backward_and_mask_mul_checks_without_gpu():
    from transmf_ad_amd import _lib
    p = 256
    with pytest.raises(_lib.TmfError, match="'mask' is NULL") as e:
        _lib.call("tmf_layernorm_bwd_masked", p, p, p, p, p, p, p, 16, 64, None, p, None)
    assert _rc(e) == -1
    with pytest.raises(_lib.TmfError, match="'dx_masked' is NULL") as e:
        _lib.call("tmf_layernorm_bwd_masked", p, p, p, p, p, p, p, 16, 64, p, None, None)
    assert _rc(e) == -1
    with pytest.raises(_lib.TmfError, match="rows=0") as e:
        _lib.call("tmf_layernorm_bwd_masked", p, p, p, p, p, p, p, 0, 64, p, p, None)
    assert _rc(e) == -2
    with pytest.raises(_lib.TmfError, match="exceeds") as e:
        _lib.call("tmf_layernorm_bwd_masked", p, p, p, p, p, p, p, 16, 4096, p, p, None)
    assert _rc(e) == -2
    with pytest.raises(_lib.TmfError, match="'mask' is NULL") as e:
        _lib.call("tmf_mask_mul", p, None, p, 64, None)
    assert _rc(e) == -1
    with pytest.raises(_lib.TmfError, match="16-byte aligned") as e:
        _lib.call("tmf_mask_mul", p + 4, p, p, 64, None)
    assert _rc(e) == -3                                          # TMF_E_ALIGN
    with pytest.raises(_lib.TmfError, match="n=0") as e:
        _lib.call("tmf_mask_mul", p, p, p, 0, None)
    assert _rc(e) == -2
