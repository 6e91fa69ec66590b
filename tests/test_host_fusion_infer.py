"""Host-side checks (no GPU) of the forward-only fusion entry (tmf_fusion_infer_fwd, csrc/fusion_path.hip): what its
workspace holds — no per-instance activations — its argument checks (pure host code, nothing launched), the routing
predicate of ops.fusion_infer on CPU tensors, and the registers of the forward-only kernel instances."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

E_NULL, E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3, -4           # include/tmf_hip.h
PACK_BYTES = (4 * 128 * 128 + 2 * 512 * 128) * 4                  # one forward weight pack at dim 128, mlp 512: 786 432


def _desc(dim=128, heads=4, N=216, B=8, depth=3, flags=0):
    from transmf_ad_amd import _lib
    return _lib.FusionDesc(B=B, N=N, dim=dim, heads=heads, dim_head=dim // heads, mlp=4 * dim, depth=depth, flags=flags)


def _ws(d):
    from transmf_ad_amd import _lib
    return _lib.query("tmf_fusion_infer_workspace_bytes", ctypes.byref(d))


def _saved(d):
    from transmf_ad_amd import _lib
    return _lib.query("tmf_fusion_saved_bytes", ctypes.byref(d))


def test_fused_workspace_holds_no_per_instance_activations():
    """B = 8, N = 216, dim 128, 4 x 32, mlp 512: an eighth of what tmf_fusion_train_fwd keeps at most, and an added
    instance costs one forward weight pack (plus its 256-byte granule) and nothing per token."""
    assert PACK_BYTES == 786432
    d3, d6 = _desc(depth=3), _desc(depth=6)
    print("infer workspace", _ws(d3), "saved", _saved(d3))
    assert 0 < _ws(d3) <= _saved(d3) // 8
    assert 0 < _ws(d6) - _ws(d3) <= 6 * (PACK_BYTES + 256)
    h8 = _desc(heads=8)
    assert _ws(h8) == _ws(d3)                   # 8 heads of 16: the same panels


def test_per_op_workspace_does_not_grow_with_depth():
    d3, d6 = _desc(dim=256, depth=3), _desc(dim=256, depth=6)
    assert 0 < _ws(d3) <= _saved(d3) // 4
    assert _ws(d6) == _ws(d3)
    for dim, heads in ((64, 4), (64, 8), (256, 8)):
        assert _ws(_desc(dim=dim, heads=heads, depth=6)) == _ws(_desc(dim=dim, heads=heads, depth=1)) > 0


def test_per_op_flag_at_dim_128_gives_the_per_op_size():
    from transmf_ad_amd import _lib
    fused, per_op = _desc(depth=3), _desc(depth=3, flags=_lib.FUSION_PER_OP)
    assert _lib.query("tmf_fusion_uses_fused", ctypes.byref(per_op)) == 0
    assert _ws(per_op) != _ws(fused)
    assert _ws(per_op) == _ws(_desc(depth=6, flags=_lib.FUSION_PER_OP))          # no weight packs, nothing per instance
    # N beyond the fused kernels' 512 keys: one launch per op whatever the flag says
    assert _ws(_desc(N=600, depth=2)) == _ws(_desc(N=600, depth=2, flags=_lib.FUSION_PER_OP))
    # depth 0 (pooling only): no instance slab is ever touched, the size query still answers
    assert _ws(_desc(depth=0)) > 0


def test_invalid_descriptor_returns_zero_and_sets_the_error_string():
    from transmf_ad_amd import _lib
    for bad in (_desc(dim=96), _desc(depth=17), _desc(B=0), _desc(N=0)):
        assert _ws(bad) == 0
        msg = (_lib.load().tmf_last_error_string() or b"").decode()
        assert "tmf_fusion_infer_workspace_bytes" in msg, msg
    assert _lib.query("tmf_fusion_infer_workspace_bytes", None) == 0


def test_argument_checks_return_before_any_launch():
    """Pointer, alignment, shape and size checks are host code: fake pointers are never touched."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    d = _desc(B=3, N=17, depth=2)
    need = _ws(d)
    inst = (_lib.XformerParams * 4)()
    p = 4096

    def call(desc, mri, pet, ins, ws, nbytes, cls):
        return lib.tmf_fusion_infer_fwd(ctypes.byref(desc), mri, pet, ins, ws, nbytes, cls, None)
    assert call(d, p, p, inst, p, need - 1, p) == E_WORKSPACE
    assert "workspace" in lib.tmf_last_error_string().decode()
    assert call(d, p, p, inst, None, need, p) == E_NULL
    assert call(d, p, p, inst, p, need, None) == E_NULL
    assert call(d, p, p, None, p, need, p) == E_NULL
    assert call(d, None, p, inst, p, need, p) == E_NULL
    assert call(_desc(dim=96), p, p, inst, p, 1 << 30, p) == E_SHAPE
    assert call(d, p + 4, p, inst, p, need, p) == E_ALIGN
    assert call(d, p, p + 8, inst, p, need, p) == E_ALIGN
    assert call(d, p, p, inst, p + 4, need, p) == E_ALIGN
    # a table with NULL parameter pointers is refused as well (after the size check, before the first launch)
    assert call(d, p, p, inst, p, need, p) == E_NULL
    assert "instance 0" in lib.tmf_last_error_string().decode()


def test_cpu_tokens_keep_the_module_path(monkeypatch):
    """ops.fusion_infer serves device tensors only: on CPU tokens the predicate is false whatever the grad mode, and the
    block walks its modules (which refuse CPU tensors: the library has no CPU fallback)."""
    import transmf_ad_amd as T
    from transmf_ad_amd import networks, ops
    assert ops.FUSION_INFER_ONE_CALL == (os.environ.get("TMF_FUSION_INFER_C", "1") != "0")
    calls = []
    monkeypatch.setattr(ops, "fusion_infer", lambda *a, **k: calls.append(1))
    fz = networks.CrossTransformer_MOD_AVG(128, 1, 4, 32, 512, 0.).eval()
    tok = torch.zeros(2, 17, 128)
    with torch.no_grad():
        assert not ops.fusion_infer_ok(tok)
        assert not fz._infer_one_call_ok(tok) and not fz._one_call_ok(tok)
        with pytest.raises(T.TmfError):
            fz(tok, tok)
    assert not ops.fusion_infer_ok(tok) and not fz._infer_one_call_ok(tok)       # grad mode on
    assert calls == []
    monkeypatch.setattr(ops, "FUSION_INFER_ONE_CALL", False)
    with torch.no_grad():
        assert not ops.fusion_infer_ok(tok)


def test_forward_only_kernels_need_no_more_registers_than_training():
    """Every (MT, EXACT, H2) instance of xf_fwd_kernel has its forward-only twin (4th template argument), without scratch
    and with no more registers than the training instance."""
    from tools import resources as R
    obj = os.path.join(R.CSRC, "xformer_fused.o")
    if not os.path.exists(obj):
        pytest.skip("objects not built (python -m transmf_ad_amd.build)")
    if not os.path.exists(f"{R.LLVM}/clang-offload-bundler"):
        pytest.skip("ROCm llvm tools not present")
    ks = {k["name"]: k for k in R.kernels_of(obj) if "xf_fwd_kernel" in k["name"]}
    tail = "EEEvNS_9XfFwdArgsE"
    train = {n: k for n, k in ks.items() if n.endswith("ELb0" + tail)}
    assert len(train) == 12 and len(ks) == 24, sorted(ks)
    for n, t in train.items():
        k = ks[n[:-len("ELb0" + tail)] + "ELb1" + tail]
        assert k.get("scratch", 0) == 0 and k["vgpr"] <= t["vgpr"] and k.get("lds", 0) == t.get("lds", 0), (k, t)
