"""Host-side checks (no GPU) of the reference's remaining model classes (models/mymodel.py:40-141) and of
networks.CrossTransformer (networks.py:233-252): exports, constructors, attribute names and state_dict keys against the
keys the reference itself recorded in the fixtures (tests/golden/make_golden_variants.py), the share=True form, and the
argument checks of the two-part-context attention entries."""
import json
import os

import numpy as np
import pytest
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["res_mid", "res_mid_drop", "res_d64_mid", "res_d256_h8_mid", "res_full_b2", "tr_mid", "cnnp_mid"]


def _meta(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    return json.loads(bytes(z["meta"]).decode())


def _build(meta):
    import transmf_ad_amd as T
    kw = meta["kwargs"]
    if meta["model"] == "model_CNN":
        return T.model_CNN(kw["dim"])
    return getattr(T, meta["model"])(dropout=meta["fusion_dropout"], **kw)


def test_package_exports_the_new_classes():
    import transmf_ad_amd as T
    from transmf_ad_amd.mymodel import model_CNN, model_transformer, model_transformer_res  # noqa: F401
    from transmf_ad_amd.networks import CrossTransformer  # noqa: F401
    for n in ("CrossTransformer", "model_CNN", "model_transformer", "model_transformer_res"):
        assert hasattr(T, n) and n in T.__all__, n


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_keys_and_shapes_match_reference(name):
    """Keys / shapes / order recorded from the imported reference's state_dict() == ours; the fixture's parameters load
    strictly."""
    from oracle import params as P
    meta = _meta(name)
    net = _build(meta)
    assert [[k, list(v.shape)] for k, v in net.state_dict().items()] == meta["keys"]
    spec = {k: (kind, tuple(s)) for (k, s), kind in zip(meta["keys"], meta["kinds"])}
    arrays = P.init_arrays(spec, seed=meta["param_seed"])
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in arrays.items()}, strict=True)
    bufs = {k for k, _ in net.named_buffers()}
    assert [k for k, kind in spec.items() if kind[0] == "buffer"] == [k for k in net.state_dict() if k in bufs]


def test_reference_attributes_and_init():
    import transmf_ad_amd as T
    torch.manual_seed(0)
    res = T.model_transformer_res(128, 3, 4, 32, 512, 0.1)
    assert [type(m) for m in res.fc_cls] == [torch.nn.Linear, torch.nn.ReLU, torch.nn.Dropout] * 2 + [torch.nn.Linear]
    assert res.fc_cls[2].p == 0.5 and res.fc_cls[5].p == 0.5 and res.fc_cls[0].in_features == 256
    assert not list(res.gap.parameters()) and not list(res.gmp.parameters())
    tok = torch.randn(2, 5, 128)
    assert torch.allclose(res.gap(tok), tok.mean(1)) and torch.equal(res.gmp(tok), tok.amax(1))
    assert isinstance(res.fuse_transformer, T.CrossTransformer) and len(res.fuse_transformer.layers) == 3
    assert res.pet_cnn.conv3[4].weight.eq(1).all() and res.pet_cnn.conv3[4].bias.eq(0).all()
    w = res.mri_cnn.conv2[3].weight
    assert abs(w.std().item() / (2.0 / (w.shape[0] * 27)) ** 0.5 - 1) < 0.05
    tr = T.model_transformer(128, 3, 4, 32, 512, 0.)
    assert isinstance(tr.fuse_transformer, T.CrossTransformer_MOD_AVG) and not hasattr(tr, "D") and not hasattr(tr, "gap")
    assert tr.fc_cls[3].p == 0.5 and tr.fc_cls[7].p == 0.5 and tr.fc_cls[0].in_features == 512
    cnn = T.model_CNN(128)
    assert cnn.fc[0].in_features == 256 and cnn.fc[2].out_features == 2 and len(cnn.transform) == 2


def test_cross_transformer_keys_match_the_reference():
    import transmf_ad_amd as T
    meta = _meta("res_mid")
    kw = meta["kwargs"]
    ct = T.CrossTransformer(kw["dim"], kw["depth"], kw["heads"], kw["dim_head"], kw["mlp_dim"], 0.)
    pre = "fuse_transformer."
    assert [[k, list(v.shape)] for k, v in ct.state_dict().items()] == \
        [[k[len(pre):], s] for k, s in meta["keys"] if k.startswith(pre)]


def test_cross_transformer_share_keys_and_its_forward_raises_type_error():
    """share=True: one Transformer per layer, the reference's keys; its forward unpacks a Transformer and raises TypeError,
    as networks.py:249 does."""
    import transmf_ad_amd as T
    meta = _meta("res_mid")
    kw = meta["kwargs"]
    ct = T.CrossTransformer(kw["dim"], kw["depth"], kw["heads"], kw["dim_head"], kw["mlp_dim"], 0., share=True)
    assert ct.share is True
    assert [[k, list(v.shape)] for k, v in ct.state_dict().items()] == meta["cross_share_keys"]
    with pytest.raises(TypeError):
        ct(torch.zeros(1, 3, kw["dim"]), torch.zeros(1, 3, kw["dim"]))


def test_cat_attention_argument_checks_without_gpu():
    """The two-part entries check their shapes and pointers on the host, before any launch."""
    from transmf_ad_amd import _lib
    p = 256
    with pytest.raises(_lib.TmfError, match="context parts"):
        _lib.call("tmf_xattn_fwd_cat", p, p, p, p, p, p, p, 1, 4, 8, 8, 0, 32, 128, 256, 1.0, None)
    with pytest.raises(_lib.TmfError, match="NULL"):
        _lib.call("tmf_xattn_fwd_cat", p, p, p, None, p, p, p, 1, 4, 8, 8, 8, 32, 128, 256, 1.0, None)
    with pytest.raises(_lib.TmfError, match="dim_head"):
        _lib.call("tmf_xattn_fwd_cat", p, p, p, p, p, p, p, 1, 4, 8, 8, 8, 12, 128, 256, 1.0, None)
    with pytest.raises(_lib.TmfError, match="context parts"):
        _lib.call("tmf_xattn_bwd_cat", *([p] * 13), 1, 4, 8, -1, 8, 32, 128, 256, 256, 1.0, None)
    with pytest.raises(_lib.TmfError, match="dkv_stride"):
        _lib.call("tmf_xattn_bwd_cat", *([p] * 13), 1, 4, 8, 8, 8, 32, 128, 256, 130, 1.0, None)
    with pytest.raises(_lib.TmfError, match="aligned"):
        _lib.call("tmf_xattn_fwd_cat", p, p, p, p + 4, p, p, p, 1, 4, 8, 8, 8, 32, 128, 256, 1.0, None)
