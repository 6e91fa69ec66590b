"""CPU-only checks of what tests/test_gpu_attention_maps.py stands on and of the host side of transmf_ad_amd.attention_maps:
the recorded restatement distances of tests/_attn_map_inputs.py, what their tolerances reject, attention_maps_torch against the
maps the reference itself builds (tests/golden/attn_maps_*.npz), the rules of the Python API, and the new names in the header
and in _lib.PROTOTYPES."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _attn_map_inputs as mi
from _attn_inputs import case_id
from _golden import GOLDEN_DIR, Golden

MAP_FIXTURES = ("ad_mid", "ad_mid_h8", "ad_d64_mid", "ad_d256_mid")


@pytest.mark.parametrize("case", mi.ATTN_CASES, ids=case_id)
def test_recorded_distances_are_reproduced(case):
    """fp64 P is a softmax (rows sum to 1, recv sums to 1); the recorded distances have not drifted by more than a factor of 2;
    both restatements and the fp64 maps rounded to fp32 pass the tolerances, those of the sums included."""
    inp = mi.attn_inputs(case)
    ref = mi.map_ref(inp)
    assert float((ref["probs"].sum(-1) - 1).abs().max()) < 1e-12 and float((ref["recv"].sum(-1) - 1).abs().max()) < 1e-12
    now, rec = mi.map_restatement_distance(case), mi.ATTN_MAP_DISTANCE[case]
    assert set(now) == set(rec)
    for key in rec:
        a, b = mi.floor_distance(rec[key]), mi.floor_distance(now[key])
        assert a / 2 <= b <= a * 2, f"{case} {key}: recorded {rec[key]:.3e}, measured {now[key]:.3e}"
    for got in (mi.map_restatement(inp, "tree"), mi.map_restatement(inp, "chain"),
                dict(probs=ref["probs"].float(), recv=ref["recv"].float())):
        ratios, sums = mi.map_ratios(got, ref, case), mi.sum_ratios(got, case)
        # a restatement lies within ONE distance (the table holds three digits of it)
        assert max(ratios.values()) <= 1.01 / mi.MARGIN, ratios
        assert max(sums.values()) <= 1.0, sums


@pytest.mark.parametrize("case", [c for c in mi.ATTN_CASES if c[2] % 32], ids=case_id)
def test_tolerances_reject_wrong_maps(case):
    """Three deliberately wrong results in the kernel's place (map_restatement says what each one is) fail the tolerance of
    the quantity they damage - by the value itself, and the two wrong recv also by the sum over the keys."""
    inp = mi.attn_inputs(case)
    ref = mi.map_ref(inp)
    N = case[2]
    for wrong, key in (("pad_rows", ("recv", "all")), ("pad_div", ("recv", "all")), ("ln_lse", ("probs", "flat"))):
        got = mi.map_restatement(inp, "tree", wrong=wrong)
        ratio = mi.map_ratios(got, ref, case)[key]
        print(f"{case_id(case)} {wrong}: err / tol {ratio:.3g}")
        assert ratio > 1.0, (wrong, ratio)
        if key[0] == "recv":
            assert mi.sum_ratios(got, case)[key] > 1.0
    assert N % 32 != 0


def _host_model_ad(g):
    """The package's model_ad with a fixture's weights on the CPU (its encoders cannot run there; the fusion block's
    parameters are what attention_maps_torch reads)."""
    import transmf_ad_amd as T
    net = T.model_ad(dropout=0., **g.kw)
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g.arrays().items()}, strict=True)
    return net.eval()


@pytest.mark.parametrize("name", MAP_FIXTURES)
def test_attention_maps_torch_against_the_reference_maps(name):
    """attention_maps_torch on the tokens the reference's fp32 run handed its fusion block, with the fixture's weights, against
    the probabilities the reference's own nn.Softmax modules returned and their column means: within
    MARGIN x floor_distance(the stored fp32 <-> fp64 distance of the tensor) x max |reference| of the tensor."""
    import transmf_ad_amd as T
    z = np.load(os.path.join(GOLDEN_DIR, f"attn_maps_{name}.npz"))
    g = Golden(name)
    net = _host_model_ad(g)
    mt, pt = torch.from_numpy(z["mri_tok"]), torch.from_numpy(z["pet_tok"])
    before = {k: v.clone() for k, v in net.state_dict().items()}
    maps = T.attention_maps_torch(net, mt, pt, probs=True)
    assert maps.logits is None and maps.grid is None
    depth, B, heads, N = g.kw["depth"], g.batch, g.kw["heads"], mt.shape[1]
    assert tuple(maps.received.shape) == (depth, 2, B, heads, N) == z["recv"].shape
    assert tuple(maps.probs.shape) == (depth, 2, B, heads, N, N) == z["probs"].shape
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert torch.equal(mt, torch.from_numpy(z["mri_tok"]))
    for got, key in ((maps.probs, "probs"), (maps.received, "recv")):
        want = torch.from_numpy(z[key]).double()
        for l in range(depth):
            for s in (0, 1):
                err = float((got[l, s].double() - want[l, s]).abs().max()) / float(want[l, s].abs().max())
                tol = mi.MARGIN * mi.floor_distance(z["dist_" + key][l, s])
                print(f"{name} {key}[{l}, {s}]: err {err:.3e} tol {tol:.3e}")
                assert err <= tol, (key, l, s, err, tol)
    assert T.attention_maps_torch(net.fuse_transformer, mt, pt).probs is None


def _host_model(pools=4, dim=16):
    """A two-stream model that runs on the CPU: a CrossTransformer_MOD_AVG whose own forward is plain torch (the package's runs
    on a HIP device only), tokens from a 1x1x1 convolution and `pools` average poolings."""
    import transmf_ad_amd as T

    class Fusion(T.CrossTransformer_MOD_AVG):
        def forward(self, m, p):
            return torch.cat([m.mean(1), p.mean(1), m.amax(1), p.amax(1)], dim=1)

    class Model(nn.Module):
        def __init__(self):
            super().__init__()
            self.lift = nn.Conv3d(1, dim, 1)
            self.fuse_transformer = Fusion(dim, 2, 2, 8, 32, 0.1)
            self.fc = nn.Linear(4 * dim, 2)
            self.register_buffer("calls", torch.zeros(()))

        def tokens(self, v):
            v = self.lift(v)
            for _ in range(pools):
                v = F.avg_pool3d(v, 2)
            return v.flatten(2).transpose(1, 2)

        def forward(self, mri, pet):
            return self.fc(self.fuse_transformer(self.tokens(mri), self.tokens(pet))), None

    torch.manual_seed(0)
    return Model().eval()


@pytest.mark.parametrize("size,grid", [((32, 32, 32), (2, 2, 2)), ((35, 38, 33), (2, 2, 2)), ((48, 64, 80), (3, 4, 5))])
def test_api_rules_on_a_host_model(size, grid):
    """logits are the model's own, the grid is every side halved four times with floor, received / probs have their shapes
    and sum to 1 over the keys, volume() gives the input's shape (or `size`), nothing of the caller's or the model's changes."""
    import transmf_ad_amd as T
    from transmf_ad_amd.attention_maps import token_grid
    net = _host_model()
    g = torch.Generator().manual_seed(1)
    mri, pet = torch.rand((2, 1) + size, generator=g), torch.rand((2, 1) + size, generator=g)
    m0, p0 = mri.clone(), pet.clone()
    before = {k: v.clone() for k, v in net.state_dict().items()}
    assert token_grid(size) == grid
    N = grid[0] * grid[1] * grid[2]
    for fn in (T.attention_maps, T.attention_maps_torch):        # CPU tensors: attention_maps routes to the torch formula
        maps = fn(net, mri, pet, probs=True)
        with torch.no_grad():
            assert torch.equal(maps.logits, net(mri, pet)[0])
        assert maps.grid == grid and not maps.received.requires_grad
        assert tuple(maps.received.shape) == (2, 2, 2, 2, N) and tuple(maps.probs.shape) == (2, 2, 2, 2, N, N)
        assert float((maps.probs.sum(-1) - 1).abs().max()) < 1e-5 and float((maps.received.sum(-1) - 1).abs().max()) < 1e-5
        assert torch.allclose(maps.probs.mean(-2), maps.received, atol=1e-6)
        assert tuple(maps.volume().shape) == (2,) + size
        assert tuple(maps.volume(layer=0, direction=1, heads=1).shape) == (2,) + size
        assert tuple(maps.volume(heads=None).shape) == (2, 2) + size
        assert tuple(maps.volume(size=(4, 6, 8)).shape) == (2, 4, 6, 8)
        want = F.interpolate(maps.received[-1, 0].mean(1, keepdim=True).reshape(2, 1, *grid), size=size, mode="trilinear",
                             align_corners=False)[:, 0]
        assert torch.equal(maps.volume(), want)
    assert fn(net, mri, pet).probs is None
    assert torch.equal(mri, m0) and torch.equal(pet, p0)
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())
    assert not net.fuse_transformer._forward_pre_hooks


def test_api_refusals():
    import transmf_ad_amd as T
    net = _host_model()
    mri = pet = torch.rand(1, 1, 32, 32, 32)
    net.train()
    with pytest.raises(ValueError, match="eval"):
        T.attention_maps(net, mri, pet)
    with pytest.raises(ValueError, match="eval"):
        T.attention_maps_torch(net, mri, pet)
    assert not net.fuse_transformer._forward_pre_hooks
    with pytest.raises(ValueError, match="grid"):                # three poolings: 4^3 tokens on a 2^3 grid
        T.attention_maps(_host_model(pools=3), mri, pet)
    res = T.model_transformer_res(dim=16, depth=1, heads=2, dim_head=8, mlp_dim=32, dropout=0.).eval()
    with pytest.raises(NotImplementedError, match="CrossTransformer"):
        T.attention_maps(res, mri, pet)
    with pytest.raises(NotImplementedError, match="CrossTransformer"):
        T.attention_maps_torch(res.fuse_transformer, mri, pet)
    with pytest.raises(TypeError):
        T.attention_maps(nn.Linear(2, 2).eval(), mri, pet)


def test_new_names_in_header_and_prototypes():
    from transmf_ad_amd import _lib, ops
    import transmf_ad_amd as T
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "tmf_hip.h")) as f:
        header = f.read()
    want = {"tmf_xattn_probs": 16, "tmf_fusion_attn_maps_workspace_bytes": 1, "tmf_fusion_attn_maps": 10}
    for name, nargs in want.items():
        m = re.search(r"\b" + name + r"\(([^;]*)\);", header)
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert callable(ops.xattn_probs) and callable(ops.fusion_attn_maps)
    assert "attention_maps" in T.__all__ and "attention_maps_torch" in T.__all__
