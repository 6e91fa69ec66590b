#!/usr/bin/env python3
"""Golden fixtures for the reference's remaining model classes (models/mymodel.py:40-141): model_transformer_res (its
fusion block is networks.CrossTransformer, networks.py:233-252), model_transformer and model_CNN.  Same recipe as
make_golden.py (whose probe helpers it uses): oracle/params inputs, parameters and masks, fc_cls's two Dropout(0.5) forced
to oracle/params.make_masks by forward hooks — at fc_cls[2] / [5] in model_transformer_res, [3] / [7] in
model_transformer — and, with a fusion Dropout p, every Transformer Dropout module forced to make_fusion_masks.  The loss is
CrossEntropy on the logits (these models have no discriminator).  oracle/tmf_oracle.state_spec does not know these
classes: the spec is read from the reference module itself and recorded in `meta` ("keys", "kinds"); res_mid also records
the keys of CrossTransformer(share=True) ("cross_share_keys").  Usage:

    python tests/golden/make_golden_variants.py [case ...]      # default: all cases below
"""
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402
from make_golden import HERE, P, gprobe, probe  # noqa: E402

K128 = dict(dim=128, depth=3, heads=4, dim_head=32, mlp_dim=512)
CASES = {
    # name: (model, ctor kwargs, volume size, batch, fusion Dropout p)
    "res_mid":         ("model_transformer_res", K128, (48, 48, 48), 2, 0.0),
    "res_mid_drop":    ("model_transformer_res", K128, (48, 48, 48), 2, 0.3),
    "tr_mid":          ("model_transformer", K128, (48, 48, 48), 4, 0.0),
    "cnnp_mid":        ("model_CNN", dict(dim=128), (48, 48, 48), 2, 0.0),
    "res_d256_h8_mid": ("model_transformer_res", dict(dim=256, depth=3, heads=8, dim_head=32, mlp_dim=1024), (48, 48, 48), 2,
                        0.0),
    "res_d64_mid":     ("model_transformer_res", dict(dim=64, depth=3, heads=4, dim_head=16, mlp_dim=256), (48, 48, 48), 2, 0.0),
    # 96^3: N = 216 tokens per stream, 432 keys per instance
    "res_full_b2":     ("model_transformer_res", K128, (96, 96, 96), 2, 0.0),
}
HEAD_DROPS = {"model_transformer_res": (2, 5), "model_transformer": (3, 7), "model_CNN": ()}


def build_reference(model, kw, dropout=0.):
    from models import mymodel
    if model == "model_CNN":
        return mymodel.model_CNN(kw["dim"])
    return getattr(mymodel, model)(dropout=dropout, **kw)


def spec_of(net):
    bufs = {k for k, _ in net.named_buffers()}
    return OrderedDict((k, ("buffer" if k in bufs else "param", tuple(v.shape))) for k, v in net.state_dict().items())


def attach_probes(net, store):
    hs = []

    def hook(name):
        def f(_m, _i, o):
            store[name] = probe(o) if torch.is_tensor(o) else np.concatenate([probe(t) for t in o])
        return f
    for c in ("mri_cnn", "pet_cnn"):
        s = getattr(net, c)
        pts = {"conv1.0": s.conv1, "conv2.0": s.conv2[2], "conv2.3": s.conv2, "conv3.0": s.conv3[2],
               "conv3.3": s.conv3, "conv4.0": s.conv4[2], "conv4.3": s.conv4}
        for k, m in pts.items():
            hs.append(m.register_forward_hook(hook(f"{c}.{k}")))
    if hasattr(net, "fuse_transformer"):
        for l, pair in enumerate(net.fuse_transformer.layers):
            for s in (0, 1):
                hs.append(pair[s].register_forward_hook(hook(f"fuse_transformer.layers.{l}.{s}")))
        hs.append(net.fuse_transformer.register_forward_hook(hook("fused")))
    return hs


def run_case(name):
    model, kw, size, B, drop_p = CASES[name]
    torch.manual_seed(0)
    spec = spec_of(build_reference(model, kw, drop_p))
    arrays = P.init_arrays(spec, seed=7)
    mri, pet, y = P.make_inputs(B, size, seed=1234, kind="blobs")
    k1, k2 = P.make_masks(B)
    meta = dict(case=name, model=model, kwargs=kw, size=list(size), batch=B, param_seed=7, input_seed=1234, mask_seed=99,
                input_kind="blobs", torch=torch.__version__, fusion_dropout=drop_p, fusion_mask_seed=123,
                head_dropout=list(HEAD_DROPS[model]), keys=[[k, list(s)] for k, (_kd, s) in spec.items()],
                kinds=[kd for kd, _s in spec.values()])
    if name == "res_mid":
        from models.networks import CrossTransformer
        ct = CrossTransformer(kw["dim"], kw["depth"], kw["heads"], kw["dim_head"], kw["mlp_dim"], 0., share=True)
        meta["cross_share_keys"] = [[k, list(v.shape)] for k, v in ct.state_dict().items()]
    out = {}
    for prec, dt in (("f32", torch.float32), ("f64", torch.float64)):
        t0 = time.time()
        torch.manual_seed(0)
        net = build_reference(model, kw, drop_p)
        net.load_state_dict({k: torch.from_numpy(np.asarray(arrays[k])) for k in spec}, strict=True)
        net = net.to(dt).train()
        pr = {}
        hooks = attach_probes(net, pr)
        for i, km in zip(HEAD_DROPS[model], (k1, k2)):
            mk = torch.from_numpy(km).to(dt)
            hooks.append(net.fc_cls[i].register_forward_hook(lambda _m, inp, _o, mk=mk: inp[0] * mk * 2.0))
        if drop_p > 0:
            tokens = (size[0] // 16) * (size[1] // 16) * (size[2] // 16)
            fm = P.make_fusion_masks(B * tokens, 2 * kw["depth"], drop_p, kw["dim"], kw["mlp_dim"], seed=123)
            inst = 0
            for pair in net.fuse_transformer.layers:
                for tr in pair:
                    at, ff = tr.layers[0][0].fn, tr.layers[0][1].fn
                    for mod, keep in zip((at.to_out[1], ff.net[2], ff.net[4]), fm[inst]):
                        assert isinstance(mod, torch.nn.Dropout) and mod.p == drop_p
                        mk = torch.from_numpy(keep.astype(np.float32) / np.float32(1.0 - drop_p)).to(dt)
                        hooks.append(mod.register_forward_hook(lambda _m, i, _o, mk=mk: i[0] * mk.reshape(i[0].shape)))
                    inst += 1
        lo = net(torch.from_numpy(mri).to(dt), torch.from_numpy(pet).to(dt))
        loss = torch.nn.CrossEntropyLoss()(lo, torch.from_numpy(y))
        loss.backward()
        for h in hooks:
            h.remove()
        out[f"{prec}/train/logits"] = lo.detach().double().numpy()
        out[f"{prec}/train/loss"] = np.float64(loss.item())
        for k, v in pr.items():
            out[f"{prec}/probe/{k}"] = v
        for k, p_ in net.named_parameters():
            out[f"{prec}/grad/{k}"] = gprobe(p_.grad if p_.grad is not None else torch.zeros_like(p_))
        if prec == "f32":
            for k, b in net.named_buffers():
                out[f"f32/buf/{k}"] = b.detach().double().numpy()
        print(f"  {name} {prec} train: loss={loss.item():.8f}  ({time.time() - t0:.1f}s)", flush=True)
        del net
    net = build_reference(model, kw, drop_p)
    net.load_state_dict({k: torch.from_numpy(np.asarray(arrays[k])) for k in spec}, strict=True)
    net.eval()
    with torch.no_grad():
        out["f32/eval/logits"] = net(torch.from_numpy(mri), torch.from_numpy(pet)).double().numpy()
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, f"{name}.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KB)")


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    for c in (sys.argv[1:] or list(CASES)):
        run_case(c)
