"""CPU-only checks of what tests/test_gpu_xf.py stands on: the fp64 reference of tests/_xf_inputs.py against _fusion64 of
tests/test_gpu_kernels.py and against autograd, the query-row classes the construction promises, the near-tie cap of the max
pool, every recorded restatement distance - and what the tolerances are worth: five deliberately wrong results, each built
from the reference, must fail at least one judged quantity in every case they apply to."""
import pytest
import torch

import _xf_inputs as xi


def test_case_table_reaches_every_boundary():
    """The table is the one the kernels' boundaries ask for: one token, the control, a ragged second tile at depth 2, three key
    tiles, B of 9 and 17, and both sides of every N at which xformer_fused.hip picks another forward instance."""
    shapes = [c[:3] for c in xi.XF_CASES]
    assert shapes[:6] == [(1, 1, 1), (3, 16, 1), (2, 17, 2), (2, 33, 1), (9, 40, 1), (17, 20, 1)]
    assert [c[3] for c in xi.XF_CASES[:6]] == [False, False, False, True, False, True]
    edges = [128, 129, 144, 145, 160, 161, 208, 209, 216, 225, 256, 257, 496, 497, 512]
    assert [n for _b, n, _d in shapes[6:]] == edges
    assert [c for c in xi.XF_CASES if c[3]][2:] == [(1, 160, 1, True), (2, 216, 2, True), (1, 512, 1, True)]
    assert all(c == ((2, 216, 2, True) if c[1] == 216 else (1, c[1], 1, c[3])) for c in xi.XF_CASES[6:])
    assert set(xi.XF_DISTANCE) == {(c, h) for c in xi.XF_CASES for h, _dh in xi.XF_HEADS}
    assert (33 + 15) // 16 == 3 and (40 + 15) // 16 == 3           # key-tile counts that are multiples of three
    for N in (1, 16, 512):
        hit = {xi.planted_key(N, r) for r in range(1, N, 4)}
        assert N < 8 or hit == set(xi.planted_keys(N)) == {0, N - 1}


def _module64(inp, heads):
    """CrossTransformer_MOD_AVG in fp64 on the CPU holding the parameters and keep-masks of `inp`."""
    from test_gpu_kernels import _FixedMask
    from transmf_ad_amd import networks
    h, dh = heads
    fz = networks.CrossTransformer_MOD_AVG(xi.DIM, len(inp["params"]) // 2, h, dh, xi.MLP, 0.).double().train()
    trs = [tr for pair in fz.layers for tr in pair]
    with torch.no_grad():
        for k, (tr, p) in enumerate(zip(trs, inp["params"])):
            at, ff = tr.layers[0][0].fn, tr.layers[0][1].fn
            at.scale = xi.f32(dh ** -0.5)                # the C float the entries compute with
            dst = dict(ln1_g=tr.layers[0][0].norm.weight, ln1_b=tr.layers[0][0].norm.bias, wq=at.to_q.weight, wkv=at.to_kv.weight,
                       wo=at.to_out[0].weight, bo=at.to_out[0].bias, ln2_g=tr.layers[0][1].norm.weight,
                       ln2_b=tr.layers[0][1].norm.bias, w1=ff.net[0].weight, b1=ff.net[0].bias, w2=ff.net[3].weight,
                       b2=ff.net[3].bias, lnf_g=tr.norm.weight, lnf_b=tr.norm.bias)
            for name in xi.PARAM_NAMES:
                dst[name].copy_(p[name].double())
            for ln in (tr.layers[0][0].norm, tr.layers[0][1].norm, tr.norm):
                ln.eps = xi.f32(xi.EPS)
            if inp["masks"] is not None:
                mo, mg, mf = inp["masks"][k]
                at.to_out[1], ff.net[2], ff.net[4] = _FixedMask(mo), _FixedMask(mg), _FixedMask(mf)
    return fz


@pytest.mark.parametrize("case", xi.XF_CASES, ids=xi.case_id)
def test_reference_inputs_and_recorded_distances(case):
    """Per head geometry: xf_ref at fp64 is _fusion64 on the module (cls) and autograd through torch's own softmax, layer_norm
    and gelu (every judged quantity), to 1e-10 of each tensor's scale; dwq_terms and the token gradients' terms are never below
    |fp64|, and the fp64 dwq rows of feature 0 are below 1e-12 of their terms - the cancellation xf_row_errors speaks of.
    Layer 0's instances have the four classes: flat rows |logit| < 16, peaked rows a planted probability >= 1 - 1e-6, low rows
    every logit in [-125, -75], high rows in [75, 125] (printed for every instance).  At most TIE_CAP of the max-pool columns
    are near ties, and the near-tie gap is at least 8 x MARGIN recorded forward distances in absolute terms, so a kernel within
    tolerance cannot flip a column that was kept.  The recorded distances have not drifted by more than a factor of 2."""
    from test_gpu_kernels import _fusion64
    B, N, depth, _masks = case
    cls = xi.xf_class(N)
    for heads in xi.XF_HEADS:
        h, dh = heads
        tag = f"{xi.case_id(case)} {h}x{dh}"
        inp = xi.xf_inputs(case, heads)
        ref = xi.xf_ref(inp, heads)

        def close(a, b, what):
            assert a.shape == b.shape, what
            assert float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max())), (tag, what)
        close(ref["cls"], _fusion64(_module64(inp, heads), inp["mri"].double(), inp["pet"].double()).detach(), "cls, _fusion64")
        c, dm, dp, grads = xi.xf_autograd(inp, heads)
        close(ref["cls"], c, "cls")
        close(ref["dmri_tok"], dm, "dmri_tok")
        close(ref["dpet_tok"], dp, "dpet_tok")
        for k, g in enumerate(grads):
            for name in xi.WEIGHTS:
                close(ref[f"i{k}.{name}"], g[name[1:]], f"i{k}.{name}")
            close(ref[f"i{k}.small"], torch.cat([g[n] for n, _w in xi.SMALL_SEGMENTS]), f"i{k}.small")
            close(ref[f"i{k}.lnf"], torch.cat([g[n] for n, _w in xi.LNF_SEGMENTS]), f"i{k}.lnf")
            for name in ("dwq", "dwkv", "small", "lnf"):
                assert bool((ref[f"i{k}.{name}_terms"] >= ref[f"i{k}.{name}"].abs() * (1 - 1e-9)).all()), (tag, k, name)
        for name in ("dmri_tok", "dpet_tok"):
            assert bool((ref[name + "_terms"] >= ref[name].abs()).all())
        if N > 1:
            shift_rows = [hh * dh for hh in range(h)]
            for k in (0, 1):
                a, t = ref[f"i{k}.dwq"][shift_rows].abs().amax(-1), ref[f"i{k}.dwq_terms"][shift_rows].amax(-1)
                assert bool((a <= 1e-12 * t).all()), (tag, k, a / t)
        # the classes
        for k, s in enumerate(ref["fwd"]["saved"]):
            lg = s["logit"]
            print(f"{tag} instance {k}: " + ", ".join(f"{name} [{float(lg[:, :, cls == c_].min()):.1f}, {float(lg[:, :, cls == c_].max()):.1f}]"
                                                      for c_, name in enumerate(xi.XF_CLASSES) if bool((cls == c_).any())))
            if k > 1:
                continue
            assert float(lg[:, :, cls == 0].abs().max()) < 16
            rows = list(range(1, N, 4))
            if rows:
                keys = torch.tensor([xi.planted_key(N, r) for r in rows]).view(1, 1, -1, 1).expand(B, h, -1, 1)
                assert float(s["P"][:, :, rows].gather(-1, keys).min()) >= 1 - 1e-6
            if N > 2:
                assert -125 < float(lg[:, :, cls == 2].min()) and float(lg[:, :, cls == 2].max()) < -75
            if N > 3:
                assert 75 < float(lg[:, :, cls == 3].min()) and float(lg[:, :, cls == 3].max()) < 125
        # near ties of the max pool
        rec = xi.XF_DISTANCE[(case, h)]
        print(f"{tag}: near-tie share {inp['tie_share']:.4f}")
        assert inp["tie_share"] <= xi.TIE_CAP
        assert not bool(inp["dcls"].view(B, 4, xi.DIM)[:, 2:][inp["ties"]].any())
        assert N == 1 or bool(inp["ties"][:, :, 0].all())                  # column 0 is constant: an exact tie
        gap = xi.TIE_GAP * min(float(ref["fwd"]["mri"].abs().max()), float(ref["fwd"]["pet"].abs().max()))
        halves = ref["cls"].view(B, 2, 2 * xi.DIM).abs().amax((0, 2))
        fwd = max(xi.floor_distance(rec[("cls", "mean")]) * float(halves[0]), xi.floor_distance(rec[("cls", "max")]) * float(halves[1]))
        assert gap >= 8 * xi.MARGIN * fwd, (tag, gap, fwd)
        # drift
        now = xi.xf_restatement_distance(case, heads)
        assert set(now) == set(rec)
        for key in rec:
            a, b = xi.floor_distance(rec[key]), xi.floor_distance(now[key])
            assert a / 2 <= b <= a * 2, f"{tag} {key}: recorded {rec[key]:.3e}, measured {now[key]:.3e}"


@pytest.mark.parametrize("case", xi.XF_CASES, ids=xi.case_id)
def test_tolerances_reject_wrong_results(case):
    """The fp64 reference rounded to fp32 passes every tolerance.  Each of these, built from the reference, fails at least
    one: one zero-logit padded key admitted to the softmax of instance 0, forward and backward; delta of its last query row
    taken as 0; batch element 8 given batch element 0's K / V panel (B > 8); the last token's row of dkv left out of dctx;
    one max-pool column routed to the runner-up token (N > 1).  Printed: the worst err / tol and the quantity that has it."""
    B, N, _depth, _masks = case
    for heads in xi.XF_HEADS:
        tag = f"{xi.case_id(case)} {heads[0]}x{heads[1]}"
        inp = xi.xf_inputs(case, heads)
        ref = xi.xf_ref(inp, heads)

        def ratios(res):
            return xi.xf_ratios({k: v.float() for k, v in res.items() if torch.is_tensor(v)}, ref, case, heads)
        clean = ratios(ref)
        assert max(clean.values()) <= 1.0, (tag, max(clean, key=clean.get))
        for wrong in xi.WRONG:
            if (wrong == "batch element" and B <= 8) or (wrong == "argmax" and N == 1):
                continue
            r = ratios(xi.xf_ref(inp, heads, wrong=wrong))
            worst = max(r, key=r.get)
            print(f"{tag} {wrong}: err / tol {r[worst]:.3g} in {worst}, {sum(v > 1 for v in r.values())} of {len(r)} quantities fail")
            assert r[worst] > 1.0, (tag, wrong)
