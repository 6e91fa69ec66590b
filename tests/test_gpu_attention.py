"""attention.hip called on its own (tmf_xattn_fwd / _bwd / _fwd_cat / _bwd_cat through _lib.call with raw pointers, nothing of
ops.py in between) against the fp64 reference of tests/_attn_inputs.py, at the shapes that reach each boundary of the three
kernels, with flat, peaked, low (every logit -100) and high (every logit +100) query rows in one tensor and in three memory
layouts.

out, lse and dq are judged per query row and head, dk and dv per key row and head:
    |kernel - fp64| <= margin x floor_distance(ATTN_DISTANCE[case][quantity, class]) x max |fp64| of the row;
a dk row in two column groups (the reserved shift and tag features, the Gaussian features), each against the largest sum of the
magnitudes of its terms in place of max |fp64| (attn_distances of tests/_attn_inputs.py says why).
Every buffer lives in the Arena of tests/test_gpu_bn_reduce.py: bytes outside the outputs (the gap columns of a wide dk / dv
buffer included) must be unchanged, every output element written and finite; the columns around a q / k / v block and the
bands around the inputs hold NaN, so a read outside a block shows in the result."""
import functools

import pytest
import torch

import _attn_inputs as ai
from test_gpu_bn_reduce import Arena, _call, _st

pytestmark = pytest.mark.gpu
F32 = torch.float32


@functools.lru_cache(maxsize=None)
def _case(case):
    """Inputs and fp64 reference of one case (shared by the tests; never modified)."""
    inp = ai.attn_inputs(case)
    return inp, ai.attn_ref(inp)


def _run(case, cat, source):
    """The entries of one case on one arena: `cat` - the _cat entries on the two parts, else the one-buffer entries on the
    whole context; source "kernel" - forward twice, then the backward twice on the first forward's own out / lse; source
    "fp64" - the backward once on the fp64 out / lse rounded to fp32.
    -> {name: (B, heads, rows, dh) / lse (B, heads, N)}, the second call's results under name + "_again"."""
    B, heads, N, M1, M2, dh = case
    M, inner = M1 + M2, heads * dh
    inp, ref = _case(case)
    cols = ai.layout_columns(case)
    parts = [(0, M1), (M1, M)] if cat else [(0, M)]
    k, v = ai.to_mem(inp["k"]), ai.to_mem(inp["v"])
    ins = dict(ai.place([(ai.to_mem(inp["q"]), cols["q"])], N, B), dout=ai.to_mem(inp["dout"]).contiguous())
    for i, (a, b) in enumerate(parts):
        for buf, t in ai.place([(k[:, a:b], cols["k"]), (v[:, a:b], cols["v"])], b - a, B).items():
            ins[f"{buf}{i}"] = t
    if source == "fp64":
        ins.update(out_in=ai.to_mem(ref["out"]).float().contiguous(), lse_in=ref["lse"].float().contiguous())
    runs = ("", "_again") if source == "kernel" else ("",)
    outs, written = {}, {}
    for tag in runs:
        if source == "kernel":
            outs.update({"out" + tag: ((B, N, inner), F32), "lse" + tag: ((B, heads, N), F32)})
        outs["dq" + tag] = ((B, N, inner), F32)
        for i, (a, b) in enumerate(parts):
            for name in ("dk", "dv"):
                buf, width, col = cols[name]
                slot = f"{buf}{i}{tag}"
                outs[slot] = ((B, b - a, width), F32)
                written.setdefault(slot, torch.zeros((B, b - a, width), dtype=torch.bool))[:, :, col:col + inner] = True
    q_stride, kv_stride, dkv_stride = cols["q"][1], cols["k"][1], cols["dk"][1]
    arena = Arena(ins, outs, tail=64 * max(q_stride, kv_stride, dkv_stride) * 4)

    def at(name, part=None, tag=""):
        buf, _width, col = cols[name]
        return arena.ptr(buf if part is None else f"{buf}{part}{tag}") + 4 * col

    scale = inp["scale"]
    kv_args = [at(n, i) for i in range(len(parts)) for n in ("k", "v")]
    m_args = [M1, M2] if cat else [M]
    for tag in runs:
        if source == "kernel":
            _call("tmf_xattn_fwd_cat" if cat else "tmf_xattn_fwd", at("q"), *kv_args, arena.ptr("out" + tag), arena.ptr("lse" + tag),
                  B, heads, N, *m_args, dh, q_stride, kv_stride, scale, _st())
    saved = (arena.ptr("out"), arena.ptr("lse")) if source == "kernel" else (arena.ptr("out_in"), arena.ptr("lse_in"))
    for tag in runs:
        dkv_args = [at(n, i, tag) for i in range(len(parts)) for n in ("dk", "dv")]
        _call("tmf_xattn_bwd_cat" if cat else "tmf_xattn_bwd", at("q"), *kv_args, *saved, arena.ptr("dout"), arena.ptr("dq" + tag),
              *dkv_args, B, heads, N, *m_args, dh, q_stride, kv_stride, dkv_stride, scale, _st())
    back = arena.fetch(may_nan=tuple(outs), written=written)    # finiteness is judged below, per row and class
    res = {}
    for tag in runs:
        if source == "kernel":
            res["out" + tag], res["lse" + tag] = ai.to_heads(back["out" + tag], heads), back["lse" + tag]
        res["dq" + tag] = ai.to_heads(back["dq" + tag], heads)
        for name in ("dk", "dv"):
            buf, _width, col = cols[name]
            rows = torch.cat([back[f"{buf}{i}{tag}"][:, :, col:col + inner] for i in range(len(parts))], 1)
            res[name + tag] = ai.to_heads(rows, heads)
    return res


def _judge(case, res, names):
    """Print the worst err / tolerance per quantity and class; -> the (quantity, class) pairs beyond their tolerance."""
    got = {n: res.get(n, _case(case)[1][n]) for n in ai.ATTN_QUANTITIES}
    bad = []
    for (name, cls), ratio in ai.attn_ratios(got, _case(case)[1], case).items():
        if name not in names:
            continue
        print(f"{ai.case_id(case)} {ai.attn_layout(case)} {name} {cls}: err / tol {ratio:.3f}")
        if not ratio <= 1.0:
            bad.append((name, cls, f"{ratio:.3g}"))
    return bad


@pytest.mark.parametrize("source", ("kernel", "fp64"))
@pytest.mark.parametrize("case", ai.ATTN_CASES, ids=ai.case_id)
def test_attention_against_fp64(case, source):
    """source "kernel": forward and backward, the backward fed the forward kernel's own out / lse, each called twice with
    bit-identical results.  source "fp64": the backward alone, fed the fp64 out / lse rounded to fp32, so that a forward error
    cannot hide a backward one.  Two-part cases run the _cat entries and, on the concatenated context in the same layout, the
    one-buffer entries: every output bit-identical.  Then every output finite and within its per-row tolerance.
    Before the dQ kernel masked the zero-filled key rows of its last tile, every case with low rows and M % 32 != 0 failed here
    with "dq is not finite in ... rows (classes ['low'])"."""
    M2 = case[4]
    names = ai.ATTN_QUANTITIES if source == "kernel" else ("dq", "dk", "dv")
    res = _run(case, M2 > 0, source)
    one = _run(case, False, source) if M2 > 0 else None
    bad = _judge(case, res, names)
    for n in names:
        rows = ~torch.isfinite(res[n].reshape(*res[n].shape[:3], -1)).all(-1)
        hit = sorted(set(rows.nonzero()[:, 2].tolist()))
        assert not hit, f"{n} is not finite in {len(hit)} rows, the first {hit[:8]}" + \
                        (f" (classes {sorted({ai.ATTN_CLASSES[r % 4] for r in hit})})" if n in ("out", "lse", "dq") else "")
    for n in names:
        if source == "kernel":
            assert torch.equal(res[n], res[n + "_again"]), f"{n}: two calls differ"
        if one is not None:
            assert torch.equal(res[n], one[n]), f"{n}: the _cat entry differs from the one-buffer entry on the concatenated context"
    assert not bad, f"{case} {source}: {bad} beyond their tolerance"
