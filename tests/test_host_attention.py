"""CPU-only checks of what tests/test_gpu_attention.py stands on: the fp64 reference of tests/_attn_inputs.py against autograd,
the properties the generator promises (planted probabilities, shifted rows and their twins, classes, planted positions,
layouts), every recorded restatement distance, the time each reference takes - and the argument checks of the four attention
entries, which refuse a call before any launch."""
import time

import pytest
import torch

import _attn_inputs as ai


def test_case_table_reaches_every_boundary_layout_and_planted_position():
    """The table is the one the kernels' boundaries ask for (the comment above ATTN_CASES names them), every layout occurs
    twice and with a two-part case, and every planted position is claimed by some case and targeted where it is claimed."""
    one = [(1, 1, 1, 1, 0, 8), (2, 3, 33, 31, 0, 8), (1, 2, 65, 129, 0, 16), (1, 1, 64, 512, 0, 32), (1, 1, 70, 513, 0, 32),
           (2, 2, 40, 257, 0, 64), (1, 2, 257, 40, 0, 64), (1, 1, 513, 70, 0, 16), (1, 4, 216, 216, 0, 32)]
    two = [(1, 2, 37, 1, 1, 8), (2, 2, 50, 33, 30, 16), (1, 1, 64, 255, 2, 64), (1, 4, 216, 216, 216, 32)]
    assert ai.ATTN_CASES == one + two and set(ai.ATTN_DISTANCE) == set(ai.ATTN_CASES)
    for lay in ai.ATTN_LAYOUTS:
        assert sum(ai.attn_layout(c) == lay for c in ai.ATTN_CASES) >= 2
        assert any(ai.attn_layout(c) == lay for c in two)
    # every planted position is claimed by some case, and where it is claimed a peaked row targets it
    claimed = set()
    for c in ai.ATTN_CASES:
        _B, _h, N, M1, M2, dh = c
        M, keys = M1 + M2, ai.planted_keys(c)
        names = {0: "first", M - 1: "last", 128: "chunk", ai.resident_cap(dh): "cap"}
        if M2:
            names[M1] = "part2"
        assert keys[0] == 0 and all(k in names and k < M for k in keys)
        hit = {ai.planted_key(c, r) for r in range(1, N, 4)}
        assert N < 2 or hit == set(keys), (c, hit, keys)
        claimed |= {names[k] for k in hit}
    assert claimed == {"first", "last", "chunk", "cap", "part2"}


@pytest.mark.parametrize("case", ai.ATTN_CASES, ids=ai.case_id)
def test_reference_inputs_and_recorded_distances(case):
    """attn_ref at fp64 is autograd through torch.softmax (1e-12 of each tensor's scale); the planted key of every peaked row
    holds probability >= 1 - 1e-6; low rows have a base-2 log-sum-exp below -130 and high rows above +130; every class the
    shape has occurs; a shifted row has the out of its flat twin; dq and dk of a one-key context are exactly zero; the fp64
    reference takes under 2 s; the recorded restatement distances have not drifted by more than a factor of 2."""
    B, heads, N, M1, M2, dh = case
    inp = ai.attn_inputs(case)
    t0 = time.perf_counter()
    ref = ai.attn_ref(inp)
    t_ref = time.perf_counter() - t0
    print(f"attention {case}: fp64 reference {t_ref * 1e3:.1f} ms")
    assert t_ref < 2.0
    auto = ai.attn_autograd(inp)
    assert set(ref) == set(ai.ATTN_QUANTITIES) | {"dk_terms"}
    assert bool((ref["dk_terms"] >= ref["dk"].abs() * (1 - 1e-12)).all())
    for name in ai.ATTN_QUANTITIES:
        assert ref[name].shape == auto[name].shape
        assert float((ref[name] - auto[name]).abs().max()) <= 1e-12 * max(1.0, float(auto[name].abs().max())), name
    cls = ai.attn_class(N)
    assert [bool((cls == c).any()) for c in range(4)] == [N > c for c in range(4)]
    if N > 1:
        assert float(ai.planted_probability(inp, case).min()) >= 1 - 1e-6
    if N > 2:
        assert float(ref["lse"][:, :, cls == 2].max()) < -130
    if N > 3:
        assert float(ref["lse"][:, :, cls == 3].min()) > 130
    for shifted, flat in ai.attn_twins(N):
        assert int(cls[flat]) == 0 and int(cls[shifted]) in (2, 3)
        a, b = ref["out"][:, :, shifted], ref["out"][:, :, flat]
        assert float((a - b).abs().max()) <= 1e-10 * float(b.abs().max())
        d = (ref["lse"][:, :, shifted] - ref["lse"][:, :, flat]) / ai.LOG2E
        want = ai.ATTN_SHIFT if int(cls[shifted]) == 3 else -ai.ATTN_SHIFT
        assert float((d - want).abs().max()) < 1e-4              # shift / scale is rounded to fp32 once
    assert len(ai.attn_twins(N)) >= min(N // 8, 2)
    if M1 + M2 == 1:
        assert not bool(ref["dq"].any()) and not bool(ref["dk"].any())
    now, rec = ai.attn_restatement_distance(case), ai.ATTN_DISTANCE[case]
    assert set(now) == set(rec)
    for key in rec:
        a, b = ai.floor_distance(rec[key]), ai.floor_distance(now[key])
        assert a / 2 <= b <= a * 2, f"{case} {key}: recorded {rec[key]:.3e}, measured {now[key]:.3e}"


@pytest.mark.parametrize("case", ai.ATTN_CASES[1:], ids=ai.case_id)
def test_tolerances_reject_wrong_gradients(case):
    """What the tolerances of dk, dv and dq are worth, shown on the host with the fp64 reference, deliberately damaged, in the
    kernel's place: the Gaussian columns of dk zero; column 0 of dk zero; delta of the last query row taken as 0 (the row one
    past a tile, the workgroup or the resident cap where N is 33, 65, 257 or 513), which must show in dk - it is the dK/dV
    kernel that reads `dels` of that row - and in dq; the last query row left out of dk and dv.  The undamaged reference rounded
    to fp32 passes.  Printed for comparison: in how many key rows the tolerance of a dk group is no wider than ONE distance for
    the whole row times max |fp64| of the row makes it (the Gaussian columns: all, by a factor of 1e3 .. 1e4; the reserved ones:
    90 - 100 %, the others being rows in which column 0 cancels, where max |fp64| says little about the error fp32 makes)."""
    B, heads, N, M1, M2, dh = case
    M, R = M1 + M2, ai.reserved_features(case)
    inp = ai.attn_inputs(case)
    ref = ai.attn_ref(inp)

    def ratios(**changed):
        return ai.attn_ratios({**{n: ref[n].float() for n in ai.ATTN_QUANTITIES}, **changed}, ref, case)

    clean = ratios()
    assert max(clean.values()) <= 1.0, clean
    dk = ref["dk"].clone()
    dk[..., R:] = 0
    r = ratios(dk=dk)
    print(f"{ai.case_id(case)} Gaussian columns of dk zero: err / tol {r[('dk', 'features')]:.3g}")
    assert (r[("dk", "features")] > 1.0) == (M > 1) and r[("dk", "reserved")] <= 1.0         # dk of a one-key context is zero
    dk = ref["dk"].clone()
    dk[..., 0] = 0
    r = ratios(dk=dk)
    print(f"{ai.case_id(case)} column 0 of dk zero: err / tol {r[('dk', 'reserved')]:.3g}")
    assert (r[("dk", "reserved")] > 1.0) == (M > 1) and r[("dk", "features")] <= 1.0
    wrong = ai.attn_ref(inp, drop_delta_row=N - 1)
    r = ratios(dk=wrong["dk"], dq=wrong["dq"])
    cname = ai.ATTN_CLASSES[(N - 1) % 4]
    print(f"{ai.case_id(case)} delta of the last query row ({cname}) zero: err / tol dk features {r[('dk', 'features')]:.3g} "
          f"reserved {r[('dk', 'reserved')]:.3g}, dq {r[('dq', cname)]:.3g}")
    assert r[("dk", "features")] > 1.0 and r[("dq", cname)] > 1.0
    part = ai.attn_ref({**inp, **{n: inp[n][:, :, :N - 1] for n in ("q", "dout")}})
    r = ratios(dk=part["dk"], dv=part["dv"])
    print(f"{ai.case_id(case)} last query row left out: err / tol dk features {r[('dk', 'features')]:.3g}, dv {r[('dv', 'all')]:.3g}")
    seen = M > 1 and cname != "peaked"                   # dS of a peaked row is 1e-17: it adds nothing to dk
    assert (r[("dk", "features")] > 1.0) == seen and r[("dv", "all")] > 1.0
    if M > 1:
        whole = max(ai.row_error(ai.attn_ref(inp, torch.float32, o)["dk"], ref["dk"]).max() for o in ("tree", "chain"))
        old = ai.floor_distance(whole) * ref["dk"].abs().amax(-1, keepdim=True)
        for group, cols in (("reserved", slice(0, R)), ("features", slice(R, dh))):
            new = ai.floor_distance(ai.ATTN_DISTANCE[case][("dk", group)]) * ref["dk_terms"][..., cols].amax(-1, keepdim=True)
            frac = float((new <= old).double().mean())
            assert frac == 1.0 or group == "reserved"
            print(f"{ai.case_id(case)} dk {group}: tolerance no wider than the whole-row one in {frac:.1%} of the key rows, "
                  f"median ratio {float((new / old).median()):.3g}")


@pytest.mark.parametrize("case", [ai.ATTN_CASES[i] for i in (1, 2, 3, 9, 10)], ids=ai.case_id)
def test_layouts_hold_the_tensors(case):
    """place() puts every tensor at the columns layout_columns names, NaN elsewhere; offsets and widths are multiples of four
    floats and wide enough; to_heads undoes to_mem."""
    B, heads, N, M1, M2, dh = case
    inner = heads * dh
    inp = ai.attn_inputs(case)
    cols = ai.layout_columns(case)
    for _buf, width, col in cols.values():
        assert width % 4 == 0 and col % 4 == 0 and col + inner <= width
    q, k, v = (ai.to_mem(inp[n]) for n in ("q", "k", "v"))
    assert torch.equal(ai.to_heads(q, heads), inp["q"])
    bufs = ai.place([(q, cols["q"])], N, B)
    bufs.update(ai.place([(k, cols["k"]), (v, cols["v"])], M1 + M2, B))
    total = 0
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        buf, _width, col = cols[name]
        assert torch.equal(bufs[buf][:, :, col:col + inner], t)
        total += t.numel()
    assert sum(int((~torch.isnan(b)).sum()) for b in bufs.values()) == total
    if ai.attn_layout(case) == "wide":
        assert cols["q"][1] == 3 * inner + 4 and cols["k"][1] == 2 * inner + 8 and cols["dk"][1] == 2 * inner + 12
    if ai.attn_layout(case) == "separate":
        assert len({cols[n][0] for n in ("k", "v", "dk", "dv")}) == 4 and cols["dk"][1] == inner


def test_attention_entries_refuse_before_any_launch():
    """dim_head 24, a row stride below heads x dh, a stride that is no multiple of 4, a _cat entry without a second part, and
    a q, out or dout that is not 16-byte aligned (every kernel reads them with 16-byte loads): each entry answers with its
    error code and text.  No launch happens, so the pointers only have to be non-NULL."""
    from transmf_ad_amd import _lib
    lib = _lib.load()
    p = 4096
    B, heads, N, M, dh = 1, 2, 8, 8, 16
    inner = heads * dh
    SHAPE, ALIGN = -2, -3

    def fwd(q=p, dh=dh, qs=inner, kvs=2 * inner):
        return lib.tmf_xattn_fwd(q, p, p, p, p, B, heads, N, M, dh, qs, kvs, 0.25, None)

    def fwd_cat(q=p, dh=dh, qs=inner, kvs=2 * inner, M2=4):
        return lib.tmf_xattn_fwd_cat(q, p, p, p, p, p, p, B, heads, N, M - 4, M2, dh, qs, kvs, 0.25, None)

    def bwd(q=p, out=p, dout=p, k=p, dh=dh, qs=inner, kvs=2 * inner, dkvs=2 * inner):
        return lib.tmf_xattn_bwd(q, k, p, out, p, dout, p, p, p, B, heads, N, M, dh, qs, kvs, dkvs, 0.25, None)

    def bwd_cat(q=p, out=p, dout=p, k=p, dh=dh, qs=inner, kvs=2 * inner, dkvs=2 * inner, M2=4):
        return lib.tmf_xattn_bwd_cat(q, p, p, k, p, out, p, dout, p, p, p, p, p, B, heads, N, M - 4, M2, dh, qs, kvs, dkvs, 0.25,
                                     None)

    def refused(rc, code, *texts):
        msg = lib.tmf_last_error_string().decode()
        assert rc == code and all(t in msg for t in texts), (rc, msg)

    for name, fn in (("tmf_xattn_fwd", fwd), ("tmf_xattn_fwd_cat", fwd_cat), ("tmf_xattn_bwd", bwd), ("tmf_xattn_bwd_cat", bwd_cat)):
        refused(fn(dh=24), SHAPE, name + ":", "dim_head 24 not in {8,16,32,64}")
        refused(fn(qs=inner - 4), SHAPE, name + ":", "row stride smaller than heads*dh")
        refused(fn(kvs=inner - 4), SHAPE, name + ":", "row stride smaller than heads*dh")
        refused(fn(qs=inner + 2), SHAPE, name + ":", "row strides must be multiples of 4 floats")
        refused(fn(kvs=2 * inner + 6), SHAPE, name + ":", "row strides must be multiples of 4 floats")
        refused(fn(q=p + 4), ALIGN, name + ":", "'q' is not 16-byte aligned")
    for name, fn in (("tmf_xattn_fwd_cat", fwd_cat), ("tmf_xattn_bwd_cat", bwd_cat)):
        refused(fn(M2=0), SHAPE, name + ":", "context parts of 4 and 0 rows")
    for name, fn in (("tmf_xattn_bwd", bwd), ("tmf_xattn_bwd_cat", bwd_cat)):
        refused(fn(dout=p + 8), ALIGN, name + ":", "'dout' is not 16-byte aligned")
        refused(fn(out=p + 4), ALIGN, name + ":", "'out' is not 16-byte aligned")
        refused(fn(dkvs=inner - 4), SHAPE, name + ":", "dkv_stride must be a multiple of 4 and >= heads*dh")
        refused(fn(dkvs=2 * inner + 2), SHAPE, name + ":", "dkv_stride must be a multiple of 4 and >= heads*dh")
    refused(bwd(k=p + 4), ALIGN, "tmf_xattn_bwd:", "'k' is not 16-byte aligned")
    refused(bwd_cat(k=p + 4), ALIGN, "tmf_xattn_bwd_cat:", "'k2' is not 16-byte aligned")
    # the same calls with every argument in order pass the checks only on a machine with a GPU, so none is made here
