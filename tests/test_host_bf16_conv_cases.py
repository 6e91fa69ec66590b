"""The tables of tests/_bf16_conv_cases.py held to the library through the queries that need no GPU (kernel names,
tmf_conv3d_wgrad_bf16_plan, the workspace size), the walk model to itself, and every category of walk the weight-gradient rows
are there for to the rows: a planner change that moves a row to another kernel or plan, or that empties a category, fails
here.  Every query runs in a fresh child process, so that no option leaks into another test."""
import itertools
import json
import os
import subprocess
import sys

import torch

import _bf16_conv_cases as K
import _bn_inputs as bi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r"""
import ctypes, itertools, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.tmf_conv3d_fwd_bf16_kernel_name.restype = lib.tmf_conv3d_wgrad_bf16_kernel_name.restype = ctypes.c_char_p
lib.tmf_conv3d_wgrad_bf16_workspace_bytes.restype = ctypes.c_size_t
job = json.loads(sys.argv[2])
def opt(name, v):
    assert lib.tmf_set_option(name, v) == 0, (name, v)
def plan(shape, io):
    ns, tps = ctypes.c_int(-1), ctypes.c_int(-1)
    n = lib.tmf_conv3d_wgrad_bf16_plan(*shape, io, ctypes.byref(ns), ctypes.byref(tps))
    return [n, ns.value, tps.value]
out = dict(wgrad=[], fwd=[], bad=[], sweep_fwd={}, sweep_wgrad={})
for tr, io, shape in job["wgrad"]:
    opt(b"wgrad_tr", tr)
    out["wgrad"].append(dict(name=lib.tmf_conv3d_wgrad_bf16_kernel_name(*shape, io).decode(), plan=plan(shape, io),
                             plans=[plan(shape, 0), plan(shape, 1)], bytes=lib.tmf_conv3d_wgrad_bf16_workspace_bytes(*shape)))
opt(b"wgrad_tr", 1)
for v2, dma, io, (B, D, H, W, cin, cout) in job["fwd"]:
    opt(b"bf16_v2", v2)
    opt(b"bf16_dma", dma)
    out["fwd"].append([lib.tmf_conv3d_fwd_bf16_kernel_name(B, D, H, W, cin, cout, io).decode(),
                       lib.tmf_conv3d_fwd_bf16_kernel_name(B, D, H, W, cout, cin, io).decode()])
ns, tps = ctypes.c_int(-1), ctypes.c_int(-1)
for args in ([0, 8, 8, 8, 8, 8, 0], [1, 8, 8, 8, 8, 0, 1], [1, 8, 8, 8, 8, 8, 2]):
    out["bad"].append([lib.tmf_conv3d_wgrad_bf16_plan(*args, ctypes.byref(ns), ctypes.byref(tps)), ns.value, tps.value])
out["bad"].append([lib.tmf_conv3d_wgrad_bf16_plan(1, 8, 8, 8, 8, 8, 0, None, ctypes.byref(tps)), ns.value, tps.value])
s = job["sweep"]
if s:
    shapes = list(itertools.product(s["B"], s["volumes"], s["cin"], s["cout"]))
    for v2, dma in itertools.product((0, 1, 2), (0, 1)):
        opt(b"bf16_v2", v2)
        opt(b"bf16_dma", dma)
        for (B, (D, H, W), cin, cout), io in itertools.product(shapes, range(4)):
            for a, b in ((cin, cout), (cout, cin)):                    # forward, and the data gradient's swapped channels
                out["sweep_fwd"].setdefault(lib.tmf_conv3d_fwd_bf16_kernel_name(B, D, H, W, a, b, io).decode(), [v2, dma, io, B, D, H, W, a, b])
    for tr in (0, 1, 2):
        opt(b"wgrad_tr", tr)
        for (B, (D, H, W), cin, cout), io in itertools.product(shapes, range(2)):
            out["sweep_wgrad"].setdefault(lib.tmf_conv3d_wgrad_bf16_kernel_name(B, D, H, W, cin, cout, io).decode(), [tr, io, B, D, H, W, cin, cout])
print(json.dumps(out))
"""

_SWEEP = dict(B=K.SWEEP_B, volumes=K.SWEEP_VOLUMES, cin=K.SWEEP_CIN, cout=K.SWEEP_COUT)


def _probe(wgrad=(), fwd=(), sweep=None):
    from transmf_ad_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtmf_hip.so not built (python -m transmf_ad_amd.build)"
    e = {k: v for k, v in os.environ.items() if not k.startswith("TMF_")}
    job = dict(wgrad=[[r[0], r[1], list(r[2])] for r in wgrad], fwd=[[r[0], r[1], r[2], list(r[3])] for r in fwd], sweep=sweep)
    r = subprocess.run([sys.executable, "-c", _PROBE, _lib.LIB_PATH, json.dumps(job)], env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_every_weight_gradient_row_names_the_kernel_and_plan_the_library_selects():
    got = _probe(wgrad=K.WGRAD_ROWS)
    for row, g in zip(K.WGRAD_ROWS, got["wgrad"]):
        _tr, _io, shape, kernel, nsplit, tps, order = row
        cin, cout = shape[4:]
        assert g["name"] == kernel, K.wgrad_row_id(row)
        assert g["plan"] == [K.ntiles(shape), nsplit, tps], K.wgrad_row_id(row)
        assert order == K.order_of(kernel, nsplit), K.wgrad_row_id(row)
        assert g["bytes"] == max((ns + K.reduce_groups(ns)) * 27 * cin * cout * 4 for _n, ns, _t in g["plans"]), K.wgrad_row_id(row)
    ids = [K.wgrad_row_id(r) for r in K.WGRAD_ROWS]
    assert len(set(ids)) == len(ids)
    # bad arguments: 0, and nothing is written
    assert got["bad"] == [[0, -1, -1]] * 4


def test_every_forward_row_names_the_kernel_the_library_selects():
    got = _probe(fwd=K.FWD_ROWS)
    for row, (fwd, dgrad) in zip(K.FWD_ROWS, got["fwd"]):
        _v2, _dma, io, shape, name = row
        assert fwd == name, K.fwd_row_id(row)
        # the data gradient runs the same brick and tensor types, with the tile count of ITS output channels
        assert dgrad in K.expected_fwd_names() and K.fwd_brick(dgrad) == K.fwd_brick(name), K.fwd_row_id(row)
        bD, bH, bW = K.fwd_brick(name)
        assert shape[1] % bD and shape[2] % bH and shape[3] % bW or _v2 == 1, K.fwd_row_id(row)
        assert shape[4] % (16 if bD == 8 else 32) != 0
    ids = [K.fwd_row_id(r) for r in K.FWD_ROWS]
    assert len(set(ids)) == len(ids)
    assert len(K.expected_fwd_names()) == K.N_FWD_NAMES and {r[4] for r in K.FWD_ROWS} == K.expected_fwd_names()
    # the permuted-channel epilogue of the 8x8x8 brick (two tiles, bf16 output) on a partial last tile
    assert {r[3][5] for r in K.FWD_ROWS if "_v2_kernel<2" in r[4] and r[2] & 2} >= {72, 130}
    # the default choice, either side of its threshold
    assert [("_v2_" in r[4]) for r in K.FWD_ROWS if r[0] == 1] == [True, False]


def test_the_walks_partition_the_bricks_and_the_stepping_agrees_with_division():
    for row in K.WGRAD_ROWS:
        shape, nsplit, tps, order = row[2], row[4], row[5], row[6]
        ws = K.walks(row)
        assert sorted(b for w in ws for b in w) == list(range(K.ntiles(shape))), K.wgrad_row_id(row)
        for s, w in enumerate(ws):
            begin, step, _end = K.walk(order, K.ntiles(shape), nsplit, tps, s)
            assert K.stepped_coordinates(shape, begin, step, len(w)) == [K.divided_coordinates(shape, b) for b in w], (K.wgrad_row_id(row), s)
    # the model itself: a hand-checked interleaved walk (63 bricks, 16 workgroups: XCD 7 holds bricks 56 .. 62)
    row = next(r for r in K.WGRAD_ROWS if r[2] == K.S63 and r[1] == 0)
    assert K.walks(row)[7] == [56, 58, 60, 62] and K.walks(row)[15] == [57, 59, 61] and K.walks(row)[8] == [1, 3, 5, 7]


def test_every_category_of_walk_is_reached():
    rows = K.WGRAD_ROWS
    by = lambda kernel: [r for r in rows if r[3] == kernel]
    assert {r[3] for r in rows} == set(K.WGRAD_NAMES) and len(K.WGRAD_NAMES) == 5
    for kernel in K.WGRAD_NAMES:
        # the steady state of the pipeline: three or more bricks in some workgroup
        assert any(K.bricks_per_workgroup(r)[1] >= 3 for r in by(kernel)), kernel
        # two or more bricks of a volume that overhangs the brick on all three axes
        assert any(K.bricks_per_workgroup(r)[1] >= 2 and all(K.overhangs(r[2])) for r in by(kernel)), kernel
    for kernels in ([K.W_REG32], [K.W_REG16], K.TR_NAMES):
        mine = [r for r in rows if r[3] in kernels]
        assert any(K.last_split_shorter(r) for r in mine), kernels
        assert any(K.crosses_sample(r) and K.bricks_per_workgroup(r)[1] >= 2 for r in mine), kernels
    # ... in the bf16-tensor form of the transposing-read kernel too: the buffer resource moves to the next sample
    assert any(K.crosses_sample(r) for r in by(K.W_TR2_16))
    tr = [r for r in rows if r[3] in K.TR_NAMES]
    inter = [r for r in tr if r[6] == "interleaved"]
    assert any(K.step_of(r) == 1 and K.bricks_per_workgroup(r)[1] >= 3 for r in inter)
    assert any(K.step_of(r) >= 2 and K.bricks_per_workgroup(r)[1] >= 3 for r in inter)
    assert any(K.last_xcd_clipped(r) and K.bricks_per_workgroup(r)[0] < K.bricks_per_workgroup(r)[1] for r in inter)
    # a step with carries: some walk steps past the end of a row of bricks
    assert any(K.step_of(r) >= 2 and K.tiles(r[2])[2] % K.step_of(r) != 0 for r in inter)
    # partial last input and output channel blocks, over three or more bricks
    assert any(r[2][4] == 72 and r[2][5] == 136 and K.bricks_per_workgroup(r)[1] >= 3 for r in rows)
    # the rows for general operands: one per kernel, among the many-brick rows
    assert sorted(r[3] for r in K.WGRAD_GENERAL_ROWS) == sorted(K.WGRAD_NAMES)
    for r in K.WGRAD_GENERAL_ROWS:
        assert r in rows and K.bricks_per_workgroup(r)[1] >= 3 and r[2][0] * r[2][1] * r[2][2] * r[2][3] <= 27648
    # tensors and workspace stay small
    for r in rows:
        B, D, H, W, cin, cout = r[2]
        assert B * D * H * W * max(cin, cout) * 4 <= 40 << 20 and r[4] * 27 * cin * cout * 4 <= 64 << 20, K.wgrad_row_id(r)


def test_no_shape_or_option_selects_a_kernel_without_a_row():
    got = _probe(sweep=_SWEEP)
    stray = {n: w for n, w in got["sweep_fwd"].items() if n not in {r[4] for r in K.FWD_ROWS}}
    assert not stray, "no row of tests/_bf16_conv_cases.py runs {}".format(stray)
    stray = {n: w for n, w in got["sweep_wgrad"].items() if n not in {r[3] for r in K.WGRAD_ROWS}}
    assert not stray, "no row of tests/_bf16_conv_cases.py runs {}".format(stray)
    # the sweep is broad enough to mean something: it finds every name itself
    assert set(got["sweep_fwd"]) == K.expected_fwd_names() and set(got["sweep_wgrad"]) == set(K.WGRAD_NAMES)


def test_the_fast_references_equal_fp64_autograd():
    """27 matrix products against conv3d autograd in fp64 on a small integer case: bit for bit, both layouts, and the forward
    and data-gradient forms."""
    shape, cin, cout = (2, 5, 7, 9), 6, 10
    x, dz = bi.wgrad_inputs(shape, cin, cout)
    ref = bi.wgrad_ref(x, dz, 3)
    dw = K.wgrad_ref27(x, dz)
    assert torch.equal(dw, bi.tap_major(ref)) and torch.equal(K.reference_layout(dw), ref)
    w = torch.randint(-1, 2, (cout, cin, 3, 3, 3), generator=torch.Generator().manual_seed(3)).double()
    xr = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    z = torch.nn.functional.conv3d(xr, w, padding=1)
    z.backward(dz.double().permute(0, 4, 1, 2, 3))
    assert torch.equal(K.conv_ref27(x, K.fwd_taps(w)), z.detach().permute(0, 2, 3, 4, 1))
    assert torch.equal(K.conv_ref27(dz, K.dgrad_taps(w)), xr.grad.permute(0, 2, 3, 4, 1))


def test_the_forward_inputs_keep_the_statistics_exact():
    """The builder's own condition on the smallest and on a thinned case (the big threshold rows are built on the GPU run)."""
    for shape in (K.FWD_ROWS[0][3], K.FWD_ROWS[-1][3]):
        c = K.fwd_case(shape)
        assert float(c["z"].abs().sum((0, 1, 2, 3)).max()) < K.EXACT and float(c["s2"].max()) < K.EXACT
        assert c["x"].abs().max() <= 2 and c["w"].abs().max() <= 1 and torch.equal(c["z"], c["z"].round())
        assert (c["z"] != 0).float().mean() > 0.5            # thinning leaves a result that still tells bricks apart
