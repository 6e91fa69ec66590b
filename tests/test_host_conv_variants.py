"""The variant table of the direct fp32 convolution (tests/_conv_variants.py) held to the planners, and the planners to the
table, through the name queries that need no GPU: every row runs the kernels it says it runs, and no shape or option makes
plan_fwd / plan_wgrad select an instantiation that no row runs.  Every query runs in a fresh child process, so that the
environment is read anew and no option leaks into another test."""
import itertools
import json
import os
import subprocess
import sys

import _conv_variants as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_PROBE = r"""
import ctypes, itertools, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.tmf_conv3d_fwd_kernel_name.restype = lib.tmf_conv3d_wgrad_kernel_name.restype = ctypes.c_char_p
job = json.loads(sys.argv[2])
def opt(name, v):
    assert lib.tmf_set_option(name, v) == 0, (name, v)
out = dict(rows=[], fwd={}, wgrad={})
for cw, (B, D, H, W, cin, cout, k) in job["rows"]:
    opt(b"conv_waves", cw)
    out["rows"].append([lib.tmf_conv3d_fwd_kernel_name(B, D, H, W, cin, cout, k).decode(),
                        lib.tmf_conv3d_fwd_kernel_name(B, D, H, W, cout, cin, k).decode(),
                        lib.tmf_conv3d_wgrad_kernel_name(B, D, H, W, cin, cout, k).decode()])
s = job["sweep"]
for cw in s["waves"]:
    opt(b"conv_waves", cw)
    for rt in s["rt"]:
        opt(b"conv_rt", rt)
        for B, (D, H, W), cin, cout, k in itertools.product(s["B"], s["volumes"], s["cin"], s["cout"], s["k"]):
            where = [cw, rt, B, D, H, W, cin, cout, k]
            for a, b in ((cin, cout), (cout, cin)):                    # forward, and the data gradient's swapped channels
                out["fwd"].setdefault(lib.tmf_conv3d_fwd_kernel_name(B, D, H, W, a, b, k).decode(), where)
            if k == 3:
                out["wgrad"].setdefault(lib.tmf_conv3d_wgrad_kernel_name(B, D, H, W, cin, cout, k).decode(), where)
print(json.dumps(out))
"""

_SWEEP = dict(B=V.SWEEP_B, volumes=V.SWEEP_VOLUMES, cin=V.SWEEP_CIN, cout=V.SWEEP_COUT, k=V.SWEEP_K, waves=V.SWEEP_WAVES, rt=V.SWEEP_RT)
_NO_SWEEP = dict(_SWEEP, waves=())


def _probe(rows, sweep, env=None):
    """-> dict(rows = [forward, data-gradient, weight-gradient name] per row under its conv_waves; fwd / wgrad = {name: the
    first (conv_waves, conv_rt, B, D, H, W, cin, cout, k) of the sweep that selects it}), from a process whose TMF_* environment
    is exactly `env`."""
    from transmf_ad_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtmf_hip.so not built (python -m transmf_ad_amd.build)"
    e = {k: v for k, v in os.environ.items() if not k.startswith("TMF_")}
    e.update(env or {})
    job = dict(rows=[[r[0], list(r[1])] for r in rows], sweep=sweep)
    r = subprocess.run([sys.executable, "-c", _PROBE, _lib.LIB_PATH, json.dumps(job)], env=e, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_every_row_names_the_kernels_the_planners_select():
    got = _probe(V.ROWS, _NO_SWEEP)["rows"]
    for row, (fwd, dgrad, wgrad) in zip(V.ROWS, got):
        k = row[1][6]
        assert (fwd, dgrad) == (row[2], row[3]), V.row_id(row)
        assert (wgrad if k == 3 else None) == row[4], V.row_id(row)
        assert k == 3 or wgrad == "conv1x1_wgrad_kernel"
        assert V.fwd_params(fwd)["KS"] == k and V.fwd_params(dgrad)["KS"] == k
    ids = [V.row_id(r) for r in V.ROWS]
    assert len(set(ids)) == len(ids)


def test_the_table_reaches_every_instantiation():
    """33 FwdCfg and 8 WgCfg names: each is some row's forward kernel, not only a data gradient's."""
    assert len({r[2] for r in V.ROWS}) == V.N_FWD_NAMES
    assert V.expected_fwd_names() == {r[2] for r in V.ROWS}
    assert len(V.expected_wgrad_names()) == V.N_WGRAD_NAMES
    # ... in the vector-channel build, so that the fused epilogue (vector channels only) runs in each of them too
    assert {r[2] for r in V.ROWS if V.takes_fused(r)} == V.expected_fwd_names()
    # the scalar-channel builds: every brick geometry forward, every 4-wave weight gradient
    scalar = [r for r in V.ROWS if not V.is_vec(r[1][4], r[1][5])]
    assert {V.geometry(r[2]) for r in scalar} | {V.geometry(r[3]) for r in scalar} >= set(V.GEOMETRIES) - {"4x4x4 x64"}   # (S64: cout % 64 == 0)
    assert {r[4] for r in scalar if r[4]} == {n for n in V.expected_wgrad_names() if V.wgrad_params(n)["NW"] == 4}
    for r in scalar:
        assert r[4] is None or V.wgrad_params(r[4])["NW"] == 4, V.row_id(r)


def test_fused_rows_take_all_three_pooled_branches():
    fused = [r for r in V.ROWS if V.takes_fused(r)]
    assert {V.pool_branch(r[2]) for r in fused} == {"tw4", "mt2", "exchange"}
    for r in fused:
        cw, (B, D, H, W, cin, cout, k) = r[0], r[1]
        p = V.fwd_params(r[2])
        if (B, D, H, W) == V.VS:
            assert V.pool_branch(r[2]) == "tw4", V.row_id(r)
        elif cin <= 16 or cw == 4:
            assert V.pool_branch(r[2]) == "mt2", V.row_id(r)
        else:                                                    # the 8-wave bricks and the half bricks
            assert V.pool_branch(r[2]) == "exchange" and (p["WM"] == 8 or p["TH"] == 4), V.row_id(r)
    # each branch with one and with two N-tiles per wave, at k = 3 and at k = 1
    for branch in ("tw4", "mt2", "exchange"):
        seen = {(V.fwd_params(r[2])["NT"], r[1][6]) for r in fused if V.pool_branch(r[2]) == branch}
        assert seen == set(itertools.product((1, 2), (3, 1))), branch


def test_write_bounds_rows_sample_every_geometry():
    rows = V.guard_rows()
    assert {V.geometry(r[2]) for r in rows if V.is_vec(r[1][4], r[1][5])} == set(V.GEOMETRIES)
    assert {r[4] for r in rows} == V.expected_wgrad_names()
    assert len(rows) <= 16


def _closure(env):
    got = _probe([], _SWEEP, env)
    fwd = {n: w for n, w in got["fwd"].items() if not n.startswith("RtCfg")}       # (RT_SHAPES of tests/test_gpu_kernels.py)
    stray = {n: w for n, w in fwd.items() if n not in V.expected_fwd_names()}
    assert not stray, "no row of tests/_conv_variants.py runs {}".format(stray)
    stray = {n: w for n, w in got["wgrad"].items() if n not in V.expected_wgrad_names()}
    assert not stray, "no row of tests/_conv_variants.py runs {}".format(stray)
    return set(fwd), set(got["wgrad"]), set(got["fwd"]) - set(fwd)


def test_no_shape_or_option_selects_a_kernel_without_a_row():
    fwd, wgrad, rt = _closure(None)
    # the sweep is broad enough to mean something: it finds every name itself
    assert fwd == V.expected_fwd_names() and wgrad == V.expected_wgrad_names() and rt == {"RtCfg<1>", "RtCfg<2>"}


def test_no_kernel_without_a_row_with_the_brick_model_off():
    """TMF_CONV_AUTO=0 (environment only, read once): the 8-wave brick everywhere — fewer names, no new one."""
    fwd, wgrad, _ = _closure({"TMF_CONV_AUTO": "0"})
    assert "FwdCfg<3, 32, 1, 1, 2, 2, 4, 4, 4, 1>" not in fwd            # the 64-channel 4x4x4 workgroups are the model's pick
    assert wgrad == V.expected_wgrad_names()
