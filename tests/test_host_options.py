"""The library's process options (tmf_set_option and the TMF_* environment, include/tmf_hip.h) pinned through the queries that
see them without a GPU: the mode queries, tmf_snet_algo_flags, the kernel names and the size queries.  Every case runs in a
fresh child process, so that the environment is read anew and no option leaks into another test.

Three settings reach no query and are not checked here: "debug" (bits passed to the kernels as an argument), TMF_C1_FWD_MULT
(the workgroup count of the first block's forward launch) and TMF_WINO_EVEN (the grid of a persistent Winograd launch)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -5

# (B, D, H, W, cin, cout, ksize) of tmf_conv3d_fwd_kernel_name: the pooled volumes (conv_rt 1), 48^3 (conv_rt 2, conv_waves),
# the reference's 22x27x22 and 11x13x11 levels (the half brick and the 64-channel workgroups of TMF_CONV_AUTO), a 1x1x1 layer
FWD = [(8, 24, 24, 24, 64, 128, 3), (8, 48, 48, 48, 32, 64, 3), (8, 22, 27, 22, 64, 128, 3), (8, 11, 13, 11, 128, 256, 3),
       (8, 48, 48, 48, 32, 32, 1)]
WGRAD = [(8, 48, 48, 48, 32, 64, 3), (8, 12, 12, 12, 16, 32, 3), (8, 24, 24, 24, 128, 128, 3)]
# (B, D, H, W, cin, cout, io) of the bf16 kernel names: 8x8x8 bricks by count (bf16_v2 1), fp32 and bf16 tensors (bf16_dma),
# a small volume on the 4x8x8-brick kernel with 64 and 32 output channels (TMF_BF_NT2)
BF16_FWD = [(8, 48, 48, 48, 64, 64, 1), (8, 48, 48, 48, 64, 64, 0), (1, 16, 16, 16, 64, 64, 1), (1, 16, 16, 16, 64, 32, 0)]
BF16_WGRAD = [(8, 24, 24, 24, 32, 64, 0), (8, 24, 24, 24, 64, 64, 0), (8, 24, 24, 24, 32, 64, 1), (8, 24, 24, 24, 32, 32, 1)]

_PROBE = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
for f in ("tmf_last_error_string", "tmf_conv3d_fwd_kernel_name", "tmf_conv3d_wgrad_kernel_name",
          "tmf_conv3d_fwd_bf16_kernel_name", "tmf_conv3d_wgrad_bf16_kernel_name"):
    getattr(lib, f).restype = ctypes.c_char_p
lib.tmf_c1_gram_bytes.restype = lib.tmf_c1_gram_bytes_bf16.restype = ctypes.c_size_t
shapes = json.loads(sys.argv[2])
def names(f, key):
    return [getattr(lib, f)(*s).decode() for s in shapes[key]]
def snapshot():
    return dict(conv_wino=lib.tmf_conv_wino_mode(), wino_p=lib.tmf_wino_p_mode(), wino_x=lib.tmf_wino_x_mode(),
                c1_split=lib.tmf_c1_split_mode(), algo=lib.tmf_snet_algo_flags(),
                c1_gram=[lib.tmf_c1_gram_bytes(8, 96, 96, 96, 32) > 0, lib.tmf_c1_gram_bytes_bf16(8, 96, 96, 96, 32) > 0],
                wino_rows=lib.tmf_conv3d_wino_stat_blocks(8, 48, 48, 48), wino_bricks=lib.tmf_conv3d_wino_bricks2(8, 12, 12, 12, 32, 32),
                winox_items=lib.tmf_conv3d_wino_bricks2(8, 22, 27, 22, 64, 128), c1_blocks=lib.tmf_c1_blocks(8, 96, 96, 96, 32),
                fwd=names("tmf_conv3d_fwd_kernel_name", "fwd"), wgrad=names("tmf_conv3d_wgrad_kernel_name", "wgrad"),
                bf16_fwd=names("tmf_conv3d_fwd_bf16_kernel_name", "bf16_fwd"),
                bf16_wgrad=names("tmf_conv3d_wgrad_bf16_kernel_name", "bf16_wgrad"))
out = []
for step in json.loads(sys.argv[3]):
    if step is None:
        out.append(snapshot())
    else:
        rc = lib.tmf_set_option(step[0].encode() if step[0] is not None else None, step[1])
        out.append([rc, lib.tmf_last_error_string().decode() if rc else ""])
print(json.dumps(out))
"""


def _run(steps, env=None):
    """Runs `steps` in a fresh process whose TMF_* environment is exactly `env`: a step None records the queries' snapshot, a
    step (name, value) calls tmf_set_option and records [return code, error text or ""]."""
    from transmf_ad_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtmf_hip.so not built (python -m transmf_ad_amd.build)"
    e = {k: v for k, v in os.environ.items() if not k.startswith("TMF_")}
    e.update(env or {})
    shapes = dict(fwd=FWD, wgrad=WGRAD, bf16_fwd=BF16_FWD, bf16_wgrad=BF16_WGRAD)
    r = subprocess.run([sys.executable, "-c", _PROBE, _lib.LIB_PATH, json.dumps(shapes), json.dumps(steps)], env=e, cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _snap(env=None, *sets):
    """The snapshot after the given tmf_set_option calls (each must succeed)."""
    out = _run([list(s) for s in sets] + [None], env)
    assert all(rc == [0, ""] for rc in out[:-1]), out[:-1]
    return out[-1]


ALGO, P, X, G, G16, S = 0x100, 0x800, 0x1000, 0x2000, 0x4000, 0x8000
FWD_DEFAULT = ["FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>",
               "FwdCfg<3, 32, 1, 1, 2, 2, 4, 4, 4, 1>", "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>"]
DEFAULT = dict(
    conv_wino=3, wino_p=1, wino_x=1, c1_split=1, algo=ALGO | (3 << 9) | P | X | G | S, c1_gram=[True, False],
    wino_bricks=2 * 3 * 3 * 3, winox_items=8 * 63, c1_blocks=1024, fwd=FWD_DEFAULT,
    wgrad=["WgCfg<1, 4, 8, 8, 8, 32>", "WgCfg<1, 4, 4, 4, 8, 16>", "WgCfg<1, 4, 8, 8, 8, 32>"],
    bf16_fwd=["conv3d_fwd_bf16_v2_kernel<2, true, false, true>", "conv3d_fwd_bf16_v2_kernel<2, false, false, false>",
              "conv3d_fwd_bf16_kernel<2, true, false>", "conv3d_fwd_bf16_kernel<1, false, false>"],
    bf16_wgrad=["conv3d_wgrad_bf16_kernel<false>", "conv3d_wgrad_bf16_tr_kernel<1, false>", "conv3d_wgrad_bf16_tr_kernel<2, true>",
                "conv3d_wgrad_bf16_tr_kernel<1, true>"])
WAVES_WGRAD4 = ["WgCfg<2, 4, 8, 8, 4, 32>", "WgCfg<1, 4, 4, 4, 4, 32>", "WgCfg<2, 4, 8, 8, 4, 32>"]
# what each accepted tmf_set_option value changes against DEFAULT (everything else stays)
SET_EFFECTS = {
    ("conv_wino", 0): dict(conv_wino=0, algo=ALGO | P | X | G | S),
    ("conv_wino", 1): dict(conv_wino=1, algo=ALGO | (1 << 9) | P | X | G | S),
    ("conv_wino", 2): dict(conv_wino=2, algo=ALGO | (2 << 9) | P | X | G | S),
    ("conv_wino", 3): {},
    ("wino_p", 0): dict(wino_p=0, algo=ALGO | (3 << 9) | X | G | S, wino_rows=8 * 12 * 6 * 6, wino_bricks=8 * 3 * 2 * 2, winox_items=8 * 72),
    ("wino_p", 1): {},
    ("wino_x", 0): dict(wino_x=0, algo=ALGO | (3 << 9) | P | G | S),
    ("wino_x", 1): {},
    ("c1_gram", 0): dict(algo=ALGO | (3 << 9) | P | X | S, c1_gram=[False, False]),
    ("c1_gram", 1): {},
    ("c1_gram", 2): dict(algo=ALGO | (3 << 9) | P | X | G | G16 | S, c1_gram=[True, True]),
    ("c1_split", 0): dict(c1_split=0, algo=ALGO | (3 << 9) | P | X | G),
    ("c1_split", 1): {},
    ("wino_cus", 5): dict(wino_rows=5),
    ("wino_cus", 0): {},
    ("conv_rt", 0): {},
    ("conv_rt", 1): dict(fwd=["RtCfg<2>"] + FWD_DEFAULT[1:]),
    ("conv_rt", 2): dict(fwd=["RtCfg<2>", "RtCfg<2>"] + FWD_DEFAULT[2:]),
    ("conv_waves", 2): dict(fwd=["FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>"] * 3 + ["FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>",
                                                                                "FwdCfg<1, 32, 1, 1, 4, 1, 4, 4, 8, 1>"], wgrad=WAVES_WGRAD4),
    ("conv_waves", 4): dict(fwd=["FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>"] * 3 + ["FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>",
                                                                                "FwdCfg<1, 32, 2, 1, 4, 1, 4, 8, 8, 1>"], wgrad=WAVES_WGRAD4),
    ("conv_waves", 8): dict(fwd=["FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>"] * 3 + ["FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>",
                                                                                "FwdCfg<1, 32, 1, 1, 8, 1, 4, 8, 8, 1>"]),
    ("conv_waves", 16): {},
    ("bf16_v2", 0): dict(bf16_fwd=["conv3d_fwd_bf16_kernel<2, true, false>", "conv3d_fwd_bf16_kernel<2, false, false>",
                                   "conv3d_fwd_bf16_kernel<2, true, false>", "conv3d_fwd_bf16_kernel<1, false, false>"]),
    ("bf16_v2", 1): {},
    ("bf16_v2", 2): dict(bf16_fwd=["conv3d_fwd_bf16_v2_kernel<2, true, false, true>", "conv3d_fwd_bf16_v2_kernel<2, false, false, false>",
                                   "conv3d_fwd_bf16_v2_kernel<2, true, false, true>", "conv3d_fwd_bf16_v2_kernel<1, false, false, false>"]),
    ("bf16_dma", 0): dict(bf16_fwd=["conv3d_fwd_bf16_v2_kernel<2, true, false, false>"] + DEFAULT["bf16_fwd"][1:]),
    ("bf16_dma", 1): {},
    ("wgrad_tr", 0): dict(bf16_wgrad=["conv3d_wgrad_bf16_kernel<false>"] * 2 + ["conv3d_wgrad_bf16_kernel<true>"] * 2),
    ("wgrad_tr", 1): {},
    ("wgrad_tr", 2): dict(bf16_wgrad=["conv3d_wgrad_bf16_tr_kernel<1, false>"] * 2 + DEFAULT["bf16_wgrad"][2:]),
}


def _default_rows():
    return _snap()["wino_rows"]


def _expect(changes, rows):
    return {**DEFAULT, "wino_rows": rows, **changes}


def test_defaults_without_environment():
    snap = _snap()
    rows = snap["wino_rows"]                  # one statistic row per compute unit (256 without a device)
    assert 64 <= rows <= 1024
    assert snap == _expect({}, rows)


def test_set_option_accepted_values():
    """Every accepted value of every option, each in a process of its own; the values the setter folds onto another."""
    rows = _default_rows()
    for (name, value), changes in SET_EFFECTS.items():
        assert _snap(None, (name, value)) == _expect(changes, rows), (name, value)
    folded = {("wino_p", 5): ("wino_p", 1), ("wino_p", -2): ("wino_p", 1), ("wino_x", 7): ("wino_x", 1),
              ("c1_split", -1): ("c1_split", 1), ("c1_gram", -3): ("c1_gram", 0), ("c1_gram", 9): ("c1_gram", 2),
              ("wino_cus", 1 << 20): ("wino_cus", 0)}                      # (never above the device's count)
    for (name, value), same in folded.items():
        assert _snap(None, (name, value)) == _expect(SET_EFFECTS[same], rows), (name, value)
    # "debug" takes any value and changes no query; a later call replaces an earlier one
    assert _snap(None, ("debug", 12345), ("debug", -7)) == _expect({}, rows)
    assert _snap(None, ("conv_wino", 0), ("wino_p", 0), ("conv_wino", 3)) == _expect(SET_EFFECTS[("wino_p", 0)], rows)


def test_set_option_rejections_keep_the_value():
    steps = [["conv_rt", 1], ["conv_waves", 8], ["bf16_v2", 0], ["wgrad_tr", 0], ["bf16_dma", 0], ["wino_cus", 5], ["conv_wino", 1]]
    bad = [
        (["conv_wino", 4], "conv_wino must be 0, 1, 2 or 3, got 4"), (["conv_wino", -1], "conv_wino must be 0, 1, 2 or 3, got -1"),
        (["wino_cus", -1], "wino_cus must be >= 0, got -1"),
        (["conv_rt", 3], "conv_rt must be 0, 1 or 2, got 3"), (["conv_rt", -1], "conv_rt must be 0, 1 or 2, got -1"),
        (["conv_waves", 3], "conv_waves must be 2, 4, 8 or 16, got 3"), (["conv_waves", 32], "conv_waves must be 2, 4, 8 or 16, got 32"),
        (["conv_waves", 0], "conv_waves must be 2, 4, 8 or 16, got 0"),
        (["bf16_v2", 3], "bf16_v2 must be 0, 1 or 2, got 3"), (["bf16_v2", -1], "bf16_v2 must be 0, 1 or 2, got -1"),
        (["bf16_dma", 2], "bf16_dma must be 0 or 1, got 2"), (["bf16_dma", -1], "bf16_dma must be 0 or 1, got -1"),
        (["wgrad_tr", 3], "wgrad_tr must be 0, 1 or 2, got 3"), (["wgrad_tr", -1], "wgrad_tr must be 0, 1 or 2, got -1"),
        (["wino", 1], "unknown option 'wino'"), (["WINO_P", 0], "unknown option 'WINO_P'"), (["", 0], "unknown option ''"),
    ]
    out = _run(steps + [None] + [b for b, _ in bad] + [[None, 1], None])
    assert all(rc == [0, ""] for rc in out[:len(steps)])
    before, after = out[len(steps)], out[-1]
    assert before == after                                                # a rejected value changes nothing
    assert before["conv_wino"] == 1 and before["wino_rows"] == 5 and before["fwd"][0] == "RtCfg<2>"
    for (step, text), got in zip(bad, out[len(steps) + 1:]):
        assert got == [E_ARG, "tmf_set_option: " + text], step
    assert out[-2] == [-1, "tmf_set_option: argument 'name' is NULL"]    # TMF_E_NULL


# (environment, the tmf_set_option call it acts as; None: the default)
ENV_AS = [
    ({"TMF_CONV_WINO": "0"}, ("conv_wino", 0)), ({"TMF_CONV_WINO": "1"}, ("conv_wino", 1)), ({"TMF_CONV_WINO": "2"}, ("conv_wino", 2)),
    ({"TMF_CONV_WINO": "3"}, None), ({"TMF_CONV_WINO": "7"}, None), ({"TMF_CONV_WINO": "-1"}, None),
    ({"TMF_WINO_P": "0"}, ("wino_p", 0)), ({"TMF_WINO_P": "1"}, None), ({"TMF_WINO_P": "5"}, None),
    ({"TMF_WINO_X": "0"}, ("wino_x", 0)), ({"TMF_WINO_X": "-4"}, None),
    ({"TMF_C1_GRAM": "-3"}, ("c1_gram", 0)), ({"TMF_C1_GRAM": "0"}, ("c1_gram", 0)), ({"TMF_C1_GRAM": "1"}, None),
    ({"TMF_C1_GRAM": "2"}, ("c1_gram", 2)), ({"TMF_C1_GRAM": "9"}, ("c1_gram", 2)),
    ({"TMF_C1_SPLIT": "0"}, ("c1_split", 0)), ({"TMF_C1_SPLIT": "2"}, None),
    ({"TMF_WINO_CUS": "5"}, ("wino_cus", 5)), ({"TMF_WINO_CUS": "0"}, None), ({"TMF_WINO_CUS": "-3"}, None),
    ({"TMF_WINO_CUS": "1048576"}, None),
    ({"TMF_CONV_RT": "1"}, ("conv_rt", 1)), ({"TMF_CONV_RT": "2"}, ("conv_rt", 2)), ({"TMF_CONV_RT": "3"}, None),
    ({"TMF_CONV_RT": "-1"}, None),
    ({"TMF_CONV_WAVES": "2"}, ("conv_waves", 2)), ({"TMF_CONV_WAVES": "4"}, ("conv_waves", 4)),
    ({"TMF_CONV_WAVES": "8"}, ("conv_waves", 8)), ({"TMF_CONV_WAVES": "16"}, None), ({"TMF_CONV_WAVES": "3"}, None),
    ({"TMF_CONV_WAVES": "32"}, None),
    ({"TMF_BF_V2": "0"}, ("bf16_v2", 0)), ({"TMF_BF_V2": "2"}, ("bf16_v2", 2)), ({"TMF_BF_V2": "1"}, None),
    ({"TMF_BF_V2": "7"}, None), ({"TMF_BF_V2": "-1"}, None), ({"TMF_BF_V2": "garbage"}, ("bf16_v2", 0)),   # (atoi: 0)
    ({"TMF_BF_V2": "x2"}, ("bf16_v2", 0)),
]


def test_environment_acts_as_the_setter():
    rows = _default_rows()
    for env, same in ENV_AS:
        assert _snap(env) == _expect(SET_EFFECTS[same] if same else {}, rows), env


def test_environment_only_switches():
    rows = _default_rows()
    for off in ("0", "false"):                                              # (atoi: "false" is 0 as well)
        assert _snap({"TMF_WINOX_SWAP": off}) == _expect(dict(winox_items=8 * 72), rows)
        assert _snap({"TMF_BF_NT2": off}) == _expect(dict(bf16_fwd=DEFAULT["bf16_fwd"][:2] + ["conv3d_fwd_bf16_kernel<1, true, false>",
                                                                                             "conv3d_fwd_bf16_kernel<1, false, false>"]), rows)
        assert _snap({"TMF_CONV_AUTO": off}) == _expect(dict(fwd=FWD_DEFAULT[:2] + ["FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>",
                                                                                  "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", FWD_DEFAULT[4]]), rows)
    for on in ("1", "2", "-1"):
        assert _snap({"TMF_WINOX_SWAP": on, "TMF_BF_NT2": on, "TMF_CONV_AUTO": on, "TMF_WINO_EVEN": on}) == _expect({}, rows)
    # TMF_C1_BLOCKS: the slab workgroups of the first block's passes; below 64 the default
    assert _snap({"TMF_C1_BLOCKS": "100"}) == _expect(dict(c1_blocks=100), rows)
    assert _snap({"TMF_C1_BLOCKS": "64"}) == _expect(dict(c1_blocks=64), rows)
    assert _snap({"TMF_C1_BLOCKS": "63"}) == _expect({}, rows) and _snap({"TMF_C1_BLOCKS": "0"}) == _expect({}, rows)
    # (TMF_WINO_EVEN and TMF_C1_FWD_MULT shape launches only: set, they change no query)
    assert _snap({"TMF_WINO_EVEN": "0", "TMF_C1_FWD_MULT": "1"}) == _expect({}, rows)


def test_setter_wins_over_the_environment():
    rows = _default_rows()
    env = {"TMF_CONV_WINO": "1", "TMF_WINO_P": "0", "TMF_WINO_X": "0", "TMF_C1_GRAM": "0", "TMF_C1_SPLIT": "0", "TMF_CONV_RT": "2",
           "TMF_CONV_WAVES": "4", "TMF_BF_V2": "0", "TMF_WINO_CUS": "7"}
    sets = [("conv_wino", 3), ("wino_p", 1), ("wino_x", 1), ("c1_gram", 1), ("c1_split", 1), ("conv_rt", 0), ("conv_waves", 16),
            ("bf16_v2", 1), ("wino_cus", 5)]
    assert _snap(env, *sets) == _expect(dict(wino_rows=5), rows)
    # ... in either order of first use: the environment is read before or after the setter, the setter's value holds
    out = _run([None] + [list(s) for s in sets] + [None], env)
    assert out[0]["conv_wino"] == 1 and out[0]["wino_p"] == 0 and out[-1] == _expect(dict(wino_rows=5), rows)
    # wino_cus 0 returns to TMF_WINO_CUS, not to the device's count
    out = _run([None, ["wino_cus", 5], None, ["wino_cus", 0], None], {"TMF_WINO_CUS": "7"})
    assert [out[0]["wino_rows"], out[2]["wino_rows"], out[4]["wino_rows"]] == [7, 5, 7]
    assert _snap({"TMF_WINO_CUS": "7"}, ("wino_cus", 1 << 20))["wino_rows"] == rows
    assert _snap({"TMF_BF_V2": "garbage"}, ("bf16_v2", 1)) == _expect({}, rows)
