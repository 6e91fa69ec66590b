"""The direct fp32 convolution's kernel variants (transmf_ad_amd/csrc/conv3d_mfma.hip) as a table of launches that reach each of
them (tests/test_host_conv_variants.py, tests/test_gpu_conv_variants.py).

plan_fwd picks among 33 FwdCfg<KS, CINC, MT, NT, WM, WN, TD, TH, TW, TPS> instantiations (and two RtCfg, which RT_SHAPES of
tests/test_gpu_kernels.py cover), plan_wgrad among eight WgCfg<NT, TD, TH, TW, NW, CI>; the pick depends on the shape and on
the option conv_waves.  Every row below names the kernels it must run; the host test holds the table to the planners (and
the planners to the table: a name no row expects fails there), the GPU test runs each row against fp64.

Plain data and helpers; nothing here touches a GPU or the library."""
import re

# Volumes (B, D, H, W), ragged on all three axes against every brick (4x8x8, 4x4x8, 4x4x4), odd sizes so that floor-mode
# pooling drops a plane and a column:
VL = (2, 17, 18, 19)           # >= 4096 voxels: the 4x8x8 and 4x4x8 bricks (135 / 225 bricks)
VL4 = (4, 17, 18, 19)          # the same with twice the bricks: past the 128 full-brick workgroups below which the half brick wins
VS = (2, 9, 10, 11)            # the 4x4x4 bricks
# cin 40 and 12 leave a partial last input chunk (32 + 8, 8 + 4); cout 72, 136 and 24 a partial output tile; 38, 6 and 10
# are no multiples of 4: the scalar-channel (VEC = false) builds.

# (conv_waves, (B, D, H, W, cin, cout, k), forward kernel, data-gradient kernel (the forward query with cin and cout swapped),
#  weight-gradient kernel (None for k = 1: conv1x1_wgrad_kernel has no variants))
ROWS = [
    # conv_waves 16 (the default): 8-wave bricks with 16-channel chunks, the half brick, MT = 2 at cin <= 16, 4x4x4 bricks
    (16, VL + (40, 72, 3), "FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (16, VL + (40, 72, 1), "FwdCfg<1, 16, 1, 2, 8, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 2, 8, 1, 4, 8, 8, 1>", None),
    (16, VL4 + (40, 24, 3), "FwdCfg<3, 16, 1, 1, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (16, VL4 + (40, 24, 1), "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 2, 8, 1, 4, 8, 8, 1>", None),
    (16, VL + (40, 24, 3), "FwdCfg<3, 32, 1, 1, 4, 1, 4, 4, 8, 3>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (16, VL + (40, 136, 3), "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (16, VL + (12, 24, 3), "FwdCfg<3, 16, 2, 1, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 1, 4, 1, 4, 4, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 16>"),
    (16, VL + (12, 24, 1), "FwdCfg<1, 16, 2, 1, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>", None),
    (16, VL + (12, 72, 3), "FwdCfg<3, 16, 2, 2, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 1, 4, 1, 4, 4, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 16>"),
    (16, VL + (12, 72, 1), "FwdCfg<1, 16, 2, 2, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>", None),
    (16, VL + (8, 24, 3), "FwdCfg<3, 8, 2, 1, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 1, 4, 1, 4, 4, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 16>"),
    (16, VL + (8, 24, 1), "FwdCfg<1, 8, 2, 1, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>", None),
    (16, VL + (8, 72, 3), "FwdCfg<3, 8, 2, 2, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 1, 4, 1, 4, 4, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 16>"),
    (16, VL + (8, 72, 1), "FwdCfg<1, 8, 2, 2, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 1, 1, 8, 1, 4, 8, 8, 1>", None),
    (16, VS + (40, 72, 3), "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 8, 32>"),
    (16, VS + (40, 72, 1), "FwdCfg<1, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "FwdCfg<1, 32, 1, 1, 2, 4, 4, 4, 4, 1>", None),
    (16, VS + (40, 192, 3), "FwdCfg<3, 32, 1, 1, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 8, 32>"),
    (16, VS + (12, 72, 3), "FwdCfg<3, 16, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 8, 16>"),
    (16, VS + (12, 72, 1), "FwdCfg<1, 16, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<1, 32, 1, 1, 2, 4, 4, 4, 4, 1>", None),
    (16, VS + (8, 72, 3), "FwdCfg<3, 8, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 8, 16>"),
    (16, VS + (8, 72, 1), "FwdCfg<1, 8, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<1, 32, 1, 1, 2, 4, 4, 4, 4, 1>", None),
    # conv_waves 8: the 8-wave bricks with 32-channel chunks
    (8, VL + (40, 24, 3), "FwdCfg<3, 32, 1, 1, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (8, VL + (40, 24, 1), "FwdCfg<1, 32, 1, 1, 8, 1, 4, 8, 8, 1>", "FwdCfg<1, 32, 1, 2, 8, 1, 4, 8, 8, 1>", None),
    (8, VL + (40, 72, 3), "FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>", "WgCfg<1, 4, 8, 8, 8, 32>"),
    (8, VL + (40, 72, 1), "FwdCfg<1, 32, 1, 2, 8, 1, 4, 8, 8, 1>", "FwdCfg<1, 32, 1, 2, 8, 1, 4, 8, 8, 1>", None),
    # conv_waves 4: the 4-wave MT = 2 bricks and S128 at 32-channel chunks, the 4-wave weight gradients
    (4, VL + (40, 24, 3), "FwdCfg<3, 32, 2, 1, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>", "WgCfg<1, 4, 8, 8, 4, 32>"),
    (4, VL + (40, 24, 1), "FwdCfg<1, 32, 2, 1, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 32, 2, 2, 4, 1, 4, 8, 8, 1>", None),
    (4, VL + (40, 72, 3), "FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>", "WgCfg<2, 4, 8, 8, 4, 32>"),
    (4, VL + (40, 72, 1), "FwdCfg<1, 32, 2, 2, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 32, 2, 2, 4, 1, 4, 8, 8, 1>", None),
    (4, VS + (40, 72, 3), "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "WgCfg<2, 4, 4, 4, 4, 32>"),
    (4, VS + (40, 72, 1), "FwdCfg<1, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<1, 32, 1, 2, 2, 2, 4, 4, 4, 1>", None),
    (4, VS + (40, 24, 3), "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 4, 32>"),
    # conv_waves 2: the 1x1x1 half bricks (k = 3 takes the half bricks of conv_waves 16)
    (2, VL + (40, 24, 1), "FwdCfg<1, 32, 1, 1, 4, 1, 4, 4, 8, 1>", "FwdCfg<1, 32, 1, 2, 4, 1, 4, 4, 8, 1>", None),
    (2, VL + (40, 72, 1), "FwdCfg<1, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "FwdCfg<1, 32, 1, 2, 4, 1, 4, 4, 8, 1>", None),
    # scalar-channel builds (VEC = false) of every brick geometry; the weight gradient then runs 4-wave at any conv_waves
    (16, VL + (38, 72, 3), "FwdCfg<3, 16, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "WgCfg<2, 4, 8, 8, 4, 32>"),
    (16, VS + (38, 72, 3), "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<2, 4, 4, 4, 4, 32>"),
    (8, VL + (38, 72, 3), "FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 1, 2, 8, 1, 4, 8, 8, 3>", "WgCfg<2, 4, 8, 8, 4, 32>"),
    (8, VS + (38, 72, 3), "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<2, 4, 4, 4, 4, 32>"),
    (4, VL + (38, 72, 3), "FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 32, 2, 2, 4, 1, 4, 8, 8, 3>", "WgCfg<2, 4, 8, 8, 4, 32>"),
    (4, VS + (38, 72, 3), "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 2, 2, 2, 4, 4, 4, 1>", "WgCfg<2, 4, 4, 4, 4, 32>"),
    (2, VL + (38, 72, 3), "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "FwdCfg<3, 32, 1, 2, 4, 1, 4, 4, 8, 1>", "WgCfg<2, 4, 8, 8, 4, 32>"),
    (2, VS + (38, 72, 3), "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "FwdCfg<3, 32, 1, 1, 2, 4, 4, 4, 4, 1>", "WgCfg<2, 4, 4, 4, 4, 32>"),
    (16, VL + (6, 10, 3), "FwdCfg<3, 8, 2, 1, 4, 1, 4, 8, 8, 3>", "FwdCfg<3, 16, 2, 1, 4, 1, 4, 8, 8, 3>", "WgCfg<1, 4, 8, 8, 4, 32>"),
    (16, VL + (6, 10, 1), "FwdCfg<1, 8, 2, 1, 4, 1, 4, 8, 8, 1>", "FwdCfg<1, 16, 2, 1, 4, 1, 4, 8, 8, 1>", None),
    (16, VS + (6, 10, 3), "FwdCfg<3, 8, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<3, 16, 1, 2, 2, 2, 4, 4, 4, 1>", "WgCfg<1, 4, 4, 4, 4, 32>"),
    (16, VS + (6, 10, 1), "FwdCfg<1, 8, 1, 2, 2, 2, 4, 4, 4, 1>", "FwdCfg<1, 16, 1, 2, 2, 2, 4, 4, 4, 1>", None),
]

N_FWD_NAMES, N_WGRAD_NAMES = 33, 8          # the instantiations plan_fwd / plan_wgrad can select (RtCfg aside)


def row_id(row):
    cw, (B, D, H, W, cin, cout, k) = row[0], row[1]
    return "w{}-{}x{}x{}x{}-{}to{}-k{}".format(cw, B, D, H, W, cin, cout, k)


def is_vec(cin, cout):
    """The vector-channel (VEC = true) build runs; otherwise the scalar-channel one."""
    return cin % 4 == 0 and cout % 4 == 0


def takes_fused(row):
    """tmf_conv3d_fwd_affine accepts the row (the FUSED build exists for vector channels only)."""
    cin, cout = row[1][4], row[1][5]
    return is_vec(cin, cout) and cin > 1


_FWD = re.compile(r"^FwdCfg<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>$")
_WG = re.compile(r"^WgCfg<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>$")


def fwd_params(name):
    """FwdCfg<...> -> dict of its template arguments."""
    m = _FWD.match(name)
    assert m, name
    return dict(zip(("KS", "CINC", "MT", "NT", "WM", "WN", "TD", "TH", "TW", "TPS"), map(int, m.groups())))


def wgrad_params(name):
    m = _WG.match(name)
    assert m, name
    return dict(zip(("NT", "TD", "TH", "TW", "NW", "CI"), map(int, m.groups())))


def pool_branch(name):
    """The branch of the fused epilogue's 2x2x2 reduction a FwdCfg takes: the two h rows of a window sit in one lane's registers
    of one M-tile ("tw4": 4x4x4 bricks), in one lane's two M-tiles ("mt2"), or in the neighbouring wave, exchanged through LDS
    ("exchange")."""
    p = fwd_params(name)
    return "tw4" if p["TW"] == 4 else ("mt2" if p["MT"] == 2 else "exchange")


def geometry(name):
    """The brick geometry of a FwdCfg, as the write-bounds test samples them."""
    p = fwd_params(name)
    if p["TW"] == 4:
        return "4x4x4 x{}".format(32 * p["NT"] * p["WN"])
    if p["TH"] == 4:
        return "4x4x8"
    return "4x8x8 MT=2" if p["MT"] == 2 else "4x8x8 8-wave"


GEOMETRIES = ("4x8x8 MT=2", "4x8x8 8-wave", "4x4x8", "4x4x4 x128", "4x4x4 x64")


def guard_rows():
    """The k = 3 rows of the write-bounds test: the first row of every (brick geometry, vector / scalar build) of the forward
    kernels and the first row of every weight-gradient kernel."""
    seen, out = set(), []
    for row in ROWS:
        cw, shape, fwd, dgrad, wg = row
        if shape[6] != 3:
            continue
        keys = {("fwd", geometry(fwd), is_vec(shape[4], shape[5])), ("wgrad", wg)}
        if not keys <= seen:
            seen |= keys
            out.append(row)
    return out


# The planner sweep of the closure test: every name it yields must be a name some row expects (or an RtCfg).
SWEEP_B = (1, 2, 3, 8)
SWEEP_VOLUMES = ((48, 48, 48), (24, 24, 24), (12, 12, 12), (22, 27, 22), (11, 13, 11)) + tuple(v[1:] for v in (VL, VL4, VS))
SWEEP_CIN = (6, 8, 12, 16, 32, 40, 64, 128, 256)
SWEEP_COUT = (8, 10, 16, 24, 32, 48, 64, 72, 128, 256)
SWEEP_K = (1, 3)
SWEEP_WAVES = (2, 4, 8, 16)
SWEEP_RT = (0, 1, 2)


def expected_fwd_names():
    return {r[2] for r in ROWS} | {r[3] for r in ROWS}


def expected_wgrad_names():
    return {r[4] for r in ROWS if r[4] is not None}
