"""The bf16 matrix-core convolution's kernels (transmf_ad_amd/csrc/conv3d_bf16.hip) as a table of launches that reach each of
them, and the weight-gradient kernels with MANY bricks per workgroup (tests/test_host_bf16_conv_cases.py,
tests/test_gpu_bf16_conv_cases.py).

plan_wgrad_bf16 gives a channel block 256 / (channel blocks) workgroups; each walks `tiles_per_split` 4x8x8 bricks.  The
register-transposing kernel conv3d_wgrad_bf16_kernel<IN16> walks a contiguous range and keeps the loads of brick n + 1 in
registers across the matrix loop of brick n; the transposing-read kernel conv3d_wgrad_bf16_tr_kernel<NH, IN16> double-buffers
bricks in LDS, advances the brick coordinates digit by digit, and walks interleaved inside an XCD's eighth of the bricks when
the workgroup count is a multiple of 8.  The rows below are chosen by what the WALK does (bricks per workgroup, a ragged last
range, steps with carries, a walk across two samples); the host test holds every row to the library's own plan and every
category to the rows, the GPU test runs each row in exact integer arithmetic.

The forward rows reach each of the 20 instantiations tmf_conv3d_fwd_bf16_t can launch in-process.

Plain data, a Python model of the two walks and exact references; nothing here touches a GPU or the library."""
import functools

import torch

TD, TH, TW = 4, 8, 8                     # the weight-gradient (and small forward) brick; the large forward brick is 8x8x8
REG, TR = "conv3d_wgrad_bf16_kernel<{}>", "conv3d_wgrad_bf16_tr_kernel<{}, {}>"
W_REG32, W_REG16 = REG.format("false"), REG.format("true")
W_TR1_32, W_TR1_16, W_TR2_16 = TR.format(1, "false"), TR.format(1, "true"), TR.format(2, "true")
WGRAD_NAMES = (W_REG32, W_REG16, W_TR1_32, W_TR1_16, W_TR2_16)
REG_NAMES, TR_NAMES = WGRAD_NAMES[:2], WGRAD_NAMES[2:]

# (B, D, H, W, cin, cout)
S27 = (1, 12, 24, 24, 128, 256)          # 27 bricks
S45, S45R = (1, 12, 24, 40, 128, 256), (1, 9, 23, 35, 128, 256)        # 45 bricks, whole and overhanging on every axis
S63, S63R = (1, 28, 24, 24, 128, 128), (1, 27, 23, 22, 128, 128)       # 63 bricks
S63W = (1, 28, 24, 24, 128, 256)
S54 = (3, 12, 16, 24, 128, 256)          # 18 bricks per sample: ranges of 7 (and of 4) cross from one sample into the next
S80 = (1, 20, 32, 32, 128, 32)
S80R, S96R = (1, 19, 31, 30, 256, 32), (1, 23, 31, 30, 256, 32)        # cout <= 32: the 32-channel bf16-tensor kernel
S45P = (1, 12, 24, 40, 72, 136)          # partial last input block (72 = 2 x 32 + 8) and output block (136 = 4 x 32 + 8)

# (wgrad_tr option, io (0 fp32 tensors, 1 bf16 tensors), shape, kernel, nsplit, tiles_per_split, order)
WGRAD_ROWS = [
    (0, 0, S27, W_REG32, 7, 4, "contiguous"),             # 4 4 4 4 4 4 3
    (0, 1, S27, W_REG16, 7, 4, "contiguous"),
    (1, 1, S27, W_TR2_16, 14, 2, "contiguous"),           # 2 x 13, 1
    (0, 0, S45R, W_REG32, 8, 6, "contiguous"),            # 6 x 7, 3
    (0, 1, S45R, W_REG16, 8, 6, "contiguous"),
    (1, 0, S45, W_TR1_32, 8, 6, "interleaved"),           # step 1; the last XCD's range is clipped to 3
    (1, 0, S45R, W_TR1_32, 8, 6, "interleaved"),
    (1, 1, S45, W_TR2_16, 15, 3, "contiguous"),
    (1, 1, S45R, W_TR2_16, 15, 3, "contiguous"),
    (1, 0, S63, W_TR1_32, 16, 4, "interleaved"),          # step 2: 4 4 per XCD, 4 3 in the last
    (1, 0, S63R, W_TR1_32, 16, 4, "interleaved"),
    (1, 1, S63, W_TR2_16, 32, 2, "interleaved"),          # step 4: 2 2 2 2 per XCD, 2 2 2 1 in the last
    (1, 1, S63R, W_TR2_16, 32, 2, "interleaved"),
    (1, 1, S63W, W_TR2_16, 16, 4, "interleaved"),         # step 2
    (0, 0, S54, W_REG32, 8, 7, "contiguous"),             # bricks 14 .. 20 and 35 .. 41 cross a sample boundary
    (0, 1, S54, W_REG16, 8, 7, "contiguous"),
    (1, 0, S54, W_TR1_32, 8, 7, "interleaved"),           # step 1, ranges of 7
    (1, 1, S54, W_TR2_16, 14, 4, "contiguous"),           # bricks 16 .. 19 cross: the buffer resource moves to the next sample
    (1, 1, S80, W_TR1_16, 40, 2, "interleaved"),          # step 5
    (1, 1, S80R, W_TR1_16, 27, 3, "contiguous"),          # 3 x 26, 2
    (1, 1, S96R, W_TR1_16, 32, 3, "interleaved"),         # step 4
    (0, 0, S45P, W_REG32, 15, 3, "contiguous"),
    (0, 1, S45P, W_REG16, 15, 3, "contiguous"),
]
# one many-brick row per kernel for general (standard-normal) operands
WGRAD_GENERAL_ROWS = [WGRAD_ROWS[i] for i in (0, 4, 6, 13, 20)]


def wgrad_row_id(r):
    return "tr{}-io{}-{}".format(r[0], r[1], "x".join(map(str, r[2])))


def tiles(shape):
    """(bricks along D, H, W) of a (B, D, H, W, ...)."""
    return -(-shape[1] // TD), -(-shape[2] // TH), -(-shape[3] // TW)


def ntiles(shape):
    tD, tH, tW = tiles(shape)
    return shape[0] * tD * tH * tW


def overhangs(shape):
    """Per axis: the volume is no whole number of bricks."""
    return shape[1] % TD != 0, shape[2] % TH != 0, shape[3] % TW != 0


def reduce_groups(nsplit):
    """tmf_reduce_groups: first-stage groups of the slab reduction."""
    return 1 if nsplit <= 64 else min(32, nsplit // 16)


def order_of(kernel, nsplit):
    """The kernels' own rule: only the transposing-read kernel interleaves, and only with a multiple of 8 workgroups."""
    return "interleaved" if kernel in TR_NAMES and nsplit % 8 == 0 else "contiguous"


def walk(order, n, nsplit, tps, s):
    """(first brick, step, end) of workgroup s, copied in meaning from the kernels."""
    if order == "contiguous":
        return s * tps, 1, min((s + 1) * tps, n)
    per_xcd, xcd = (n + 7) >> 3, s & 7
    return xcd * per_xcd + (s >> 3), nsplit >> 3, min((xcd + 1) * per_xcd, n)


def walks(row):
    """The brick list of every workgroup of a row."""
    _tr, _io, shape, _kernel, nsplit, tps, order = row
    return [list(range(*[walk(order, ntiles(shape), nsplit, tps, s)[i] for i in (0, 2, 1)])) for s in range(nsplit)]


def step_of(row):
    return walk(row[6], ntiles(row[2]), row[4], row[5], 0)[1]


def bricks_per_workgroup(row):
    n = [len(w) for w in walks(row)]
    return min(n), max(n)


def crosses_sample(row):
    """Some workgroup walks bricks of two samples."""
    tD, tH, tW = tiles(row[2])
    return any(len({b // (tD * tH * tW) for b in w}) > 1 for w in walks(row))


def last_split_shorter(row):
    n = [len(w) for w in walks(row)]
    return row[6] == "contiguous" and 0 < n[-1] < n[0] and len(set(n[:-1])) == 1


def last_xcd_clipped(row):
    return row[6] == "interleaved" and ntiles(row[2]) % 8 != 0


def stepped_coordinates(shape, begin, step, count):
    """The (b, d, h, w) brick coordinates origin_next() of the transposing-read kernel hands out: the cursor starts at
    `begin` and advances by the digits of `step` with carries, never dividing again."""
    tD, tH, tW = tiles(shape)

    def digits(t):
        return [t % tW, t // tW % tH, t // (tW * tH) % tD, t // (tW * tH * tD)]
    cw, ch, cd, cb = digits(begin)
    sw, sh, sd, sb = digits(step)
    out = []
    for _ in range(count):
        out.append((cb, cd, ch, cw))
        cw += sw
        if cw >= tW:
            cw -= tW
            ch += 1
        ch += sh
        if ch >= tH:
            ch -= tH
            cd += 1
        cd += sd
        if cd >= tD:
            cd -= tD
            cb += 1
        cb += sb
    return out


def divided_coordinates(shape, brick):
    tD, tH, tW = tiles(shape)
    return brick // (tW * tH * tD), brick // (tW * tH) % tD, brick // tW % tH, brick % tW


# ---------------------------------------------------------------------------------------------------------------------
# forward rows: (bf16_v2 option, bf16_dma option, io (bit 0: x is bf16, bit 1: z is bf16), (B, D, H, W, cin, cout), kernel)
# ---------------------------------------------------------------------------------------------------------------------
_tf = lambda b: "true" if b else "false"


def fwd_name(nt, io):
    return "conv3d_fwd_bf16_kernel<{}, {}, {}>".format(nt, _tf(io & 1), _tf(io & 2))


def fwd_v2_name(nt, io, dma):
    return "conv3d_fwd_bf16_v2_kernel<{}, {}, {}, {}>".format(nt, _tf(io & 1), _tf(io & 2), _tf(dma and io & 1))


def expected_fwd_names():
    small = {fwd_name(nt, io) for nt in (1, 2) for io in range(4)}
    large = {fwd_v2_name(nt, io, dma) for nt in (1, 2) for io in range(4) for dma in (0, 1)}
    return small | large


N_FWD_NAMES = 20                          # 8 + 12
VF = (2, 5, 9, 11)                        # overhangs the 4x8x8 brick on every axis
VF2 = (2, 9, 10, 11)                      # ... and the 8x8x8 brick
# cin 40: a partial last 32-channel chunk (small brick) and 16-channel chunk (8x8x8 brick); cin 24: 16 + 8.  cout 72 = 2 x 32 + 8
# and 130 = 4 x 32 + 2: a partial last tile (130 with a bf16 output: the permuted-channel epilogue on a tile of one channel
# pair); the small-brick NT = 2 kernel needs cout % 64 == 0 and has no partial tile.
FWD_ROWS = (
    [(0, 1, io, VF + (40, 72), fwd_name(1, io)) for io in range(4)]
    + [(0, 1, io, VF + (40, 64), fwd_name(2, io)) for io in range(3)] + [(0, 1, 3, (1, 6, 10, 9, 40, 128), fwd_name(2, 3))]
    + [(2, 1, 0, VF2 + (24, 24), fwd_v2_name(1, 0, 1)), (2, 1, 1, VF2 + (40, 24), fwd_v2_name(1, 1, 1)),
       (2, 0, 1, VF2 + (40, 24), fwd_v2_name(1, 1, 0)), (2, 1, 2, VF2 + (40, 24), fwd_v2_name(1, 2, 1)),
       (2, 1, 3, VF2 + (40, 24), fwd_v2_name(1, 3, 1)), (2, 0, 3, VF2 + (24, 32), fwd_v2_name(1, 3, 0))]
    + [(2, 1, 0, VF2 + (40, 72), fwd_v2_name(2, 0, 1)), (2, 1, 1, VF2 + (40, 72), fwd_v2_name(2, 1, 1)),
       (2, 0, 1, VF2 + (24, 72), fwd_v2_name(2, 1, 0)), (2, 1, 2, VF2 + (40, 130), fwd_v2_name(2, 2, 1)),
       (2, 1, 2, VF2 + (24, 72), fwd_v2_name(2, 2, 1)), (2, 1, 3, VF2 + (40, 72), fwd_v2_name(2, 3, 1)),
       (2, 1, 3, VF2 + (40, 130), fwd_v2_name(2, 3, 1)), (2, 0, 3, VF2 + (40, 130), fwd_v2_name(2, 3, 0))]
    # the default choice by the brick count, either side of its threshold of 384 8x8x8 bricks
    + [(1, 1, 0, (1, 48, 64, 64, 8, 16), fwd_v2_name(1, 0, 1)), (1, 1, 0, (1, 48, 64, 56, 8, 16), fwd_name(1, 0))]
)


def fwd_row_id(r):
    return "v{}-dma{}-io{}-{}".format(r[0], r[1], r[2], "x".join(map(str, r[3])))


def fwd_brick(name):
    return (8, 8, 8) if "_v2_" in name else (4, 8, 8)


# ---------------------------------------------------------------------------------------------------------------------
# the name sweep of the host test
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_B = (1, 2, 3, 8)
SWEEP_VOLUMES = ((4, 8, 8), (9, 10, 11), (24, 24, 24), (48, 64, 56), (48, 64, 64), (64, 64, 64))
SWEEP_CIN = (8, 16, 40, 64, 128)
SWEEP_COUT = (16, 24, 32, 64, 72, 128, 256)


# ---------------------------------------------------------------------------------------------------------------------
# exact references: 27 fp64 matrix products over the padded, shifted tensors (channels-last (B, D, H, W, C) throughout)
# ---------------------------------------------------------------------------------------------------------------------
def _shifted(xp, t, D, H, W):
    kd, kh, kw = t // 9, t // 3 % 3, t % 3
    return xp[:, kd:kd + D, kh:kh + H, kw:kw + W].reshape(-1, xp.shape[-1])


def _padded(x):
    return torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1, 1, 1))


def wgrad_ref27(x, dz):
    """fp64 dw[t][ci][co] = sum over voxels v of x[v + t - 1][ci] dz[v][co] (zero outside the volume): tap-major (27, cin, cout)."""
    _B, D, H, W, _cin = x.shape
    xp, d = _padded(x), dz.double().reshape(-1, dz.shape[-1])
    return torch.stack([_shifted(xp, t, D, H, W).t() @ d for t in range(27)])


def conv_ref27(x, wt):
    """fp64 z[v][co] = sum over t, ci of x[v + t - 1][ci] wt[t][ci][co]; wt (27, cin, cout) -> (B, D, H, W, cout)."""
    B, D, H, W, _cin = x.shape
    xp, wt = _padded(x), wt.double()
    z = torch.zeros((B * D * H * W, wt.shape[-1]), dtype=torch.float64)
    for t in range(27):
        z += _shifted(xp, t, D, H, W) @ wt[t]
    return z.view(B, D, H, W, -1)


def fwd_taps(w):
    """(cout, cin, 3, 3, 3) -> the forward convolution's wt[t][ci][co]."""
    return w.reshape(w.shape[0], w.shape[1], 27).permute(2, 1, 0)


def dgrad_taps(w):
    """... -> the data gradient's wt[t][co][ci] = w[co][ci][26 - t] (a convolution of dz with cout input channels)."""
    return w.reshape(w.shape[0], w.shape[1], 27).flip(2).permute(2, 0, 1)


def reference_layout(dw):
    """tap-major (27, cin, cout) -> nn.Conv3d's (cout, cin, 3, 3, 3)."""
    return dw.permute(2, 1, 0).reshape(dw.shape[2], dw.shape[1], 3, 3, 3).contiguous()


@functools.lru_cache(maxsize=None)
def wgrad_case(shape):
    """Integer x, dz in [-2, 2] (as _bn_inputs.wgrad_inputs) and the fp64 weight gradient, computed once per shape and shared,
    read only, by the io modes and options.  Every product is exact in bf16 x bf16 -> fp32 and every sum, in any order, an
    integer below 4 B D H W < 2^24."""
    B, D, H, W, cin, cout = shape
    assert 4 * B * D * H * W < 1 << 24
    g = torch.Generator().manual_seed(1000 * D + 100 * H + W + cin + cout)
    x = torch.randint(-2, 3, (B, D, H, W, cin), generator=g).float()
    dz = torch.randint(-2, 3, (B, D, H, W, cout), generator=g).float()
    dw = wgrad_ref27(x, dz)
    assert float(dw.abs().max()) < 1 << 24
    return dict(x=x, dz=dz, dw=dw.float(), dw_ref=reference_layout(dw).float())


@functools.lru_cache(maxsize=None)
def wgrad_general_case(shape):
    """Standard-normal x, dz and the fp64 weight gradient of their bf16 roundings."""
    B, D, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(7 + D + H + W + cin + cout)
    x = torch.randn((B, D, H, W, cin), generator=g)
    dz = torch.randn((B, D, H, W, cout), generator=g)
    return dict(x=x, dz=dz, dw=wgrad_ref27(x.bfloat16().float(), dz.bfloat16().float()))


EXACT = float(1 << 24)


@functools.lru_cache(maxsize=None)
def fwd_case(shape):
    """Integer x, dz in [-2, 2] and w in [-1, 1] of a forward row's shape with the exact z and (cout % 8 == 0) the exact input
    gradient.  x and w are thinned until, for every output channel, sum |z| and sum z^2 over the whole volume stay below
    2^24: then every partial sum of the kernels' statistics is an integer below 2^24 in any order - exact in fp32."""
    B, D, H, W, cin, cout = shape
    g = torch.Generator().manual_seed(31 * D + 7 * W + cin + 1000 * cout)
    x = torch.randint(-2, 3, (B, D, H, W, cin), generator=g).float()
    w = torch.randint(-1, 2, (cout, cin, 3, 3, 3), generator=g).float()
    dz = torch.randint(-2, 3, (B, D, H, W, cout), generator=g).float()
    for _ in range(12):
        z = conv_ref27(x, fwd_taps(w))
        s1, s2 = z.abs().sum((0, 1, 2, 3)), (z * z).sum((0, 1, 2, 3))
        if float(s1.max()) < EXACT and float(s2.max()) < EXACT:
            break
        w = w * (torch.rand(w.shape, generator=g) < 0.5)
        x = x * (torch.rand(x.shape, generator=g) < 0.7)
    assert float(s1.max()) < EXACT and float(s2.max()) < EXACT and float(z.abs().max()) > 0
    r = dict(x=x, w=w, dz=dz, z=z, s1=z.sum((0, 1, 2, 3)), s2=s2)
    if cout % 8 == 0:
        r["dx"] = conv_ref27(dz, dgrad_taps(w))
        assert float(r["dx"].abs().max()) < EXACT
    return r
