"""Cases, inputs and references of the fused transformer kernel tests (tests/test_host_xf.py, tests/test_gpu_xf.py): the three
one-call fusion entries tmf_fusion_train_fwd / _train_bwd / _infer_fwd at dim 128 - csrc/xformer_fused.hip behind them, or
one launch per op with TMF_FUSION_PER_OP.

The reference is the explicit formula of _fusion64 (tests/test_gpu_kernels.py) and its gradients on plain tensors, fp64; the
yardstick is the same formula in fp32 in two orders of every contraction (torch's own fp32 matmul / sum, and a chain that adds
one rounded product after the other).  The larger distance from fp64 is recorded per (case, heads, quantity, class) in
XF_DISTANCE; a row's tolerance is margin x floor_distance(recorded) x scale of the row.

What the judged quantities cannot see: the mean half of cls dilutes ONE token's forward error by 1 / N (at N = 512 a token
row that is wrong by 1e-3 of its scale moves the mean by 2e-6 of it, inside the tolerance).  The per-row checks of the token
gradients (a wrong forward row has a wrong P, a wrong GELU derivative and wrong LayerNorm statistics in ITS gradient row), the
(1, 1, 1) case, where cls IS the one token's output in both halves, and the deliberately wrong results of the host test are
what cover a single token's forward.

Nothing here touches a GPU or a file."""
import functools
import math

import numpy as np
import torch

from _attn_inputs import ATTN_CLASSES, ATTN_PEAK, ATTN_SHIFT
from _bn_inputs import U32, f32  # noqa: F401  (re-exported to the two test modules)
from _token_inputs import MARGIN, _sum_axis, floor_distance  # noqa: F401

DIM, MLP, EPS = 128, 512, 1e-5
LOG2E = 1.4426950408889634
XF_HEADS = ((4, 32), (8, 16))               # (heads, dim_head) of the two fused geometries

# (B, N, depth, masks) and what each reaches (N <= 128: guarded MT 8; 129..144, 161..208, 225..256: guarded MT 16;
# 145..160: exact MT 10; 209..224: exact MT 14; 257..496: guarded MT 32; 497..512: exact MT 32)
XF_CASES = [
    (1, 1, 1, False),        # one token: the softmax is over one key, P = 1 and dS = 0; cls is that token's output in both halves
    (3, 16, 1, False),       # one full tile with no padded row anywhere: the control
    (2, 17, 2, False),       # one valid row in the second tile; depth 2 reaches dctx_acc
    (2, 33, 1, True),        # three key tiles: the by-three loops of the backward with no overhang
    (9, 40, 1, False),       # second batch group of xf_who, seven dead workgroups per slot
    (17, 20, 1, True),       # three batch groups
    (1, 128, 1, False),      # last N of guarded MT 8
    (1, 129, 1, False),      # first N of guarded MT 16
    (1, 144, 1, False),      # last N below exact MT 10
    (1, 145, 1, False),      # first N of exact MT 10
    (1, 160, 1, True),       # last N of exact MT 10
    (1, 161, 1, False),      # first N above it
    (1, 208, 1, False),      # last N below exact MT 14
    (1, 209, 1, False),      # first N of exact MT 14
    (2, 216, 2, True),       # the workload's own shape
    (1, 225, 1, False),      # first N above exact MT 14 (224 + 1)
    (1, 256, 1, False),      # last N of guarded MT 16
    (1, 257, 1, False),      # first N of guarded MT 32
    (1, 496, 1, False),      # last N of guarded MT 32
    (1, 497, 1, False),      # first N of exact MT 32
    (1, 512, 1, True),       # the limit
]
# case -> seed other than 0: a case whose near-tie share exceeds TIE_CAP gets another seed, not another cap ((1, 225): 6.6 % of
# the columns at 8 heads with seed 0, 5.5 % at 4 heads with seed 1, 3.5 % at both with seed 2)
XF_SEED = {(1, 225, 1, False): 2}
XF_CLASSES = ATTN_CLASSES    # query row r of the layer-0 instances is of class r % 4: flat, peaked, low, high
TIE_GAP, TIE_CAP = 1e-3, 0.05
SMALL_SEGMENTS = (("b2", DIM), ("b1", MLP), ("bo", DIM), ("ln2_g", DIM), ("ln2_b", DIM), ("ln1_g", DIM), ("ln1_b", DIM))
LNF_SEGMENTS = (("lnf_g", DIM), ("lnf_b", DIM))
WEIGHTS = ("dwq", "dwkv", "dwo", "dw1", "dw2")
PARAM_NAMES = ("ln1_g", "ln1_b", "wq", "wkv", "wo", "bo", "ln2_g", "ln2_b", "w1", "b1", "w2", "b2", "lnf_g", "lnf_b")   # XFORMER_PTRS
# columns of both token tensors: 0 constant 1, TAG_COLS[t] 1 in planted key t alone; SEL_SHIFT / SEL_TAGS[t] the selector
# columns a query row's class is written in
TAG_COLS, SEL_SHIFT, SEL_TAGS, SEL_STEP = (1, 2), 127, (126, 125), 8.0
WRONG = ("padded key", "delta", "batch element", "last token", "argmax")


def case_id(case):
    B, N, depth, masks = case
    return f"{B}x{N}x{depth}" + ("m" if masks else "")


def xf_class(N):
    return torch.arange(N) % 4


def planted_keys(N):
    """The first and the last key (one key: that one)."""
    return [0] if N == 1 else [0, N - 1]


def planted_key(N, r):
    """The planted key of peaked query row r (r % 4 == 1): the rows take the positions in turn."""
    keys = planted_keys(N)
    return keys[(r // 4) % len(keys)]


def reserved_columns(N):
    """The token columns the construction owns: 0, the tag columns and the selector columns."""
    n = len(planted_keys(N))
    return [0] + list(TAG_COLS[:n]) + list(SEL_TAGS[:n])[::-1] + [SEL_SHIFT]


def _ln64(x, g, b):
    x = x.double()
    d = x - x.mean(-1, keepdim=True)
    return d / torch.sqrt((d * d).mean(-1, keepdim=True) + f32(EPS)) * g.double() + b.double()


def _plant_tokens(t):
    """Column 0 constant 1; the tag columns 1 in their planted key alone; every selector column the mean of the row's other
    columns (LayerNorm maps it to 0) plus -8 (low rows) / +8 (high rows) on the shift selector and +8 on the selector of the
    planted key a peaked row targets."""
    _B, N, _D = t.shape
    keys = planted_keys(N)
    sels = [SEL_SHIFT] + list(SEL_TAGS[:len(keys)])
    t[..., 0] = 1.0
    for j, key in enumerate(keys):
        t[..., TAG_COLS[j]] = 0.0
        t[:, key, TAG_COLS[j]] = 1.0
    other = torch.ones(DIM, dtype=torch.bool)
    other[sels] = False
    t[..., sels] = t[..., other].double().mean(-1, keepdim=True).float()
    cls = xf_class(N)
    t[:, cls == 2, SEL_SHIFT] -= SEL_STEP
    t[:, cls == 3, SEL_SHIFT] += SEL_STEP
    for r in range(1, N, 4):
        t[:, r, SEL_TAGS[keys.index(planted_key(N, r))]] += SEL_STEP


def _plant_instance(p, x, ctx_col0, heads):
    """The reserved features of a layer-0 instance with queries `x`: in every head feature 0 (the shift) and feature 1 + t (the
    tag of planted key t).  Their to_kv K-rows read context column 0 / tag column t alone with weight 1; their to_q rows read
    the shift / tag selector column of LN1(x) alone, with a gain taken from the fp64 LN1 output: the mean |logit| the step of 8
    gives is ATTN_SHIFT (shift) and ATTN_PEAK (tags) natural units.  ln1_b is 0 in the selector columns."""
    h, dh = heads
    _B, N, _D = x.shape
    keys = planted_keys(N)
    scale = f32(dh ** -0.5)
    sels = [SEL_SHIFT] + list(SEL_TAGS[:len(keys)])
    p["ln1_b"][sels] = 0.0
    xn = _ln64(x, p["ln1_g"], p["ln1_b"])
    cls = xf_class(N)
    rows = [(cls >= 2).nonzero().flatten().tolist()]
    rows += [[r for r in range(1, N, 4) if planted_key(N, r) == key] for key in keys]
    cols = [0] + list(TAG_COLS[:len(keys)])
    for f, (sel, col, rr) in enumerate(zip(sels, cols, rows)):
        size = float(xn[:, rr, sel].abs().mean()) if rr else SEL_STEP
        gain = (ATTN_SHIFT / ctx_col0 if f == 0 else ATTN_PEAK) / (scale * size)
        for hh in range(h):
            row = hh * dh + f
            p["wq"][row] = 0.0
            p["wq"][row, sel] = f32(gain)
            p["wkv"][row] = 0.0
            p["wkv"][row, col] = 1.0


def _near_ties(tok):
    """(B, dim) bool: the fp64 top-two gap of the column over the tokens is below TIE_GAP x max |tokens|; one token: no tie."""
    if tok.shape[1] == 1:
        return torch.zeros(tok.shape[0], tok.shape[2], dtype=torch.bool)
    top = tok.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) < TIE_GAP * float(tok.abs().max())


@functools.lru_cache(maxsize=None)
def xf_inputs(case, heads):
    """dict(mri, pet (B, N, 128), params [2 depth] of {name: tensor} in PARAM_NAMES, masks [2 depth][3] or None, dcls (B, 512),
    ties (B, 2, 128) bool, tie_share) of float32 tensors: Gaussian tokens and parameters at the scales of _params of
    tests/test_gpu_fusion_infer.py with the class construction on top (_plant_tokens, _plant_instance on instances 0 and 1);
    lnf_g is 0 in column 0 and the tag columns of every instance and lnf_b is 0 in the tag columns, so column 0 stays constant
    and the tags stay what they are down the chain.  The max half of dcls is 0 in the near-tie columns."""
    B, N, depth, with_masks = case
    h, dh = heads
    inner = h * dh
    idx = XF_CASES.index(tuple(case))
    g = torch.Generator().manual_seed(1000 * idx + 7919 * XF_SEED.get(tuple(case), 0) + h)

    def rn(*s, scale=1.0):
        return torch.randn(*s, generator=g) * scale
    mri, pet = rn(B, N, DIM), rn(B, N, DIM)
    params = []
    for _ in range(2 * depth):
        ts = [1 + rn(DIM, scale=0.1), rn(DIM, scale=0.1), rn(inner, DIM, scale=DIM ** -0.5), rn(2 * inner, DIM, scale=DIM ** -0.5),
              rn(DIM, inner, scale=inner ** -0.5), rn(DIM, scale=0.1), 1 + rn(DIM, scale=0.1), rn(DIM, scale=0.1),
              rn(MLP, DIM, scale=DIM ** -0.5), rn(MLP, scale=0.1), rn(DIM, MLP, scale=MLP ** -0.5), rn(DIM, scale=0.1),
              1 + rn(DIM, scale=0.1), rn(DIM, scale=0.1)]
        p = dict(zip(PARAM_NAMES, ts))
        tags = list(TAG_COLS[:len(planted_keys(N))])
        p["lnf_g"][[0] + tags] = 0.0
        p["lnf_b"][tags] = 0.0
        params.append(p)
    dcls = rn(B, 4 * DIM)
    _plant_tokens(mri)
    _plant_tokens(pet)
    _plant_instance(params[0], mri, 1.0, heads)
    _plant_instance(params[1], pet, 1.0 + float(params[0]["lnf_b"][0]), heads)     # its context is the new mri: y + mri
    masks = None
    if with_masks:
        from test_gpu_dropout_dims import _keep
        rs = np.random.RandomState(3 + idx)
        masks = [[_keep(rs, B * N, w).view(B, N, w) for w in (DIM, MLP, DIM)] for _ in range(2 * depth)]
    inp = dict(mri=mri, pet=pet, params=params, masks=masks, dcls=dcls)
    fw = xf_forward(inp, heads)
    ties = torch.stack([_near_ties(fw["mri"]), _near_ties(fw["pet"])], 1)
    dcls.view(B, 4, DIM)[:, 2:][ties] = 0.0
    inp.update(ties=ties, tie_share=float(ties.double().mean()))
    return inp


# ---------------------------------------------------------------------------------------------------------------------
# the formula, forward and backward, in one dtype and one order of its contractions
# ---------------------------------------------------------------------------------------------------------------------
class _Arith:
    """dtype and order of the sums: fp64 - torch's; fp32 "torch" - torch's own fp32 matmul and sum; fp32 "chain" - every
    contraction adds its rounded products one after the other (acc = round(acc + round(a_k b_k))).
    The chain restatement also has the attention in the form every backward that keeps no P has to take: logits in base 2
    (the constant scale log2(e) folded into one float), the log-sum-exp kept as ONE fp32 number per row, and a backward that
    recomputes P' = exp2(s' - lse) from logits s' summed in another order than the forward's (here from the last feature to the
    first), while
    delta = dout . out still comes from the forward's P.  A logit of +-100 natural units is 144 in base 2, where one fp32 ulp is
    1.5e-5: s' is another rounding of the same sum, so P' = P (1 +- 1e-5) in a low or high row, the rows of
    dS = P' (dP - delta) no longer sum to 0 to the last bit, and every sum that is 0 only because they do (dq of feature 0,
    the sum of dk of feature 0 over the keys, times +-ATTN_SHIFT / scale) carries that 1e-5 - which a restatement that hands
    the forward's own P to its backward does not show.  With such a restatement alone the first GPU run had column 0 of
    instance 0's lnf_b (that sum over the keys) at 1e-2 absolute with one launch per op, whose attention backward recomputes
    the logits in its own tile order, 2.5e-4 fused, whose backward repeats the forward's order, and 1.4e-4 / 2.5e-5 in the two
    restatements."""

    def __init__(self, dtype, order):
        self.dtype, self.chain = dtype, dtype != torch.float64 and order == "chain"

    def mm(self, a, b):
        """(..., n, K) x (..., K, m)"""
        if not self.chain:
            return a @ b
        acc = a[..., :, 0:1] * b[..., 0:1, :]
        for k in range(1, a.shape[-1]):
            acc = acc + a[..., :, k:k + 1] * b[..., k:k + 1, :]
        return acc

    def sum(self, t, axis):
        return _sum_axis(t, axis, "chain") if self.chain else t.sum(axis)

    def fn(self, f, x):
        """An elementary function, below fp64 correctly rounded (evaluated in fp64 and rounded once): the last bits of torch's
        own fp32 exp, erf and log2 depend on the CPU's vector width, and with logits of +-100 they decide which rounding every
        later step draws - with them 5 of the 21 cases measured a distance 2 .. 3 times off its recorded value on another
        CPU model, on identical inputs."""
        return f(x) if self.dtype == torch.float64 else f(x.double()).to(self.dtype)

    def ln(self, x, g, b):
        mean = self.sum(x, -1) / DIM
        d = x - mean.unsqueeze(-1)
        rstd = 1.0 / torch.sqrt(self.sum(d * d, -1) / DIM + f32(EPS))
        xhat = d * rstd.unsqueeze(-1)
        return xhat * g + b, xhat, rstd

    def ln_bwd(self, dy, g, xhat, rstd):
        """-> (dx, dgamma, dbeta): dx = rstd (gy - mean gy - xhat mean(gy xhat)), gy = dy gamma."""
        gy = dy * g
        s1 = self.sum(gy, -1) / DIM
        s2 = self.sum(gy * xhat, -1) / DIM
        dx = rstd.unsqueeze(-1) * (gy - s1.unsqueeze(-1) - xhat * s2.unsqueeze(-1))
        return dx, self.rows(dy * xhat), self.rows(dy)

    def rows(self, t):
        """sum over every token row of every batch element -> (width,)"""
        return self.sum(t.reshape(-1, t.shape[-1]), 0)

    def wgrad(self, dy, x):
        """dW (out, in) = sum over the token rows of dy[row, out] x[row, in]"""
        return self.mm(dy.reshape(-1, dy.shape[-1]).t(), x.reshape(-1, x.shape[-1]))


def _split(t, h):
    B, N, inner = t.shape
    return t.reshape(B, N, h, inner // h).permute(0, 2, 1, 3)


def _merge(t):
    B, h, N, dh = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, h * dh)


def _inst_fwd(A, p, mk, x, ctx, heads, wrong=None):
    """One Transformer(depth 1) instance: LN1, to_q | to_kv, softmax attention, to_out (+ mask) + x, LN2, Linear-GELU(-mask)-
    Linear(-mask) + x1, the final LN.  -> every intermediate the backward needs.  `wrong` (instance 0 only): "padded key" -
    one key of zero K and V rows (logit 0) joins the softmax; "batch element" - batch element 8 uses batch element 0's K / V."""
    h, dh = heads
    inner = h * dh
    scale = f32(dh ** -0.5)
    s = dict(x=x, ctx=ctx)
    s["xn1"], s["xh1"], s["r1"] = A.ln(x, p["ln1_g"], p["ln1_b"])
    q = A.mm(s["xn1"], p["wq"].t())
    kv = A.mm(ctx, p["wkv"].t())
    if wrong == "batch element":
        kv = kv.clone()
        kv[8] = kv[0]
    qh, kh, vh = _split(q, h), _split(kv[..., :inner], h), _split(kv[..., inner:], h)
    if wrong == "padded key":
        zero = torch.zeros_like(kh[:, :, :1])
        kh, vh = torch.cat([kh, zero], 2), torch.cat([vh, zero], 2)
    logit = A.mm(qh, kh.transpose(-1, -2))
    if A.chain:          # in base 2, as the kernels have it: the constant folded, the log-sum-exp kept in fp32
        s["c2"] = f32(f32(scale) * f32(LOG2E))
        logit = logit * s["c2"]
        mx = logit.max(-1, keepdim=True).values
        e = A.fn(torch.exp2, logit - mx)
        lsum = A.sum(e, -1).unsqueeze(-1)
        s["lse2"] = mx + A.fn(torch.log2, lsum)
    else:
        logit = logit * scale
        e = A.fn(torch.exp, logit - logit.max(-1, keepdim=True).values)
        lsum = A.sum(e, -1).unsqueeze(-1)
    P = e / lsum
    oh = A.mm(P, vh)
    s.update(qh=qh, kh=kh, vh=vh, P=P, oh=oh, logit=logit, out=_merge(oh))
    a = A.mm(s["out"], p["wo"].t()) + p["bo"]
    s["x1"] = (a if mk is None else a * mk[0]) + x
    s["xn2"], s["xh2"], s["r2"] = A.ln(s["x1"], p["ln2_g"], p["ln2_b"])
    s["hpre"] = A.mm(s["xn2"], p["w1"].t()) + p["b1"]
    gl = 0.5 * s["hpre"] * (1 + A.fn(torch.erf, s["hpre"] / 2 ** 0.5))
    s["hd"] = gl if mk is None else gl * mk[1]
    f = A.mm(s["hd"], p["w2"].t()) + p["b2"]
    x2 = (f if mk is None else f * mk[2]) + s["x1"]
    s["y"], s["xhf"], s["rf"] = A.ln(x2, p["lnf_g"], p["lnf_b"])
    return s


def _inst_bwd(A, p, mk, s, dy, heads, wrong=None, dy_terms=None):
    """The gradients of one instance under dy = d / dy: -> (dx (without the outer "+ x"), dctx, {gradient name: tensor}).
    `wrong` (instance 0 only): "padded key" - the recomputed P holds the padded key (it is in s); "delta" - delta of the last
    query row taken as 0; "last token" - the last token's row of dkv left out of dctx.
    fp64 only, in the returned dict: dwq_terms, dwkv_terms, dctx_terms, small_terms and lnf_terms, the magnitude the terms of
    these sums have before they cancel (xf_row_errors); `dy_terms`: that magnitude of dy itself where it is above |dy|."""
    h, dh = heads
    scale = f32(dh ** -0.5)
    g = {}
    dx2, g["lnf_g"], g["lnf_b"] = A.ln_bwd(dy, p["lnf_g"], s["xhf"], s["rf"])
    df = dx2 if mk is None else dx2 * mk[2]
    g["dw2"], g["b2"] = A.wgrad(df, s["hd"]), A.rows(df)
    dhd = A.mm(df, p["w2"])
    if mk is not None:
        dhd = dhd * mk[1]
    hp = s["hpre"]
    dh_ = dhd * (0.5 * (1 + A.fn(torch.erf, hp / 2 ** 0.5)) + hp * A.fn(torch.exp, -0.5 * hp * hp) / math.sqrt(2 * math.pi))
    g["dw1"], g["b1"] = A.wgrad(dh_, s["xn2"]), A.rows(dh_)
    dxn2 = A.mm(dh_, p["w1"])
    d, g["ln2_g"], g["ln2_b"] = A.ln_bwd(dxn2, p["ln2_g"], s["xh2"], s["r2"])
    dx1 = dx2 + d
    da = dx1 if mk is None else dx1 * mk[0]
    g["dwo"], g["bo"] = A.wgrad(da, s["out"]), A.rows(da)
    doh = _split(A.mm(da, p["wo"]), h)
    P, kh, vh, qh = s["P"], s["kh"], s["vh"], s["qh"]
    if A.chain:          # recomputed against the saved log-sum-exp from logits summed in ANOTHER order (_Arith says why)
        P = A.fn(torch.exp2, A.mm(qh.flip(-1), kh.flip(-1).transpose(-1, -2)) * s["c2"] - s["lse2"])
    dP = A.mm(doh, vh.transpose(-1, -2))
    delta = A.sum(doh * s["oh"], -1)
    if wrong == "delta":
        delta = delta.clone()
        delta[:, :, -1] = 0
    dS = P * (dP - delta.unsqueeze(-1))
    if A.dtype == torch.float64 and P.shape[-1] == 1 and wrong != "delta":
        dS = torch.zeros_like(dS)       # one key: P = 1, out = v, dP = delta - the fp64 value is 0, not the two sums' last bits
    dqh, dkh, dvh = A.mm(dS, kh) * scale, A.mm(dS.transpose(-1, -2), qh) * scale, A.mm(P.transpose(-1, -2), doh)
    if wrong == "padded key":
        dkh, dvh = dkh[:, :, :-1], dvh[:, :, :-1]
    dq, dkv = _merge(dqh), torch.cat([_merge(dkh), _merge(dvh)], -1)
    g["dwq"], g["dwkv"] = A.wgrad(dq, s["xn1"]), A.wgrad(dkv, s["ctx"])
    if A.dtype == torch.float64:
        dS_mag = P * (dP.abs() + delta.abs().unsqueeze(-1))         # |P dP| + |P delta|: dS before ITS two terms cancel
        dq_terms = _merge(A.mm(dS_mag, kh.abs())) * scale
        g["dwq_terms"] = A.wgrad(dq_terms, s["xn1"].abs())
        dkv_terms = torch.cat([_merge(A.mm(dS_mag.transpose(-1, -2), qh.abs())[:, :, :dvh.shape[2]]) * scale, _merge(dvh).abs()], -1)
        g["dwkv_terms"] = A.wgrad(dkv_terms, s["ctx"].abs())
        g["dctx_terms"] = A.mm(dkv_terms, p["wkv"].abs())
        dyt = dy.abs() if dy_terms is None else dy_terms
        dxn1_terms = A.mm(dq_terms, p["wq"].abs())
        g["dx_terms"] = s["r1"].unsqueeze(-1) * dxn1_terms * p["ln1_g"].abs()       # the leading term of LN1's backward
        t = dict(b2=df.abs(), b1=dh_.abs(), bo=da.abs(), ln2_g=(dxn2 * s["xh2"]).abs(), ln2_b=dxn2.abs(),
                 ln1_g=dxn1_terms * s["xh1"].abs(), ln1_b=dxn1_terms, lnf_g=dyt * s["xhf"].abs(), lnf_b=dyt)
        g["small_terms"] = torch.cat([A.rows(t[n]) for n, _w in SMALL_SEGMENTS])
        g["lnf_terms"] = torch.cat([A.rows(t[n]) for n, _w in LNF_SEGMENTS])
    if wrong == "last token":
        dkv = dkv.clone()
        dkv[:, -1] = 0
    dctx = A.mm(dkv, p["wkv"])
    dxn1 = A.mm(dq, p["wq"])
    d, g["ln1_g"], g["ln1_b"] = A.ln_bwd(dxn1, p["ln1_g"], s["xh1"], s["r1"])
    # what each segment of small and lnf sums over the token rows (xf_restatement_distance)
    t = dict(b2=df, b1=dh_, bo=da, ln2_g=dxn2 * s["xh2"], ln2_b=dxn2, ln1_g=dxn1 * s["xh1"], ln1_b=dxn1, lnf_g=dy * s["xhf"], lnf_b=dy)
    g["small_summands"] = torch.cat([t[n].reshape(-1, w) for n, w in SMALL_SEGMENTS], 1)
    g["lnf_summands"] = torch.cat([t[n].reshape(-1, w) for n, w in LNF_SEGMENTS], 1)
    return dx1 + d, dctx, g


def _cast(inp, dtype):
    masks = inp["masks"]
    return (inp["mri"].to(dtype), inp["pet"].to(dtype), [{k: v.to(dtype) for k, v in p.items()} for p in inp["params"]],
            [None if masks is None else [m.to(dtype) for m in mk] for mk in (masks or [None] * len(inp["params"]))])


def xf_forward(inp, heads, dtype=torch.float64, order="torch", wrong=None):
    """mri <- inst(mri | pet) + mri, pet <- inst(pet | new mri) + pet per layer, then cls = [mean mri | mean pet | max mri |
    max pet] over the tokens -> dict(cls, mri, pet (the final tokens), saved [2 depth], argmax (B, 2, 128))."""
    A = _Arith(dtype, order)
    mri, pet, params, masks = _cast(inp, dtype)
    saved = []
    for i in range(0, len(params), 2):
        saved.append(_inst_fwd(A, params[i], masks[i], mri, pet, heads, wrong if i == 0 and wrong in ("padded key", "batch element") else None))
        mri = saved[-1]["y"] + mri
        saved.append(_inst_fwd(A, params[i + 1], masks[i + 1], pet, mri, heads))
        pet = saved[-1]["y"] + pet
    N = mri.shape[1]
    mx = [t.max(1) for t in (mri, pet)]
    cls = torch.cat([A.sum(mri, 1) / N, A.sum(pet, 1) / N, mx[0].values, mx[1].values], 1)
    return dict(cls=cls, mri=mri, pet=pet, saved=saved, argmax=torch.stack([mx[0].indices, mx[1].indices], 1))


def xf_ref(inp, heads, dtype=torch.float64, order="torch", wrong=None):
    """Every judged quantity in `dtype`: cls (B, 512), dmri_tok, dpet_tok (B, N, 128), per instance k "i{k}.dwq" ... "i{k}.dw2"
    (nn.Linear layout), "i{k}.small" (SMALL_SEGMENTS in a row) and "i{k}.lnf"; fp64 also "i{k}.dwq_terms" and, under "fwd", the
    forward's intermediates.  `wrong`: one of WRONG - a deliberately wrong result for the host test that shows the tolerances
    reject it ("argmax": the max-pool column of mri, batch row 0, with the largest |dcls| routed to the runner-up token)."""
    A = _Arith(dtype, order)
    fw = xf_forward(inp, heads, dtype, order, wrong)
    _mri, _pet, params, masks = _cast(inp, dtype)
    B, N, _D = fw["mri"].shape
    d = inp["dcls"].to(dtype).view(B, 4, DIM)
    am = fw["argmax"]
    if wrong == "argmax":
        c = int(d[0, 2].abs().argmax())
        am = am.clone()
        am[0, 0, c] = fw["mri"][0, :, c].topk(2).indices[1]
    hit = torch.arange(N).view(1, 1, N, 1) == am.view(B, 2, 1, DIM)
    dtok = d[:, :2].unsqueeze(2) / N + hit * d[:, 2:].unsqueeze(2)
    dmri, dpet = dtok[:, 0], dtok[:, 1]
    res = dict(cls=fw["cls"])
    for i in range(len(params) - 2, -1, -2):
        dx, dctx, g1 = _inst_bwd(A, params[i + 1], masks[i + 1], fw["saved"][i + 1], dpet, heads)
        dpet, dmri = dpet + dx, dmri + dctx
        dx, dctx, g0 = _inst_bwd(A, params[i], masks[i], fw["saved"][i], dmri, heads,
                                 wrong if i == 0 and wrong in ("padded key", "delta", "last token") else None,
                                 dmri.abs() + g1["dctx_terms"] if i == 0 and "dctx_terms" in g1 else None)
        dmri, dpet = dmri + dx, dpet + dctx
        for k, g in ((i, g0), (i + 1, g1)):
            for name in WEIGHTS:
                res[f"i{k}.{name}"] = g[name]
            res[f"i{k}.small"] = torch.cat([g[n] for n, _w in SMALL_SEGMENTS])
            res[f"i{k}.lnf"] = torch.cat([g[n] for n, _w in LNF_SEGMENTS])
            for name in ("dwq_terms", "dwkv_terms", "small_terms", "lnf_terms", "small_summands", "lnf_summands"):
                if name in g:
                    res[f"i{k}.{name}"] = g[name]
    res.update(dmri_tok=dmri, dpet_tok=dpet)
    if dtype == torch.float64:
        res["fwd"] = fw
        # instance 0's context is pet, instance 1's the new mri, whose gradient reaches dmri_tok through the "+ mri"
        # and its queries are mri (instance 1: pet), which dq reaches through to_q and LN1
        res["dpet_tok_terms"] = dpet.abs() + (g0["dctx_terms"] + g1["dx_terms"] if params else 0)
        res["dmri_tok_terms"] = dmri.abs() + (g1["dctx_terms"] + g0["dx_terms"] if params else 0)
    return res


def xf_autograd(inp, heads):
    """The same quantities in fp64 from torch.softmax, F.layer_norm, F.gelu and autograd -> (cls, dmri_tok, dpet_tok,
    [per instance {parameter name: gradient}])."""
    import torch.nn.functional as F
    h, _dh = heads
    mri, pet, params, masks = _cast(inp, torch.float64)
    mri, pet = mri.requires_grad_(True), pet.requires_grad_(True)
    for p in params:
        for v in p.values():
            v.requires_grad_(True)

    def inst(p, mk, x, ctx):
        one = torch.ones(()) if mk is None else None
        mo, mg, mf = (one, one, one) if mk is None else mk
        xn = F.layer_norm(x, (DIM,), p["ln1_g"], p["ln1_b"], f32(EPS))
        q, (k, v) = xn @ p["wq"].t(), (ctx @ p["wkv"].t()).chunk(2, -1)
        dots = torch.einsum("bhid,bhjd->bhij", _split(q, h), _split(k, h)) * f32((q.shape[-1] // h) ** -0.5)
        out = _merge(torch.einsum("bhij,bhjd->bhid", dots.softmax(-1), _split(v, h)))
        x1 = (out @ p["wo"].t() + p["bo"]) * mo + x
        hd = F.gelu(F.layer_norm(x1, (DIM,), p["ln2_g"], p["ln2_b"], f32(EPS)) @ p["w1"].t() + p["b1"]) * mg
        return F.layer_norm((hd @ p["w2"].t() + p["b2"]) * mf + x1, (DIM,), p["lnf_g"], p["lnf_b"], f32(EPS))
    m, q = mri, pet
    for i in range(0, len(params), 2):
        m = inst(params[i], masks[i], m, q) + m
        q = inst(params[i + 1], masks[i + 1], q, m) + q
    cls = torch.cat([m.mean(1), q.mean(1), m.max(1).values, q.max(1).values], 1)
    cls.backward(inp["dcls"].double())
    return cls.detach(), mri.grad, pet.grad, [{k: v.grad for k, v in p.items()} for p in params]


# ---------------------------------------------------------------------------------------------------------------------
# judgment
# ---------------------------------------------------------------------------------------------------------------------
def row_error(got, ref, terms=None):
    """Per row (the last axis) of `ref`: max |got - ref| over the row's scale - max |ref| of the row, or max `terms` of the row
    where that is given.  A row whose scale is exactly zero in fp64 is judged by its absolute error.  A row with a non-finite
    element has error inf."""
    ref = ref.double()
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs().amax(-1)
    scale = (ref if terms is None else terms.double()).abs().amax(-1)
    rel = torch.where(scale > 0, err / scale.clamp_min(1e-300), err)
    return torch.where(torch.isfinite(got).all(-1), rel, torch.full_like(rel, math.inf))


def xf_row_errors(got, ref64):
    """{(quantity, class): tensor of row errors}, the rows in the order of the tensor.
    cls: per batch row, the mean half and the max half apart.
    dmri_tok, dpet_tok: per token row, by the row's class r % 4, in two column groups, as dk of tests/_attn_inputs.py.  Column 0
    of a context's gradient is sum_f Wkv[f, 0] dk_f with dk of feature 0 = scale sum_i dS_ij q_i0 and q_i0 = +-ATTN_SHIFT /
    scale in the shifted queries: it holds the maximum of nearly every row, 20 .. 600 times the Gaussian columns, so one scale
    for the whole row would let a Gaussian column be replaced by zero unnoticed; and its terms have both signs - in the few
    rows where they cancel to a thousandth, max |fp64| of the row says nothing about the error fp32 makes (row errors of 2e-3
    against a median of 1.4e-5 at (1, 512)) and that row's error would be every row's tolerance.  So the Gaussian columns
    ("dmri_tok") are judged on their own max |fp64|, and the reserved columns ("dmri_tok.reserved": column 0, the tags, the
    selectors) on the largest sum of their terms' MAGNITUDES: |fp64| + (scale sum_i |dS_ij| |q_i| , |dv|) |Wkv| of the layer-0
    instance whose context the tensor is, + rstd |ln1_g| (scale sum_j P_ij (|dP_ij| + |delta_i|) |k_j|) |Wq| of the one whose
    queries it is (`dmri_tok_terms`) - never below max |fp64| of those columns.
    Every dw*: per weight row (class "rows"), the scale max |fp64| of the row - except dwq and dwkv, whose scale is the largest
    sum of their terms' MAGNITUDES, sum_r scale sum_j |dS_rj| |k_jf| |LN1(x)_rc| (`dwq_terms`; `dwkv_terms` likewise from
    scale sum_i |dS_ij| |q_if| and |dv|), as dk_terms of tests/_attn_inputs.py: feature 0 of every key of a layer-0 instance is
    the same number, so dq of feature 0 is that number times the sum of a dS row, which is 0 - the fp64 value of such a dwq
    row is 1e-17 of its terms and says nothing about the error fp32 makes (tests/test_host_xf.py shows the cancellation); and
    dk of feature 0 is a sum of terms +-ATTN_SHIFT / scale times dS that adds up to 0 over the keys, which a dwkv row then
    multiplies by the context's constant column.
    small and lnf: per segment, every one a sum over all token rows: the scale is the largest sum of the terms' magnitudes in
    the segment (sum_r |dy_r|, sum_r |dy_r xhat_r|, as dgamma_terms of tests/_token_inputs.py), the terms of instance 0's own dy
    being those of dmri_tok.reserved - column 0 of its lnf_b is the sum over the keys just named.  The first GPU run, with
    max |fp64| of the segment as the scale, had that lnf_b at 19 tolerances with one launch per op and at 1.3 .. 2.6 fused,
    everything else of both paths within 2: both paths alike, the yardstick's scale was what was wrong.  A segment of dim
    columns is judged in the two column groups of the token gradients (segment_groups)."""
    out = {}
    N = ref64["dmri_tok"].shape[1]
    c = got["cls"].double().view(-1, 2, 2 * DIM)
    r = ref64["cls"].view(-1, 2, 2 * DIM)
    out[("cls", "mean")], out[("cls", "max")] = row_error(c[:, 0], r[:, 0]), row_error(c[:, 1], r[:, 1])
    cls = xf_class(N)
    res = reserved_columns(N)
    feat = [c for c in range(DIM) if c not in res]
    for name in ("dmri_tok", "dpet_tok"):
        g, r = got[name].reshape(ref64[name].shape), ref64[name]
        groups = ((name, row_error(g[..., feat], r[..., feat])),
                  (name + ".reserved", row_error(g[..., res], r[..., res], ref64[name + "_terms"][..., res])))
        for key, rel in groups:
            for k, cname in enumerate(XF_CLASSES):
                if bool((cls == k).any()):
                    out[(key, cname)] = rel[:, cls == k]
    for key in ref64:
        inst, _, name = key.partition(".")
        if name in WEIGHTS:
            out[(key, "rows")] = row_error(got[key], ref64[key], ref64.get(key + "_terms"))
        elif name in ("small", "lnf"):
            for seg, cols in segment_groups(name, N):
                out[(key, seg)] = row_error(got[key].reshape(-1)[cols], ref64[key][cols], ref64[key + "_terms"][cols])
    return out


def segment_groups(name, N):
    """[(segment or segment + ".reserved", its columns in `small` / `lnf`)]: a segment of dim columns in two groups, the Gaussian
    columns and reserved_columns(N), as the token gradients and for the same reason."""
    res = reserved_columns(N)
    feat = [c for c in range(DIM) if c not in res]
    out, at = [], 0
    for seg, w in (SMALL_SEGMENTS if name == "small" else LNF_SEGMENTS):
        if w == DIM:
            out += [(seg, [at + c for c in feat]), (seg + ".reserved", [at + c for c in res])]
        else:
            out.append((seg, list(range(at, at + w))))
        at += w
    return out


def xf_distances(got, ref64):
    return {key: float(v.max()) for key, v in xf_row_errors(got, ref64).items()}


def summand_distances(got, ref64):
    """{(quantity, segment group): root-sum-square over the token rows of the errors in what the segment SUMS, over the group's
    scale}.  The error of a sum over R rows whose terms are each wrong by e_r is ONE draw from a distribution of width
    sqrt(sum e_r^2); where one column holds a group's scale (column 0 of instance 0's lnf: +-ATTN_SHIFT / scale times dS, summed
    over the keys) the |error| of a restatement is that one draw and may be anything from 0 up - the first GPU runs had
    kernels at 6 .. 9 x 2^-24 of the scale there against restatement draws of 0.2 .. 10 x 2^-24 from case to case.  The width
    is what a tolerance can be built on: a restatement's distance of a segment group is the larger of its draw and this."""
    out = {}
    N = ref64["dmri_tok"].shape[1]
    for key in ref64:
        _inst, _, name = key.partition(".")
        if name in ("small", "lnf"):
            e = (got[key + "_summands"].double() - ref64[key + "_summands"]).pow(2).sum(0).sqrt()
            for seg, cols in segment_groups(name, N):
                out[(key, seg)] = float(row_error(e[cols] + ref64[key][cols], ref64[key][cols], ref64[key + "_terms"][cols]))
    return out


def xf_margin(case, heads, key):
    return XF_MARGIN.get((tuple(case), heads[0]) + tuple(key), MARGIN)


def xf_tolerance(case, heads, key):
    """margin x floor_distance(recorded distance) of one (quantity, class).  The reserved columns of a segment of small / lnf are
    six columns of the same sum in the same arithmetic as the segment's 122 Gaussian columns; the largest error of six draws
    says less about the width of their distribution than that of 122, so they are held to the larger of the two groups'
    recorded distances, each on its own scale (at (1, 496) and 8 heads the fused kernels' bo has an error of 2.8e-6 rms over
    all 128 columns, 0.9 tolerances in the Gaussian group; 8.2e-6 in column 126 was 1.6 of the six columns' own)."""
    rec = XF_DISTANCE[(tuple(case), heads[0])]
    d = rec[key]
    if key[1].endswith(".reserved") and key[0].endswith((".small", ".lnf")):
        d = max(d, rec[(key[0], key[1][:-len(".reserved")])])
    return xf_margin(case, heads, key) * floor_distance(d)


def xf_ratios(got, ref64, case, heads):
    """{(quantity, class): worst row error over its tolerance}; above 1 fails."""
    return {key: d / xf_tolerance(case, heads, key) for key, d in xf_distances(got, ref64).items()}


def xf_restatement_distance(case, heads):
    """The larger of the two fp32 restatements' distances from fp64, per (quantity, class)."""
    inp = xf_inputs(case, heads)
    r64 = xf_ref(inp, heads)
    out = {}
    for order in ("torch", "chain"):
        r32 = xf_ref(inp, heads, torch.float32, order)
        for d in (xf_distances(r32, r64), summand_distances(r32, r64)):
            for key, v in d.items():
                out[key] = max(out.get(key, 0.0), v)
    return out


def print_tables():
    """Maintenance: the text between BEGIN TABLES and END TABLES."""
    print("XF_DISTANCE = {      # (case, heads) -> {(quantity, class): distance}")
    for case in XF_CASES:
        for heads in XF_HEADS:
            d = xf_restatement_distance(case, heads)
            print(f"    ({case}, {heads[0]}): {{" + ", ".join(f"{k}: {v:.2e}" for k, v in d.items()) + "},", flush=True)
    print("}")


# A margin of its own, keyed by case, heads, quantity and class, with its cause (as ATTN_MARGIN of tests/_attn_inputs.py).
# (1, 1, 1) is the one case with margins of its own: 4 x MARGIN, as there, for the quantities in which ONE number decides.
# - dq is 0 in fp64 (one key: P = 1, dS = dP - delta = 0); what fp32 returns is nu = the difference of two roundings of one
#   dh-term dot product (matrix pipe against fma chain in the fused kernels, matmul against sum in the restatements), 0 or a
#   few ulps of |dP| per head.  The to_q rows of feature 0 multiply it by a gain of 70 into the selector column of LN1's
#   gradient: the reserved columns of ln1_b, ln1_g and of the query tensor's token gradient are nu times that gain and nothing
#   else, and with one token there is one such number per head, not a maximum over hundreds of rows.  The recorded distance is
#   one draw of nu (8e-7 .. 5e-6 of the scale); the fused kernels drew 2.7e-5 of ln1_b's scale at both head geometries, 1.5 and
#   8.2 tolerances, one launch per op 0.6.
# - with one token a weight-gradient row is ONE product dy_o x, so its error over max |fp64| of the row is the relative error
#   of dy_o, a sum of 128 .. 512 terms that cancels to any degree: the worst of 128 .. 512 such ratios has no typical size
#   (i1.dwkv was at 1.06 tolerances fused at 4 heads, i0.dw2 at 1.28 at 8 heads, every other weight row of the case below 1).
XF_MARGIN = {((1, 1, 1, False), h, q, c): 4 * MARGIN for h in (4, 8)
             for q, c in [(f"i{k}.{w}", "rows") for k in (0, 1) for w in WEIGHTS]}

# ---------------------------------------------------------------------------------------------------------------------
# recorded restatement distances (torch 2.x CPU, fp32 against fp64); tests/test_host_xf.py measures them again and fails on a
# drift beyond 2x.  A value enters a tolerance through floor_distance().
# ---------------------------------------------------------------------------------------------------------------------
# BEGIN TABLES
XF_DISTANCE = {      # (case, heads) -> {(quantity, class): distance}
    ((1, 1, 1, False), 4): {('cls', 'mean'): 1.99e-07, ('cls', 'max'): 1.99e-07, ('dmri_tok', 'flat'): 2.62e-07, ('dmri_tok.reserved', 'flat'): 2.95e-08, ('dpet_tok', 'flat'): 1.82e-07, ('dpet_tok.reserved', 'flat'): 1.83e-08, ('i0.dwq', 'rows'): 1.84e-07, ('i0.dwkv', 'rows'): 1.20e-04, ('i0.dwo', 'rows'): 2.40e-05, ('i0.dw1', 'rows'): 1.09e-04, ('i0.dw2', 'rows'): 3.09e-05, ('i0.small', 'b2'): 3.28e-07, ('i0.small', 'b2.reserved'): 3.19e-07, ('i0.small', 'b1'): 4.18e-07, ('i0.small', 'bo'): 4.11e-07, ('i0.small', 'bo.reserved'): 3.22e-07, ('i0.small', 'ln2_g'): 5.22e-07, ('i0.small', 'ln2_g.reserved'): 2.13e-07, ('i0.small', 'ln2_b'): 7.75e-07, ('i0.small', 'ln2_b.reserved'): 6.39e-07, ('i0.small', 'ln1_g'): 1.13e-08, ('i0.small', 'ln1_g.reserved'): 1.25e-08, ('i0.small', 'ln1_b'): 2.53e-08, ('i0.small', 'ln1_b.reserved'): 3.13e-08, ('i0.lnf', 'lnf_g'): 5.55e-08, ('i0.lnf', 'lnf_g.reserved'): 1.80e-08, ('i0.lnf', 'lnf_b'): 4.19e-08, ('i0.lnf', 'lnf_b.reserved'): 1.09e-08, ('i1.dwq', 'rows'): 2.46e-07, ('i1.dwkv', 'rows'): 7.07e-05, ('i1.dwo', 'rows'): 1.17e-04, ('i1.dw1', 'rows'): 9.17e-04, ('i1.dw2', 'rows'): 9.92e-06, ('i1.small', 'b2'): 1.67e-07, ('i1.small', 'b2.reserved'): 1.52e-07, ('i1.small', 'b1'): 4.95e-07, ('i1.small', 'bo'): 2.14e-07, ('i1.small', 'bo.reserved'): 2.27e-07, ('i1.small', 'ln2_g'): 6.83e-07, ('i1.small', 'ln2_g.reserved'): 2.45e-07, ('i1.small', 'ln2_b'): 8.71e-07, ('i1.small', 'ln2_b.reserved'): 6.00e-07, ('i1.small', 'ln1_g'): 9.89e-09, ('i1.small', 'ln1_g.reserved'): 2.92e-09, ('i1.small', 'ln1_b'): 1.45e-08, ('i1.small', 'ln1_b.reserved'): 1.92e-08, ('i1.lnf', 'lnf_g'): 2.67e-07, ('i1.lnf', 'lnf_g.reserved'): 3.76e-07, ('i1.lnf', 'lnf_b'): 5.36e-08, ('i1.lnf', 'lnf_b.reserved'): 2.92e-08},
    ((1, 1, 1, False), 8): {('cls', 'mean'): 1.67e-07, ('cls', 'max'): 1.67e-07, ('dmri_tok', 'flat'): 2.35e-07, ('dmri_tok.reserved', 'flat'): 1.80e-08, ('dpet_tok', 'flat'): 1.73e-07, ('dpet_tok.reserved', 'flat'): 2.35e-08, ('i0.dwq', 'rows'): 1.13e-06, ('i0.dwkv', 'rows'): 2.49e-04, ('i0.dwo', 'rows'): 8.72e-05, ('i0.dw1', 'rows'): 2.01e-04, ('i0.dw2', 'rows'): 2.09e-05, ('i0.small', 'b2'): 2.90e-07, ('i0.small', 'b2.reserved'): 2.86e-07, ('i0.small', 'b1'): 2.58e-07, ('i0.small', 'bo'): 3.53e-07, ('i0.small', 'bo.reserved'): 3.14e-07, ('i0.small', 'ln2_g'): 7.04e-07, ('i0.small', 'ln2_g.reserved'): 8.04e-07, ('i0.small', 'ln2_b'): 5.91e-07, ('i0.small', 'ln2_b.reserved'): 5.70e-07, ('i0.small', 'ln1_g'): 1.24e-08, ('i0.small', 'ln1_g.reserved'): 9.04e-09, ('i0.small', 'ln1_b'): 1.30e-08, ('i0.small', 'ln1_b.reserved'): 1.82e-08, ('i0.lnf', 'lnf_g'): 3.82e-08, ('i0.lnf', 'lnf_g.reserved'): 1.95e-08, ('i0.lnf', 'lnf_b'): 4.13e-08, ('i0.lnf', 'lnf_b.reserved'): 2.26e-08, ('i1.dwq', 'rows'): 7.23e-07, ('i1.dwkv', 'rows'): 2.51e-05, ('i1.dwo', 'rows'): 9.75e-06, ('i1.dw1', 'rows'): 7.39e-05, ('i1.dw2', 'rows'): 3.93e-05, ('i1.small', 'b2'): 1.29e-07, ('i1.small', 'b2.reserved'): 4.62e-08, ('i1.small', 'b1'): 4.33e-07, ('i1.small', 'bo'): 2.36e-07, ('i1.small', 'bo.reserved'): 7.12e-07, ('i1.small', 'ln2_g'): 4.09e-07, ('i1.small', 'ln2_g.reserved'): 1.03e-06, ('i1.small', 'ln2_b'): 6.50e-07, ('i1.small', 'ln2_b.reserved'): 5.06e-07, ('i1.small', 'ln1_g'): 1.16e-08, ('i1.small', 'ln1_g.reserved'): 1.96e-08, ('i1.small', 'ln1_b'): 2.28e-08, ('i1.small', 'ln1_b.reserved'): 2.50e-08, ('i1.lnf', 'lnf_g'): 6.32e-07, ('i1.lnf', 'lnf_g.reserved'): 3.74e-07, ('i1.lnf', 'lnf_b'): 2.95e-08, ('i1.lnf', 'lnf_b.reserved'): 2.12e-08},
    ((3, 16, 1, False), 4): {('cls', 'mean'): 2.28e-06, ('cls', 'max'): 1.91e-06, ('dmri_tok', 'flat'): 2.59e-06, ('dmri_tok', 'peaked'): 8.85e-06, ('dmri_tok', 'low'): 2.08e-05, ('dmri_tok', 'high'): 2.37e-05, ('dmri_tok.reserved', 'flat'): 5.62e-06, ('dmri_tok.reserved', 'peaked'): 6.27e-06, ('dmri_tok.reserved', 'low'): 4.42e-06, ('dmri_tok.reserved', 'high'): 6.86e-06, ('dpet_tok', 'flat'): 2.04e-06, ('dpet_tok', 'peaked'): 4.26e-06, ('dpet_tok', 'low'): 3.35e-05, ('dpet_tok', 'high'): 1.92e-05, ('dpet_tok.reserved', 'flat'): 3.02e-06, ('dpet_tok.reserved', 'peaked'): 6.82e-06, ('dpet_tok.reserved', 'low'): 9.70e-06, ('dpet_tok.reserved', 'high'): 4.94e-06, ('i0.dwq', 'rows'): 6.18e-06, ('i0.dwkv', 'rows'): 7.37e-06, ('i0.dwo', 'rows'): 2.07e-05, ('i0.dw1', 'rows'): 4.28e-05, ('i0.dw2', 'rows'): 1.32e-05, ('i0.small', 'b2'): 2.34e-06, ('i0.small', 'b2.reserved'): 1.51e-06, ('i0.small', 'b1'): 1.87e-06, ('i0.small', 'bo'): 2.34e-06, ('i0.small', 'bo.reserved'): 1.21e-06, ('i0.small', 'ln2_g'): 2.63e-06, ('i0.small', 'ln2_g.reserved'): 1.18e-06, ('i0.small', 'ln2_b'): 2.38e-06, ('i0.small', 'ln2_b.reserved'): 1.88e-06, ('i0.small', 'ln1_g'): 1.85e-07, ('i0.small', 'ln1_g.reserved'): 6.40e-07, ('i0.small', 'ln1_b'): 1.68e-07, ('i0.small', 'ln1_b.reserved'): 3.30e-07, ('i0.lnf', 'lnf_g'): 1.84e-07, ('i0.lnf', 'lnf_g.reserved'): 4.74e-07, ('i0.lnf', 'lnf_b'): 1.56e-07, ('i0.lnf', 'lnf_b.reserved'): 3.29e-07, ('i1.dwq', 'rows'): 3.00e-06, ('i1.dwkv', 'rows'): 8.50e-06, ('i1.dwo', 'rows'): 1.67e-05, ('i1.dw1', 'rows'): 3.62e-05, ('i1.dw2', 'rows'): 1.25e-05, ('i1.small', 'b2'): 1.01e-06, ('i1.small', 'b2.reserved'): 1.11e-06, ('i1.small', 'b1'): 2.13e-06, ('i1.small', 'bo'): 1.19e-06, ('i1.small', 'bo.reserved'): 1.17e-06, ('i1.small', 'ln2_g'): 2.56e-06, ('i1.small', 'ln2_g.reserved'): 3.91e-06, ('i1.small', 'ln2_b'): 1.66e-06, ('i1.small', 'ln2_b.reserved'): 9.83e-07, ('i1.small', 'ln1_g'): 1.77e-07, ('i1.small', 'ln1_g.reserved'): 4.97e-07, ('i1.small', 'ln1_b'): 1.41e-07, ('i1.small', 'ln1_b.reserved'): 2.37e-07, ('i1.lnf', 'lnf_g'): 3.78e-06, ('i1.lnf', 'lnf_g.reserved'): 1.42e-06, ('i1.lnf', 'lnf_b'): 3.99e-07, ('i1.lnf', 'lnf_b.reserved'): 1.72e-07},
    ((3, 16, 1, False), 8): {('cls', 'mean'): 1.68e-06, ('cls', 'max'): 9.62e-07, ('dmri_tok', 'flat'): 2.00e-06, ('dmri_tok', 'peaked'): 2.79e-06, ('dmri_tok', 'low'): 7.79e-06, ('dmri_tok', 'high'): 6.99e-06, ('dmri_tok.reserved', 'flat'): 2.64e-06, ('dmri_tok.reserved', 'peaked'): 1.83e-06, ('dmri_tok.reserved', 'low'): 2.48e-06, ('dmri_tok.reserved', 'high'): 2.13e-06, ('dpet_tok', 'flat'): 1.37e-06, ('dpet_tok', 'peaked'): 1.53e-06, ('dpet_tok', 'low'): 1.76e-05, ('dpet_tok', 'high'): 1.20e-05, ('dpet_tok.reserved', 'flat'): 2.23e-06, ('dpet_tok.reserved', 'peaked'): 1.86e-06, ('dpet_tok.reserved', 'low'): 1.46e-06, ('dpet_tok.reserved', 'high'): 2.25e-06, ('i0.dwq', 'rows'): 1.71e-06, ('i0.dwkv', 'rows'): 6.34e-06, ('i0.dwo', 'rows'): 1.41e-05, ('i0.dw1', 'rows'): 2.73e-05, ('i0.dw2', 'rows'): 8.23e-06, ('i0.small', 'b2'): 1.28e-06, ('i0.small', 'b2.reserved'): 1.16e-06, ('i0.small', 'b1'): 1.36e-06, ('i0.small', 'bo'): 1.05e-06, ('i0.small', 'bo.reserved'): 1.11e-06, ('i0.small', 'ln2_g'): 1.93e-06, ('i0.small', 'ln2_g.reserved'): 7.02e-07, ('i0.small', 'ln2_b'): 1.57e-06, ('i0.small', 'ln2_b.reserved'): 5.24e-07, ('i0.small', 'ln1_g'): 6.73e-08, ('i0.small', 'ln1_g.reserved'): 1.85e-07, ('i0.small', 'ln1_b'): 7.95e-08, ('i0.small', 'ln1_b.reserved'): 8.06e-08, ('i0.lnf', 'lnf_g'): 1.06e-07, ('i0.lnf', 'lnf_g.reserved'): 3.29e-07, ('i0.lnf', 'lnf_b'): 1.09e-07, ('i0.lnf', 'lnf_b.reserved'): 1.55e-07, ('i1.dwq', 'rows'): 3.16e-06, ('i1.dwkv', 'rows'): 4.99e-06, ('i1.dwo', 'rows'): 1.16e-05, ('i1.dw1', 'rows'): 2.39e-05, ('i1.dw2', 'rows'): 6.65e-06, ('i1.small', 'b2'): 4.24e-07, ('i1.small', 'b2.reserved'): 5.91e-07, ('i1.small', 'b1'): 1.61e-06, ('i1.small', 'bo'): 7.52e-07, ('i1.small', 'bo.reserved'): 6.40e-07, ('i1.small', 'ln2_g'): 1.54e-06, ('i1.small', 'ln2_g.reserved'): 5.39e-07, ('i1.small', 'ln2_b'): 1.04e-06, ('i1.small', 'ln2_b.reserved'): 7.04e-07, ('i1.small', 'ln1_g'): 9.19e-08, ('i1.small', 'ln1_g.reserved'): 1.83e-07, ('i1.small', 'ln1_b'): 9.13e-08, ('i1.small', 'ln1_b.reserved'): 1.28e-07, ('i1.lnf', 'lnf_g'): 1.47e-06, ('i1.lnf', 'lnf_g.reserved'): 4.82e-07, ('i1.lnf', 'lnf_b'): 4.88e-07, ('i1.lnf', 'lnf_b.reserved'): 4.58e-07},
    ((2, 17, 2, False), 4): {('cls', 'mean'): 1.79e-06, ('cls', 'max'): 1.68e-06, ('dmri_tok', 'flat'): 4.82e-06, ('dmri_tok', 'peaked'): 3.96e-06, ('dmri_tok', 'low'): 1.00e-05, ('dmri_tok', 'high'): 1.69e-05, ('dmri_tok.reserved', 'flat'): 5.41e-06, ('dmri_tok.reserved', 'peaked'): 6.90e-06, ('dmri_tok.reserved', 'low'): 3.25e-06, ('dmri_tok.reserved', 'high'): 6.15e-06, ('dpet_tok', 'flat'): 3.88e-06, ('dpet_tok', 'peaked'): 2.28e-06, ('dpet_tok', 'low'): 1.50e-05, ('dpet_tok', 'high'): 3.38e-05, ('dpet_tok.reserved', 'flat'): 5.16e-06, ('dpet_tok.reserved', 'peaked'): 6.91e-06, ('dpet_tok.reserved', 'low'): 6.68e-06, ('dpet_tok.reserved', 'high'): 2.81e-06, ('i2.dwq', 'rows'): 2.13e-06, ('i2.dwkv', 'rows'): 4.68e-06, ('i2.dwo', 'rows'): 9.25e-06, ('i2.dw1', 'rows'): 1.69e-05, ('i2.dw2', 'rows'): 9.35e-06, ('i2.small', 'b2'): 6.14e-07, ('i2.small', 'b2.reserved'): 5.80e-07, ('i2.small', 'b1'): 1.24e-06, ('i2.small', 'bo'): 5.54e-07, ('i2.small', 'bo.reserved'): 8.13e-07, ('i2.small', 'ln2_g'): 1.47e-06, ('i2.small', 'ln2_g.reserved'): 1.85e-06, ('i2.small', 'ln2_b'): 9.62e-07, ('i2.small', 'ln2_b.reserved'): 1.25e-06, ('i2.small', 'ln1_g'): 1.18e-07, ('i2.small', 'ln1_g.reserved'): 4.46e-08, ('i2.small', 'ln1_b'): 9.16e-08, ('i2.small', 'ln1_b.reserved'): 5.42e-08, ('i2.lnf', 'lnf_g'): 1.03e-06, ('i2.lnf', 'lnf_g.reserved'): 3.24e-07, ('i2.lnf', 'lnf_b'): 5.48e-07, ('i2.lnf', 'lnf_b.reserved'): 4.38e-07, ('i3.dwq', 'rows'): 1.19e-06, ('i3.dwkv', 'rows'): 4.24e-06, ('i3.dwo', 'rows'): 9.22e-06, ('i3.dw1', 'rows'): 1.64e-05, ('i3.dw2', 'rows'): 8.50e-06, ('i3.small', 'b2'): 4.45e-07, ('i3.small', 'b2.reserved'): 3.52e-07, ('i3.small', 'b1'): 1.69e-06, ('i3.small', 'bo'): 6.28e-07, ('i3.small', 'bo.reserved'): 3.44e-07, ('i3.small', 'ln2_g'): 2.06e-06, ('i3.small', 'ln2_g.reserved'): 1.04e-06, ('i3.small', 'ln2_b'): 1.12e-06, ('i3.small', 'ln2_b.reserved'): 6.69e-07, ('i3.small', 'ln1_g'): 9.49e-08, ('i3.small', 'ln1_g.reserved'): 8.62e-08, ('i3.small', 'ln1_b'): 9.65e-08, ('i3.small', 'ln1_b.reserved'): 3.99e-08, ('i3.lnf', 'lnf_g'): 1.97e-06, ('i3.lnf', 'lnf_g.reserved'): 7.13e-07, ('i3.lnf', 'lnf_b'): 3.47e-07, ('i3.lnf', 'lnf_b.reserved'): 2.05e-07, ('i0.dwq', 'rows'): 3.58e-06, ('i0.dwkv', 'rows'): 1.29e-05, ('i0.dwo', 'rows'): 2.71e-05, ('i0.dw1', 'rows'): 3.46e-05, ('i0.dw2', 'rows'): 1.56e-05, ('i0.small', 'b2'): 2.44e-06, ('i0.small', 'b2.reserved'): 1.56e-06, ('i0.small', 'b1'): 2.25e-06, ('i0.small', 'bo'): 2.39e-06, ('i0.small', 'bo.reserved'): 2.03e-06, ('i0.small', 'ln2_g'): 1.99e-06, ('i0.small', 'ln2_g.reserved'): 3.38e-06, ('i0.small', 'ln2_b'): 1.68e-06, ('i0.small', 'ln2_b.reserved'): 2.01e-06, ('i0.small', 'ln1_g'): 1.43e-07, ('i0.small', 'ln1_g.reserved'): 8.02e-07, ('i0.small', 'ln1_b'): 1.70e-07, ('i0.small', 'ln1_b.reserved'): 1.90e-07, ('i0.lnf', 'lnf_g'): 2.13e-07, ('i0.lnf', 'lnf_g.reserved'): 4.54e-07, ('i0.lnf', 'lnf_b'): 1.85e-07, ('i0.lnf', 'lnf_b.reserved'): 3.71e-07, ('i1.dwq', 'rows'): 3.12e-06, ('i1.dwkv', 'rows'): 1.11e-05, ('i1.dwo', 'rows'): 1.56e-05, ('i1.dw1', 'rows'): 2.80e-05, ('i1.dw2', 'rows'): 1.16e-05, ('i1.small', 'b2'): 1.29e-06, ('i1.small', 'b2.reserved'): 9.38e-07, ('i1.small', 'b1'): 1.86e-06, ('i1.small', 'bo'): 1.36e-06, ('i1.small', 'bo.reserved'): 1.46e-06, ('i1.small', 'ln2_g'): 3.14e-06, ('i1.small', 'ln2_g.reserved'): 1.80e-06, ('i1.small', 'ln2_b'): 1.81e-06, ('i1.small', 'ln2_b.reserved'): 1.81e-06, ('i1.small', 'ln1_g'): 2.20e-07, ('i1.small', 'ln1_g.reserved'): 4.90e-07, ('i1.small', 'ln1_b'): 1.67e-07, ('i1.small', 'ln1_b.reserved'): 2.34e-07, ('i1.lnf', 'lnf_g'): 2.18e-06, ('i1.lnf', 'lnf_g.reserved'): 1.12e-06, ('i1.lnf', 'lnf_b'): 1.38e-06, ('i1.lnf', 'lnf_b.reserved'): 7.11e-07},
    ((2, 17, 2, False), 8): {('cls', 'mean'): 9.61e-07, ('cls', 'max'): 5.81e-07, ('dmri_tok', 'flat'): 2.45e-06, ('dmri_tok', 'peaked'): 1.48e-06, ('dmri_tok', 'low'): 4.98e-06, ('dmri_tok', 'high'): 7.59e-06, ('dmri_tok.reserved', 'flat'): 1.35e-06, ('dmri_tok.reserved', 'peaked'): 2.38e-06, ('dmri_tok.reserved', 'low'): 1.73e-06, ('dmri_tok.reserved', 'high'): 1.66e-06, ('dpet_tok', 'flat'): 1.54e-06, ('dpet_tok', 'peaked'): 2.33e-06, ('dpet_tok', 'low'): 5.99e-06, ('dpet_tok', 'high'): 1.37e-05, ('dpet_tok.reserved', 'flat'): 1.98e-06, ('dpet_tok.reserved', 'peaked'): 2.29e-06, ('dpet_tok.reserved', 'low'): 1.53e-06, ('dpet_tok.reserved', 'high'): 1.22e-06, ('i2.dwq', 'rows'): 8.74e-07, ('i2.dwkv', 'rows'): 2.61e-06, ('i2.dwo', 'rows'): 5.02e-06, ('i2.dw1', 'rows'): 7.61e-06, ('i2.dw2', 'rows'): 3.61e-06, ('i2.small', 'b2'): 3.37e-07, ('i2.small', 'b2.reserved'): 3.85e-07, ('i2.small', 'b1'): 5.51e-07, ('i2.small', 'bo'): 3.54e-07, ('i2.small', 'bo.reserved'): 4.32e-07, ('i2.small', 'ln2_g'): 1.01e-06, ('i2.small', 'ln2_g.reserved'): 7.93e-07, ('i2.small', 'ln2_b'): 5.22e-07, ('i2.small', 'ln2_b.reserved'): 4.64e-07, ('i2.small', 'ln1_g'): 6.04e-08, ('i2.small', 'ln1_g.reserved'): 2.81e-08, ('i2.small', 'ln1_b'): 4.81e-08, ('i2.small', 'ln1_b.reserved'): 2.32e-08, ('i2.lnf', 'lnf_g'): 8.83e-07, ('i2.lnf', 'lnf_g.reserved'): 6.74e-07, ('i2.lnf', 'lnf_b'): 3.41e-07, ('i2.lnf', 'lnf_b.reserved'): 4.08e-07, ('i3.dwq', 'rows'): 8.21e-07, ('i3.dwkv', 'rows'): 2.80e-06, ('i3.dwo', 'rows'): 1.08e-05, ('i3.dw1', 'rows'): 9.72e-06, ('i3.dw2', 'rows'): 4.75e-06, ('i3.small', 'b2'): 2.57e-07, ('i3.small', 'b2.reserved'): 2.94e-07, ('i3.small', 'b1'): 7.79e-07, ('i3.small', 'bo'): 3.23e-07, ('i3.small', 'bo.reserved'): 4.09e-07, ('i3.small', 'ln2_g'): 1.30e-06, ('i3.small', 'ln2_g.reserved'): 9.09e-07, ('i3.small', 'ln2_b'): 5.87e-07, ('i3.small', 'ln2_b.reserved'): 7.32e-07, ('i3.small', 'ln1_g'): 3.96e-08, ('i3.small', 'ln1_g.reserved'): 3.32e-08, ('i3.small', 'ln1_b'): 3.45e-08, ('i3.small', 'ln1_b.reserved'): 3.55e-08, ('i3.lnf', 'lnf_g'): 1.51e-06, ('i3.lnf', 'lnf_g.reserved'): 8.39e-07, ('i3.lnf', 'lnf_b'): 2.44e-07, ('i3.lnf', 'lnf_b.reserved'): 5.16e-07, ('i0.dwq', 'rows'): 3.11e-06, ('i0.dwkv', 'rows'): 7.83e-06, ('i0.dwo', 'rows'): 1.36e-05, ('i0.dw1', 'rows'): 1.79e-05, ('i0.dw2', 'rows'): 8.54e-06, ('i0.small', 'b2'): 1.18e-06, ('i0.small', 'b2.reserved'): 7.05e-07, ('i0.small', 'b1'): 1.18e-06, ('i0.small', 'bo'): 1.26e-06, ('i0.small', 'bo.reserved'): 1.02e-06, ('i0.small', 'ln2_g'): 1.52e-06, ('i0.small', 'ln2_g.reserved'): 1.35e-06, ('i0.small', 'ln2_b'): 1.27e-06, ('i0.small', 'ln2_b.reserved'): 1.03e-06, ('i0.small', 'ln1_g'): 1.21e-07, ('i0.small', 'ln1_g.reserved'): 1.97e-07, ('i0.small', 'ln1_b'): 9.79e-08, ('i0.small', 'ln1_b.reserved'): 8.74e-08, ('i0.lnf', 'lnf_g'): 1.20e-07, ('i0.lnf', 'lnf_g.reserved'): 2.07e-07, ('i0.lnf', 'lnf_b'): 1.04e-07, ('i0.lnf', 'lnf_b.reserved'): 1.61e-07, ('i1.dwq', 'rows'): 3.36e-06, ('i1.dwkv', 'rows'): 7.79e-06, ('i1.dwo', 'rows'): 1.25e-05, ('i1.dw1', 'rows'): 2.25e-05, ('i1.dw2', 'rows'): 6.71e-06, ('i1.small', 'b2'): 6.27e-07, ('i1.small', 'b2.reserved'): 7.21e-07, ('i1.small', 'b1'): 9.46e-07, ('i1.small', 'bo'): 6.08e-07, ('i1.small', 'bo.reserved'): 7.15e-07, ('i1.small', 'ln2_g'): 1.81e-06, ('i1.small', 'ln2_g.reserved'): 4.54e-07, ('i1.small', 'ln2_b'): 9.11e-07, ('i1.small', 'ln2_b.reserved'): 5.94e-07, ('i1.small', 'ln1_g'): 1.01e-07, ('i1.small', 'ln1_g.reserved'): 1.66e-07, ('i1.small', 'ln1_b'): 9.57e-08, ('i1.small', 'ln1_b.reserved'): 1.82e-07, ('i1.lnf', 'lnf_g'): 1.77e-06, ('i1.lnf', 'lnf_g.reserved'): 1.69e-06, ('i1.lnf', 'lnf_b'): 6.22e-07, ('i1.lnf', 'lnf_b.reserved'): 5.85e-07},
    ((2, 33, 1, True), 4): {('cls', 'mean'): 1.77e-06, ('cls', 'max'): 2.74e-06, ('dmri_tok', 'flat'): 4.30e-06, ('dmri_tok', 'peaked'): 1.07e-05, ('dmri_tok', 'low'): 1.53e-05, ('dmri_tok', 'high'): 1.76e-05, ('dmri_tok.reserved', 'flat'): 4.67e-06, ('dmri_tok.reserved', 'peaked'): 4.48e-06, ('dmri_tok.reserved', 'low'): 5.28e-06, ('dmri_tok.reserved', 'high'): 5.78e-06, ('dpet_tok', 'flat'): 3.08e-06, ('dpet_tok', 'peaked'): 8.75e-06, ('dpet_tok', 'low'): 1.40e-05, ('dpet_tok', 'high'): 5.10e-05, ('dpet_tok.reserved', 'flat'): 4.06e-06, ('dpet_tok.reserved', 'peaked'): 6.14e-06, ('dpet_tok.reserved', 'low'): 7.82e-06, ('dpet_tok.reserved', 'high'): 4.59e-06, ('i0.dwq', 'rows'): 2.83e-06, ('i0.dwkv', 'rows'): 8.98e-06, ('i0.dwo', 'rows'): 2.12e-05, ('i0.dw1', 'rows'): 4.16e-05, ('i0.dw2', 'rows'): 2.20e-05, ('i0.small', 'b2'): 2.22e-06, ('i0.small', 'b2.reserved'): 2.24e-06, ('i0.small', 'b1'): 2.36e-06, ('i0.small', 'bo'): 2.07e-06, ('i0.small', 'bo.reserved'): 1.65e-06, ('i0.small', 'ln2_g'): 2.31e-06, ('i0.small', 'ln2_g.reserved'): 1.83e-06, ('i0.small', 'ln2_b'): 1.73e-06, ('i0.small', 'ln2_b.reserved'): 1.52e-06, ('i0.small', 'ln1_g'): 1.10e-07, ('i0.small', 'ln1_g.reserved'): 7.50e-07, ('i0.small', 'ln1_b'): 9.33e-08, ('i0.small', 'ln1_b.reserved'): 1.73e-07, ('i0.lnf', 'lnf_g'): 1.45e-07, ('i0.lnf', 'lnf_g.reserved'): 4.36e-07, ('i0.lnf', 'lnf_b'): 1.80e-07, ('i0.lnf', 'lnf_b.reserved'): 3.89e-07, ('i1.dwq', 'rows'): 2.64e-06, ('i1.dwkv', 'rows'): 7.93e-06, ('i1.dwo', 'rows'): 2.58e-05, ('i1.dw1', 'rows'): 3.42e-05, ('i1.dw2', 'rows'): 1.81e-05, ('i1.small', 'b2'): 1.04e-06, ('i1.small', 'b2.reserved'): 4.79e-07, ('i1.small', 'b1'): 2.93e-06, ('i1.small', 'bo'): 1.91e-06, ('i1.small', 'bo.reserved'): 1.32e-06, ('i1.small', 'ln2_g'): 3.41e-06, ('i1.small', 'ln2_g.reserved'): 1.03e-06, ('i1.small', 'ln2_b'): 1.57e-06, ('i1.small', 'ln2_b.reserved'): 1.15e-06, ('i1.small', 'ln1_g'): 1.60e-07, ('i1.small', 'ln1_g.reserved'): 4.93e-07, ('i1.small', 'ln1_b'): 1.56e-07, ('i1.small', 'ln1_b.reserved'): 2.19e-07, ('i1.lnf', 'lnf_g'): 4.42e-06, ('i1.lnf', 'lnf_g.reserved'): 4.44e-07, ('i1.lnf', 'lnf_b'): 8.11e-07, ('i1.lnf', 'lnf_b.reserved'): 2.27e-07},
    ((2, 33, 1, True), 8): {('cls', 'mean'): 8.76e-07, ('cls', 'max'): 1.10e-06, ('dmri_tok', 'flat'): 2.94e-06, ('dmri_tok', 'peaked'): 4.11e-06, ('dmri_tok', 'low'): 9.58e-06, ('dmri_tok', 'high'): 5.71e-06, ('dmri_tok.reserved', 'flat'): 2.70e-06, ('dmri_tok.reserved', 'peaked'): 2.47e-06, ('dmri_tok.reserved', 'low'): 1.81e-06, ('dmri_tok.reserved', 'high'): 1.36e-06, ('dpet_tok', 'flat'): 2.22e-06, ('dpet_tok', 'peaked'): 3.46e-06, ('dpet_tok', 'low'): 1.09e-05, ('dpet_tok', 'high'): 1.21e-05, ('dpet_tok.reserved', 'flat'): 1.37e-06, ('dpet_tok.reserved', 'peaked'): 1.93e-06, ('dpet_tok.reserved', 'low'): 1.82e-06, ('dpet_tok.reserved', 'high'): 2.26e-06, ('i0.dwq', 'rows'): 1.63e-06, ('i0.dwkv', 'rows'): 7.36e-06, ('i0.dwo', 'rows'): 1.38e-05, ('i0.dw1', 'rows'): 1.78e-05, ('i0.dw2', 'rows'): 1.03e-05, ('i0.small', 'b2'): 1.46e-06, ('i0.small', 'b2.reserved'): 6.27e-07, ('i0.small', 'b1'): 1.30e-06, ('i0.small', 'bo'): 1.04e-06, ('i0.small', 'bo.reserved'): 5.46e-07, ('i0.small', 'ln2_g'): 1.61e-06, ('i0.small', 'ln2_g.reserved'): 6.36e-07, ('i0.small', 'ln2_b'): 8.38e-07, ('i0.small', 'ln2_b.reserved'): 6.65e-07, ('i0.small', 'ln1_g'): 5.42e-08, ('i0.small', 'ln1_g.reserved'): 1.25e-07, ('i0.small', 'ln1_b'): 5.54e-08, ('i0.small', 'ln1_b.reserved'): 5.12e-08, ('i0.lnf', 'lnf_g'): 1.25e-07, ('i0.lnf', 'lnf_g.reserved'): 1.88e-07, ('i0.lnf', 'lnf_b'): 9.65e-08, ('i0.lnf', 'lnf_b.reserved'): 1.11e-07, ('i1.dwq', 'rows'): 1.46e-06, ('i1.dwkv', 'rows'): 4.36e-06, ('i1.dwo', 'rows'): 1.02e-05, ('i1.dw1', 'rows'): 1.36e-05, ('i1.dw2', 'rows'): 6.00e-06, ('i1.small', 'b2'): 5.57e-07, ('i1.small', 'b2.reserved'): 3.02e-07, ('i1.small', 'b1'): 1.00e-06, ('i1.small', 'bo'): 7.62e-07, ('i1.small', 'bo.reserved'): 7.36e-07, ('i1.small', 'ln2_g'): 1.40e-06, ('i1.small', 'ln2_g.reserved'): 7.29e-07, ('i1.small', 'ln2_b'): 9.47e-07, ('i1.small', 'ln2_b.reserved'): 8.30e-07, ('i1.small', 'ln1_g'): 8.37e-08, ('i1.small', 'ln1_g.reserved'): 1.82e-07, ('i1.small', 'ln1_b'): 6.88e-08, ('i1.small', 'ln1_b.reserved'): 1.09e-07, ('i1.lnf', 'lnf_g'): 1.64e-06, ('i1.lnf', 'lnf_g.reserved'): 4.08e-07, ('i1.lnf', 'lnf_b'): 8.00e-07, ('i1.lnf', 'lnf_b.reserved'): 1.53e-07},
    ((9, 40, 1, False), 4): {('cls', 'mean'): 1.63e-06, ('cls', 'max'): 2.22e-06, ('dmri_tok', 'flat'): 1.77e-05, ('dmri_tok', 'peaked'): 1.28e-05, ('dmri_tok', 'low'): 2.73e-05, ('dmri_tok', 'high'): 2.29e-05, ('dmri_tok.reserved', 'flat'): 1.20e-05, ('dmri_tok.reserved', 'peaked'): 6.96e-06, ('dmri_tok.reserved', 'low'): 8.82e-06, ('dmri_tok.reserved', 'high'): 6.68e-06, ('dpet_tok', 'flat'): 8.85e-06, ('dpet_tok', 'peaked'): 2.08e-05, ('dpet_tok', 'low'): 2.53e-05, ('dpet_tok', 'high'): 3.16e-05, ('dpet_tok.reserved', 'flat'): 6.00e-06, ('dpet_tok.reserved', 'peaked'): 5.37e-06, ('dpet_tok.reserved', 'low'): 6.04e-06, ('dpet_tok.reserved', 'high'): 4.72e-06, ('i0.dwq', 'rows'): 9.09e-07, ('i0.dwkv', 'rows'): 2.90e-06, ('i0.dwo', 'rows'): 1.90e-05, ('i0.dw1', 'rows'): 2.65e-05, ('i0.dw2', 'rows'): 1.13e-05, ('i0.small', 'b2'): 1.33e-06, ('i0.small', 'b2.reserved'): 8.84e-07, ('i0.small', 'b1'): 7.82e-07, ('i0.small', 'bo'): 8.68e-07, ('i0.small', 'bo.reserved'): 5.09e-07, ('i0.small', 'ln2_g'): 1.16e-06, ('i0.small', 'ln2_g.reserved'): 7.28e-07, ('i0.small', 'ln2_b'): 7.97e-07, ('i0.small', 'ln2_b.reserved'): 4.64e-07, ('i0.small', 'ln1_g'): 4.58e-08, ('i0.small', 'ln1_g.reserved'): 1.32e-07, ('i0.small', 'ln1_b'): 5.15e-08, ('i0.small', 'ln1_b.reserved'): 6.01e-08, ('i0.lnf', 'lnf_g'): 5.75e-08, ('i0.lnf', 'lnf_g.reserved'): 1.28e-07, ('i0.lnf', 'lnf_b'): 5.89e-08, ('i0.lnf', 'lnf_b.reserved'): 1.29e-07, ('i1.dwq', 'rows'): 8.81e-07, ('i1.dwkv', 'rows'): 2.12e-06, ('i1.dwo', 'rows'): 2.39e-05, ('i1.dw1', 'rows'): 2.95e-05, ('i1.dw2', 'rows'): 1.62e-05, ('i1.small', 'b2'): 4.21e-07, ('i1.small', 'b2.reserved'): 2.83e-07, ('i1.small', 'b1'): 7.46e-07, ('i1.small', 'bo'): 5.88e-07, ('i1.small', 'bo.reserved'): 2.85e-07, ('i1.small', 'ln2_g'): 1.34e-06, ('i1.small', 'ln2_g.reserved'): 1.19e-06, ('i1.small', 'ln2_b'): 6.54e-07, ('i1.small', 'ln2_b.reserved'): 2.50e-07, ('i1.small', 'ln1_g'): 7.93e-08, ('i1.small', 'ln1_g.reserved'): 1.74e-07, ('i1.small', 'ln1_b'): 4.54e-08, ('i1.small', 'ln1_b.reserved'): 1.68e-07, ('i1.lnf', 'lnf_g'): 2.29e-06, ('i1.lnf', 'lnf_g.reserved'): 4.23e-07, ('i1.lnf', 'lnf_b'): 1.64e-06, ('i1.lnf', 'lnf_b.reserved'): 7.60e-07},
    ((9, 40, 1, False), 8): {('cls', 'mean'): 9.75e-07, ('cls', 'max'): 8.92e-07, ('dmri_tok', 'flat'): 8.44e-06, ('dmri_tok', 'peaked'): 8.69e-06, ('dmri_tok', 'low'): 1.87e-05, ('dmri_tok', 'high'): 1.73e-05, ('dmri_tok.reserved', 'flat'): 3.41e-06, ('dmri_tok.reserved', 'peaked'): 1.84e-06, ('dmri_tok.reserved', 'low'): 3.21e-06, ('dmri_tok.reserved', 'high'): 3.83e-06, ('dpet_tok', 'flat'): 4.55e-06, ('dpet_tok', 'peaked'): 7.63e-06, ('dpet_tok', 'low'): 1.45e-05, ('dpet_tok', 'high'): 2.34e-05, ('dpet_tok.reserved', 'flat'): 1.88e-06, ('dpet_tok.reserved', 'peaked'): 1.96e-06, ('dpet_tok.reserved', 'low'): 1.83e-06, ('dpet_tok.reserved', 'high'): 2.26e-06, ('i0.dwq', 'rows'): 5.51e-07, ('i0.dwkv', 'rows'): 1.96e-06, ('i0.dwo', 'rows'): 9.79e-06, ('i0.dw1', 'rows'): 1.83e-05, ('i0.dw2', 'rows'): 6.61e-06, ('i0.small', 'b2'): 1.00e-06, ('i0.small', 'b2.reserved'): 3.27e-07, ('i0.small', 'b1'): 6.88e-07, ('i0.small', 'bo'): 5.72e-07, ('i0.small', 'bo.reserved'): 3.89e-07, ('i0.small', 'ln2_g'): 4.29e-07, ('i0.small', 'ln2_g.reserved'): 2.59e-07, ('i0.small', 'ln2_b'): 6.57e-07, ('i0.small', 'ln2_b.reserved'): 4.90e-07, ('i0.small', 'ln1_g'): 4.73e-08, ('i0.small', 'ln1_g.reserved'): 9.02e-08, ('i0.small', 'ln1_b'): 3.04e-08, ('i0.small', 'ln1_b.reserved'): 2.65e-08, ('i0.lnf', 'lnf_g'): 4.34e-08, ('i0.lnf', 'lnf_g.reserved'): 5.16e-08, ('i0.lnf', 'lnf_b'): 5.11e-08, ('i0.lnf', 'lnf_b.reserved'): 4.62e-08, ('i1.dwq', 'rows'): 4.78e-07, ('i1.dwkv', 'rows'): 1.96e-06, ('i1.dwo', 'rows'): 7.10e-06, ('i1.dw1', 'rows'): 1.42e-05, ('i1.dw2', 'rows'): 6.26e-06, ('i1.small', 'b2'): 2.67e-07, ('i1.small', 'b2.reserved'): 1.52e-07, ('i1.small', 'b1'): 3.92e-07, ('i1.small', 'bo'): 3.11e-07, ('i1.small', 'bo.reserved'): 2.72e-07, ('i1.small', 'ln2_g'): 8.31e-07, ('i1.small', 'ln2_g.reserved'): 2.48e-07, ('i1.small', 'ln2_b'): 3.79e-07, ('i1.small', 'ln2_b.reserved'): 2.96e-07, ('i1.small', 'ln1_g'): 3.82e-08, ('i1.small', 'ln1_g.reserved'): 6.40e-08, ('i1.small', 'ln1_b'): 2.76e-08, ('i1.small', 'ln1_b.reserved'): 3.10e-08, ('i1.lnf', 'lnf_g'): 8.90e-07, ('i1.lnf', 'lnf_g.reserved'): 1.28e-07, ('i1.lnf', 'lnf_b'): 1.53e-06, ('i1.lnf', 'lnf_b.reserved'): 7.00e-07},
    ((17, 20, 1, True), 4): {('cls', 'mean'): 2.58e-06, ('cls', 'max'): 2.34e-06, ('dmri_tok', 'flat'): 7.52e-06, ('dmri_tok', 'peaked'): 1.65e-05, ('dmri_tok', 'low'): 3.53e-05, ('dmri_tok', 'high'): 4.07e-05, ('dmri_tok.reserved', 'flat'): 9.77e-06, ('dmri_tok.reserved', 'peaked'): 9.45e-06, ('dmri_tok.reserved', 'low'): 9.53e-06, ('dmri_tok.reserved', 'high'): 6.92e-06, ('dpet_tok', 'flat'): 7.02e-06, ('dpet_tok', 'peaked'): 1.58e-05, ('dpet_tok', 'low'): 2.79e-05, ('dpet_tok', 'high'): 2.39e-05, ('dpet_tok.reserved', 'flat'): 5.65e-06, ('dpet_tok.reserved', 'peaked'): 6.50e-06, ('dpet_tok.reserved', 'low'): 5.71e-06, ('dpet_tok.reserved', 'high'): 6.01e-06, ('i0.dwq', 'rows'): 1.05e-06, ('i0.dwkv', 'rows'): 2.63e-06, ('i0.dwo', 'rows'): 1.79e-05, ('i0.dw1', 'rows'): 3.42e-05, ('i0.dw2', 'rows'): 1.23e-05, ('i0.small', 'b2'): 1.26e-06, ('i0.small', 'b2.reserved'): 6.03e-07, ('i0.small', 'b1'): 1.04e-06, ('i0.small', 'bo'): 1.21e-06, ('i0.small', 'bo.reserved'): 5.88e-07, ('i0.small', 'ln2_g'): 1.29e-06, ('i0.small', 'ln2_g.reserved'): 1.49e-06, ('i0.small', 'ln2_b'): 9.51e-07, ('i0.small', 'ln2_b.reserved'): 5.59e-07, ('i0.small', 'ln1_g'): 5.37e-08, ('i0.small', 'ln1_g.reserved'): 2.23e-07, ('i0.small', 'ln1_b'): 4.65e-08, ('i0.small', 'ln1_b.reserved'): 1.17e-07, ('i0.lnf', 'lnf_g'): 7.18e-08, ('i0.lnf', 'lnf_g.reserved'): 1.74e-07, ('i0.lnf', 'lnf_b'): 7.17e-08, ('i0.lnf', 'lnf_b.reserved'): 1.40e-07, ('i1.dwq', 'rows'): 1.16e-06, ('i1.dwkv', 'rows'): 2.41e-06, ('i1.dwo', 'rows'): 1.78e-05, ('i1.dw1', 'rows'): 4.21e-05, ('i1.dw2', 'rows'): 1.34e-05, ('i1.small', 'b2'): 5.00e-07, ('i1.small', 'b2.reserved'): 3.01e-07, ('i1.small', 'b1'): 1.13e-06, ('i1.small', 'bo'): 7.11e-07, ('i1.small', 'bo.reserved'): 7.32e-07, ('i1.small', 'ln2_g'): 1.61e-06, ('i1.small', 'ln2_g.reserved'): 7.66e-07, ('i1.small', 'ln2_b'): 8.37e-07, ('i1.small', 'ln2_b.reserved'): 3.86e-07, ('i1.small', 'ln1_g'): 8.31e-08, ('i1.small', 'ln1_g.reserved'): 1.74e-07, ('i1.small', 'ln1_b'): 5.79e-08, ('i1.small', 'ln1_b.reserved'): 8.65e-08, ('i1.lnf', 'lnf_g'): 1.99e-06, ('i1.lnf', 'lnf_g.reserved'): 3.62e-07, ('i1.lnf', 'lnf_b'): 6.37e-07, ('i1.lnf', 'lnf_b.reserved'): 5.86e-07},
    ((17, 20, 1, True), 8): {('cls', 'mean'): 1.85e-06, ('cls', 'max'): 1.09e-06, ('dmri_tok', 'flat'): 4.76e-06, ('dmri_tok', 'peaked'): 6.98e-06, ('dmri_tok', 'low'): 1.22e-05, ('dmri_tok', 'high'): 2.02e-05, ('dmri_tok.reserved', 'flat'): 3.03e-06, ('dmri_tok.reserved', 'peaked'): 3.67e-06, ('dmri_tok.reserved', 'low'): 4.45e-06, ('dmri_tok.reserved', 'high'): 2.98e-06, ('dpet_tok', 'flat'): 4.73e-06, ('dpet_tok', 'peaked'): 3.33e-06, ('dpet_tok', 'low'): 1.92e-05, ('dpet_tok', 'high'): 1.68e-05, ('dpet_tok.reserved', 'flat'): 2.63e-06, ('dpet_tok.reserved', 'peaked'): 2.37e-06, ('dpet_tok.reserved', 'low'): 3.38e-06, ('dpet_tok.reserved', 'high'): 2.70e-06, ('i0.dwq', 'rows'): 5.15e-07, ('i0.dwkv', 'rows'): 1.37e-06, ('i0.dwo', 'rows'): 8.89e-06, ('i0.dw1', 'rows'): 2.38e-05, ('i0.dw2', 'rows'): 7.15e-06, ('i0.small', 'b2'): 7.79e-07, ('i0.small', 'b2.reserved'): 7.08e-07, ('i0.small', 'b1'): 6.13e-07, ('i0.small', 'bo'): 8.46e-07, ('i0.small', 'bo.reserved'): 5.91e-07, ('i0.small', 'ln2_g'): 8.13e-07, ('i0.small', 'ln2_g.reserved'): 4.16e-07, ('i0.small', 'ln2_b'): 5.34e-07, ('i0.small', 'ln2_b.reserved'): 4.07e-07, ('i0.small', 'ln1_g'): 3.88e-08, ('i0.small', 'ln1_g.reserved'): 6.35e-08, ('i0.small', 'ln1_b'): 3.56e-08, ('i0.small', 'ln1_b.reserved'): 3.67e-08, ('i0.lnf', 'lnf_g'): 5.81e-08, ('i0.lnf', 'lnf_g.reserved'): 6.78e-08, ('i0.lnf', 'lnf_b'): 4.34e-08, ('i0.lnf', 'lnf_b.reserved'): 5.75e-08, ('i1.dwq', 'rows'): 6.52e-07, ('i1.dwkv', 'rows'): 2.40e-06, ('i1.dwo', 'rows'): 7.41e-06, ('i1.dw1', 'rows'): 1.41e-05, ('i1.dw2', 'rows'): 6.01e-06, ('i1.small', 'b2'): 2.38e-07, ('i1.small', 'b2.reserved'): 3.42e-07, ('i1.small', 'b1'): 5.78e-07, ('i1.small', 'bo'): 4.40e-07, ('i1.small', 'bo.reserved'): 3.20e-07, ('i1.small', 'ln2_g'): 8.80e-07, ('i1.small', 'ln2_g.reserved'): 2.99e-07, ('i1.small', 'ln2_b'): 4.15e-07, ('i1.small', 'ln2_b.reserved'): 4.22e-07, ('i1.small', 'ln1_g'): 4.35e-08, ('i1.small', 'ln1_g.reserved'): 5.93e-08, ('i1.small', 'ln1_b'): 3.05e-08, ('i1.small', 'ln1_b.reserved'): 3.00e-08, ('i1.lnf', 'lnf_g'): 7.00e-07, ('i1.lnf', 'lnf_g.reserved'): 4.73e-07, ('i1.lnf', 'lnf_b'): 4.08e-07, ('i1.lnf', 'lnf_b.reserved'): 6.89e-07},
    ((1, 128, 1, False), 4): {('cls', 'mean'): 9.50e-07, ('cls', 'max'): 8.63e-07, ('dmri_tok', 'flat'): 2.00e-05, ('dmri_tok', 'peaked'): 2.43e-05, ('dmri_tok', 'low'): 2.32e-05, ('dmri_tok', 'high'): 2.68e-05, ('dmri_tok.reserved', 'flat'): 8.06e-06, ('dmri_tok.reserved', 'peaked'): 5.51e-06, ('dmri_tok.reserved', 'low'): 5.07e-06, ('dmri_tok.reserved', 'high'): 4.23e-06, ('dpet_tok', 'flat'): 1.01e-05, ('dpet_tok', 'peaked'): 2.07e-05, ('dpet_tok', 'low'): 1.26e-05, ('dpet_tok', 'high'): 1.97e-05, ('dpet_tok.reserved', 'flat'): 3.97e-06, ('dpet_tok.reserved', 'peaked'): 5.20e-06, ('dpet_tok.reserved', 'low'): 2.74e-06, ('dpet_tok.reserved', 'high'): 4.69e-06, ('i0.dwq', 'rows'): 1.07e-06, ('i0.dwkv', 'rows'): 8.87e-06, ('i0.dwo', 'rows'): 2.75e-05, ('i0.dw1', 'rows'): 2.42e-05, ('i0.dw2', 'rows'): 1.14e-05, ('i0.small', 'b2'): 2.06e-06, ('i0.small', 'b2.reserved'): 1.08e-06, ('i0.small', 'b1'): 1.29e-06, ('i0.small', 'bo'): 1.50e-06, ('i0.small', 'bo.reserved'): 6.98e-07, ('i0.small', 'ln2_g'): 1.42e-06, ('i0.small', 'ln2_g.reserved'): 6.44e-07, ('i0.small', 'ln2_b'): 1.17e-06, ('i0.small', 'ln2_b.reserved'): 8.80e-07, ('i0.small', 'ln1_g'): 7.38e-08, ('i0.small', 'ln1_g.reserved'): 2.63e-07, ('i0.small', 'ln1_b'): 5.67e-08, ('i0.small', 'ln1_b.reserved'): 9.80e-08, ('i0.lnf', 'lnf_g'): 1.19e-07, ('i0.lnf', 'lnf_g.reserved'): 2.48e-07, ('i0.lnf', 'lnf_b'): 1.28e-07, ('i0.lnf', 'lnf_b.reserved'): 2.46e-07, ('i1.dwq', 'rows'): 1.44e-06, ('i1.dwkv', 'rows'): 5.36e-06, ('i1.dwo', 'rows'): 1.80e-05, ('i1.dw1', 'rows'): 2.46e-05, ('i1.dw2', 'rows'): 1.13e-05, ('i1.small', 'b2'): 6.31e-07, ('i1.small', 'b2.reserved'): 5.58e-07, ('i1.small', 'b1'): 1.31e-06, ('i1.small', 'bo'): 9.44e-07, ('i1.small', 'bo.reserved'): 1.14e-06, ('i1.small', 'ln2_g'): 1.89e-06, ('i1.small', 'ln2_g.reserved'): 6.87e-07, ('i1.small', 'ln2_b'): 1.18e-06, ('i1.small', 'ln2_b.reserved'): 9.25e-07, ('i1.small', 'ln1_g'): 9.50e-08, ('i1.small', 'ln1_g.reserved'): 2.84e-07, ('i1.small', 'ln1_b'): 8.00e-08, ('i1.small', 'ln1_b.reserved'): 1.38e-07, ('i1.lnf', 'lnf_g'): 2.66e-06, ('i1.lnf', 'lnf_g.reserved'): 1.70e-06, ('i1.lnf', 'lnf_b'): 1.25e-06, ('i1.lnf', 'lnf_b.reserved'): 2.21e-06},
    ((1, 128, 1, False), 8): {('cls', 'mean'): 6.99e-07, ('cls', 'max'): 4.18e-07, ('dmri_tok', 'flat'): 7.52e-06, ('dmri_tok', 'peaked'): 1.10e-05, ('dmri_tok', 'low'): 9.08e-06, ('dmri_tok', 'high'): 1.18e-05, ('dmri_tok.reserved', 'flat'): 2.51e-06, ('dmri_tok.reserved', 'peaked'): 1.68e-06, ('dmri_tok.reserved', 'low'): 2.03e-06, ('dmri_tok.reserved', 'high'): 1.59e-06, ('dpet_tok', 'flat'): 3.33e-06, ('dpet_tok', 'peaked'): 6.06e-06, ('dpet_tok', 'low'): 1.12e-05, ('dpet_tok', 'high'): 8.20e-06, ('dpet_tok.reserved', 'flat'): 1.35e-06, ('dpet_tok.reserved', 'peaked'): 1.36e-06, ('dpet_tok.reserved', 'low'): 1.26e-06, ('dpet_tok.reserved', 'high'): 1.80e-06, ('i0.dwq', 'rows'): 5.30e-07, ('i0.dwkv', 'rows'): 5.94e-06, ('i0.dwo', 'rows'): 1.12e-05, ('i0.dw1', 'rows'): 1.38e-05, ('i0.dw2', 'rows'): 1.03e-05, ('i0.small', 'b2'): 1.10e-06, ('i0.small', 'b2.reserved'): 6.33e-07, ('i0.small', 'b1'): 1.03e-06, ('i0.small', 'bo'): 9.15e-07, ('i0.small', 'bo.reserved'): 3.66e-07, ('i0.small', 'ln2_g'): 6.96e-07, ('i0.small', 'ln2_g.reserved'): 4.19e-07, ('i0.small', 'ln2_b'): 7.48e-07, ('i0.small', 'ln2_b.reserved'): 5.05e-07, ('i0.small', 'ln1_g'): 3.21e-08, ('i0.small', 'ln1_g.reserved'): 6.21e-08, ('i0.small', 'ln1_b'): 3.08e-08, ('i0.small', 'ln1_b.reserved'): 2.90e-08, ('i0.lnf', 'lnf_g'): 6.65e-08, ('i0.lnf', 'lnf_g.reserved'): 8.33e-08, ('i0.lnf', 'lnf_b'): 8.20e-08, ('i0.lnf', 'lnf_b.reserved'): 6.99e-08, ('i1.dwq', 'rows'): 1.08e-06, ('i1.dwkv', 'rows'): 4.63e-06, ('i1.dwo', 'rows'): 7.42e-06, ('i1.dw1', 'rows'): 1.29e-05, ('i1.dw2', 'rows'): 5.10e-06, ('i1.small', 'b2'): 3.49e-07, ('i1.small', 'b2.reserved'): 1.86e-07, ('i1.small', 'b1'): 6.93e-07, ('i1.small', 'bo'): 4.76e-07, ('i1.small', 'bo.reserved'): 3.43e-07, ('i1.small', 'ln2_g'): 7.74e-07, ('i1.small', 'ln2_g.reserved'): 5.79e-07, ('i1.small', 'ln2_b'): 5.47e-07, ('i1.small', 'ln2_b.reserved'): 5.10e-07, ('i1.small', 'ln1_g'): 5.93e-08, ('i1.small', 'ln1_g.reserved'): 1.01e-07, ('i1.small', 'ln1_b'): 7.18e-08, ('i1.small', 'ln1_b.reserved'): 5.68e-08, ('i1.lnf', 'lnf_g'): 2.34e-06, ('i1.lnf', 'lnf_g.reserved'): 2.66e-07, ('i1.lnf', 'lnf_b'): 1.73e-06, ('i1.lnf', 'lnf_b.reserved'): 1.92e-06},
    ((1, 129, 1, False), 4): {('cls', 'mean'): 1.10e-06, ('cls', 'max'): 8.19e-07, ('dmri_tok', 'flat'): 1.26e-05, ('dmri_tok', 'peaked'): 1.41e-05, ('dmri_tok', 'low'): 2.53e-05, ('dmri_tok', 'high'): 4.04e-05, ('dmri_tok.reserved', 'flat'): 7.24e-06, ('dmri_tok.reserved', 'peaked'): 5.90e-06, ('dmri_tok.reserved', 'low'): 5.92e-06, ('dmri_tok.reserved', 'high'): 6.10e-06, ('dpet_tok', 'flat'): 1.02e-05, ('dpet_tok', 'peaked'): 1.56e-05, ('dpet_tok', 'low'): 1.56e-05, ('dpet_tok', 'high'): 3.77e-05, ('dpet_tok.reserved', 'flat'): 2.96e-06, ('dpet_tok.reserved', 'peaked'): 2.62e-06, ('dpet_tok.reserved', 'low'): 3.90e-06, ('dpet_tok.reserved', 'high'): 2.60e-06, ('i0.dwq', 'rows'): 1.07e-06, ('i0.dwkv', 'rows'): 5.66e-06, ('i0.dwo', 'rows'): 1.47e-05, ('i0.dw1', 'rows'): 2.16e-05, ('i0.dw2', 'rows'): 1.04e-05, ('i0.small', 'b2'): 1.62e-06, ('i0.small', 'b2.reserved'): 1.02e-06, ('i0.small', 'b1'): 1.19e-06, ('i0.small', 'bo'): 1.38e-06, ('i0.small', 'bo.reserved'): 8.24e-07, ('i0.small', 'ln2_g'): 1.56e-06, ('i0.small', 'ln2_g.reserved'): 6.87e-07, ('i0.small', 'ln2_b'): 1.06e-06, ('i0.small', 'ln2_b.reserved'): 5.76e-07, ('i0.small', 'ln1_g'): 5.90e-08, ('i0.small', 'ln1_g.reserved'): 1.89e-07, ('i0.small', 'ln1_b'): 3.89e-08, ('i0.small', 'ln1_b.reserved'): 1.43e-07, ('i0.lnf', 'lnf_g'): 1.26e-07, ('i0.lnf', 'lnf_g.reserved'): 2.46e-07, ('i0.lnf', 'lnf_b'): 1.07e-07, ('i0.lnf', 'lnf_b.reserved'): 2.44e-07, ('i1.dwq', 'rows'): 1.54e-06, ('i1.dwkv', 'rows'): 6.16e-06, ('i1.dwo', 'rows'): 2.48e-05, ('i1.dw1', 'rows'): 2.69e-05, ('i1.dw2', 'rows'): 1.03e-05, ('i1.small', 'b2'): 1.22e-06, ('i1.small', 'b2.reserved'): 3.14e-07, ('i1.small', 'b1'): 1.45e-06, ('i1.small', 'bo'): 8.82e-07, ('i1.small', 'bo.reserved'): 8.63e-07, ('i1.small', 'ln2_g'): 1.81e-06, ('i1.small', 'ln2_g.reserved'): 7.52e-07, ('i1.small', 'ln2_b'): 1.08e-06, ('i1.small', 'ln2_b.reserved'): 1.57e-06, ('i1.small', 'ln1_g'): 8.12e-08, ('i1.small', 'ln1_g.reserved'): 2.57e-07, ('i1.small', 'ln1_b'): 8.68e-08, ('i1.small', 'ln1_b.reserved'): 1.85e-07, ('i1.lnf', 'lnf_g'): 3.62e-06, ('i1.lnf', 'lnf_g.reserved'): 4.58e-07, ('i1.lnf', 'lnf_b'): 2.08e-06, ('i1.lnf', 'lnf_b.reserved'): 8.25e-07},
    ((1, 129, 1, False), 8): {('cls', 'mean'): 6.68e-07, ('cls', 'max'): 5.86e-07, ('dmri_tok', 'flat'): 6.02e-06, ('dmri_tok', 'peaked'): 7.46e-06, ('dmri_tok', 'low'): 8.75e-06, ('dmri_tok', 'high'): 1.77e-05, ('dmri_tok.reserved', 'flat'): 1.48e-06, ('dmri_tok.reserved', 'peaked'): 1.76e-06, ('dmri_tok.reserved', 'low'): 2.19e-06, ('dmri_tok.reserved', 'high'): 2.47e-06, ('dpet_tok', 'flat'): 5.34e-06, ('dpet_tok', 'peaked'): 9.85e-06, ('dpet_tok', 'low'): 1.51e-05, ('dpet_tok', 'high'): 1.07e-05, ('dpet_tok.reserved', 'flat'): 1.22e-06, ('dpet_tok.reserved', 'peaked'): 1.40e-06, ('dpet_tok.reserved', 'low'): 1.12e-06, ('dpet_tok.reserved', 'high'): 1.48e-06, ('i0.dwq', 'rows'): 6.35e-07, ('i0.dwkv', 'rows'): 4.25e-06, ('i0.dwo', 'rows'): 1.26e-05, ('i0.dw1', 'rows'): 9.18e-06, ('i0.dw2', 'rows'): 8.58e-06, ('i0.small', 'b2'): 1.08e-06, ('i0.small', 'b2.reserved'): 3.19e-07, ('i0.small', 'b1'): 9.62e-07, ('i0.small', 'bo'): 8.77e-07, ('i0.small', 'bo.reserved'): 3.55e-07, ('i0.small', 'ln2_g'): 5.95e-07, ('i0.small', 'ln2_g.reserved'): 3.80e-07, ('i0.small', 'ln2_b'): 8.46e-07, ('i0.small', 'ln2_b.reserved'): 5.52e-07, ('i0.small', 'ln1_g'): 4.07e-08, ('i0.small', 'ln1_g.reserved'): 6.44e-08, ('i0.small', 'ln1_b'): 3.23e-08, ('i0.small', 'ln1_b.reserved'): 2.89e-08, ('i0.lnf', 'lnf_g'): 6.44e-08, ('i0.lnf', 'lnf_g.reserved'): 1.28e-07, ('i0.lnf', 'lnf_b'): 8.03e-08, ('i0.lnf', 'lnf_b.reserved'): 9.75e-08, ('i1.dwq', 'rows'): 1.21e-06, ('i1.dwkv', 'rows'): 7.80e-06, ('i1.dwo', 'rows'): 1.13e-05, ('i1.dw1', 'rows'): 1.18e-05, ('i1.dw2', 'rows'): 5.43e-06, ('i1.small', 'b2'): 3.13e-07, ('i1.small', 'b2.reserved'): 3.42e-07, ('i1.small', 'b1'): 5.81e-07, ('i1.small', 'bo'): 3.55e-07, ('i1.small', 'bo.reserved'): 3.03e-07, ('i1.small', 'ln2_g'): 7.85e-07, ('i1.small', 'ln2_g.reserved'): 4.56e-07, ('i1.small', 'ln2_b'): 4.50e-07, ('i1.small', 'ln2_b.reserved'): 3.17e-07, ('i1.small', 'ln1_g'): 5.85e-08, ('i1.small', 'ln1_g.reserved'): 1.43e-07, ('i1.small', 'ln1_b'): 4.97e-08, ('i1.small', 'ln1_b.reserved'): 5.88e-08, ('i1.lnf', 'lnf_g'): 1.38e-06, ('i1.lnf', 'lnf_g.reserved'): 1.46e-07, ('i1.lnf', 'lnf_b'): 1.77e-06, ('i1.lnf', 'lnf_b.reserved'): 1.09e-06},
    ((1, 144, 1, False), 4): {('cls', 'mean'): 6.11e-07, ('cls', 'max'): 1.05e-06, ('dmri_tok', 'flat'): 3.16e-05, ('dmri_tok', 'peaked'): 2.68e-05, ('dmri_tok', 'low'): 2.36e-05, ('dmri_tok', 'high'): 3.11e-05, ('dmri_tok.reserved', 'flat'): 9.92e-06, ('dmri_tok.reserved', 'peaked'): 5.83e-06, ('dmri_tok.reserved', 'low'): 5.07e-06, ('dmri_tok.reserved', 'high'): 8.46e-06, ('dpet_tok', 'flat'): 1.25e-05, ('dpet_tok', 'peaked'): 1.40e-05, ('dpet_tok', 'low'): 2.61e-05, ('dpet_tok', 'high'): 4.25e-05, ('dpet_tok.reserved', 'flat'): 3.77e-06, ('dpet_tok.reserved', 'peaked'): 3.47e-06, ('dpet_tok.reserved', 'low'): 3.42e-06, ('dpet_tok.reserved', 'high'): 3.28e-06, ('i0.dwq', 'rows'): 1.37e-06, ('i0.dwkv', 'rows'): 8.37e-06, ('i0.dwo', 'rows'): 1.77e-05, ('i0.dw1', 'rows'): 3.47e-05, ('i0.dw2', 'rows'): 1.87e-05, ('i0.small', 'b2'): 1.95e-06, ('i0.small', 'b2.reserved'): 8.32e-07, ('i0.small', 'b1'): 1.33e-06, ('i0.small', 'bo'): 1.85e-06, ('i0.small', 'bo.reserved'): 7.82e-07, ('i0.small', 'ln2_g'): 2.17e-06, ('i0.small', 'ln2_g.reserved'): 8.58e-07, ('i0.small', 'ln2_b'): 1.21e-06, ('i0.small', 'ln2_b.reserved'): 8.54e-07, ('i0.small', 'ln1_g'): 6.48e-08, ('i0.small', 'ln1_g.reserved'): 1.76e-07, ('i0.small', 'ln1_b'): 4.46e-08, ('i0.small', 'ln1_b.reserved'): 8.02e-08, ('i0.lnf', 'lnf_g'): 1.31e-07, ('i0.lnf', 'lnf_g.reserved'): 2.93e-07, ('i0.lnf', 'lnf_b'): 1.15e-07, ('i0.lnf', 'lnf_b.reserved'): 2.49e-07, ('i1.dwq', 'rows'): 1.53e-06, ('i1.dwkv', 'rows'): 4.77e-06, ('i1.dwo', 'rows'): 1.93e-05, ('i1.dw1', 'rows'): 2.88e-05, ('i1.dw2', 'rows'): 1.25e-05, ('i1.small', 'b2'): 9.73e-07, ('i1.small', 'b2.reserved'): 3.08e-07, ('i1.small', 'b1'): 2.08e-06, ('i1.small', 'bo'): 1.14e-06, ('i1.small', 'bo.reserved'): 7.55e-07, ('i1.small', 'ln2_g'): 2.39e-06, ('i1.small', 'ln2_g.reserved'): 1.89e-06, ('i1.small', 'ln2_b'): 1.20e-06, ('i1.small', 'ln2_b.reserved'): 1.16e-06, ('i1.small', 'ln1_g'): 1.09e-07, ('i1.small', 'ln1_g.reserved'): 2.16e-07, ('i1.small', 'ln1_b'): 9.37e-08, ('i1.small', 'ln1_b.reserved'): 1.15e-07, ('i1.lnf', 'lnf_g'): 3.32e-06, ('i1.lnf', 'lnf_g.reserved'): 5.96e-07, ('i1.lnf', 'lnf_b'): 2.35e-06, ('i1.lnf', 'lnf_b.reserved'): 9.85e-07},
    ((1, 144, 1, False), 8): {('cls', 'mean'): 3.70e-07, ('cls', 'max'): 4.38e-07, ('dmri_tok', 'flat'): 1.14e-05, ('dmri_tok', 'peaked'): 1.07e-05, ('dmri_tok', 'low'): 1.06e-05, ('dmri_tok', 'high'): 1.11e-05, ('dmri_tok.reserved', 'flat'): 2.63e-06, ('dmri_tok.reserved', 'peaked'): 2.16e-06, ('dmri_tok.reserved', 'low'): 2.51e-06, ('dmri_tok.reserved', 'high'): 1.90e-06, ('dpet_tok', 'flat'): 3.48e-06, ('dpet_tok', 'peaked'): 6.77e-06, ('dpet_tok', 'low'): 1.20e-05, ('dpet_tok', 'high'): 1.45e-05, ('dpet_tok.reserved', 'flat'): 9.10e-07, ('dpet_tok.reserved', 'peaked'): 1.54e-06, ('dpet_tok.reserved', 'low'): 1.20e-06, ('dpet_tok.reserved', 'high'): 1.20e-06, ('i0.dwq', 'rows'): 5.76e-07, ('i0.dwkv', 'rows'): 8.54e-06, ('i0.dwo', 'rows'): 8.11e-06, ('i0.dw1', 'rows'): 1.35e-05, ('i0.dw2', 'rows'): 1.15e-05, ('i0.small', 'b2'): 1.61e-06, ('i0.small', 'b2.reserved'): 1.05e-06, ('i0.small', 'b1'): 1.19e-06, ('i0.small', 'bo'): 1.41e-06, ('i0.small', 'bo.reserved'): 7.62e-07, ('i0.small', 'ln2_g'): 6.44e-07, ('i0.small', 'ln2_g.reserved'): 1.23e-06, ('i0.small', 'ln2_b'): 8.00e-07, ('i0.small', 'ln2_b.reserved'): 8.06e-07, ('i0.small', 'ln1_g'): 3.31e-08, ('i0.small', 'ln1_g.reserved'): 7.77e-08, ('i0.small', 'ln1_b'): 3.32e-08, ('i0.small', 'ln1_b.reserved'): 2.53e-08, ('i0.lnf', 'lnf_g'): 8.85e-08, ('i0.lnf', 'lnf_g.reserved'): 9.16e-08, ('i0.lnf', 'lnf_b'): 1.04e-07, ('i0.lnf', 'lnf_b.reserved'): 7.53e-08, ('i1.dwq', 'rows'): 1.11e-06, ('i1.dwkv', 'rows'): 3.79e-06, ('i1.dwo', 'rows'): 1.01e-05, ('i1.dw1', 'rows'): 2.10e-05, ('i1.dw2', 'rows'): 5.38e-06, ('i1.small', 'b2'): 4.75e-07, ('i1.small', 'b2.reserved'): 2.74e-07, ('i1.small', 'b1'): 4.44e-07, ('i1.small', 'bo'): 4.18e-07, ('i1.small', 'bo.reserved'): 2.36e-07, ('i1.small', 'ln2_g'): 7.85e-07, ('i1.small', 'ln2_g.reserved'): 4.84e-07, ('i1.small', 'ln2_b'): 5.96e-07, ('i1.small', 'ln2_b.reserved'): 3.08e-07, ('i1.small', 'ln1_g'): 4.84e-08, ('i1.small', 'ln1_g.reserved'): 8.11e-08, ('i1.small', 'ln1_b'): 7.98e-08, ('i1.small', 'ln1_b.reserved'): 4.92e-08, ('i1.lnf', 'lnf_g'): 1.57e-06, ('i1.lnf', 'lnf_g.reserved'): 2.03e-07, ('i1.lnf', 'lnf_b'): 1.63e-06, ('i1.lnf', 'lnf_b.reserved'): 1.28e-06},
    ((1, 145, 1, False), 4): {('cls', 'mean'): 8.98e-07, ('cls', 'max'): 1.04e-06, ('dmri_tok', 'flat'): 2.17e-05, ('dmri_tok', 'peaked'): 1.69e-05, ('dmri_tok', 'low'): 3.15e-05, ('dmri_tok', 'high'): 2.35e-05, ('dmri_tok.reserved', 'flat'): 6.07e-06, ('dmri_tok.reserved', 'peaked'): 4.72e-06, ('dmri_tok.reserved', 'low'): 5.61e-06, ('dmri_tok.reserved', 'high'): 4.58e-06, ('dpet_tok', 'flat'): 1.11e-05, ('dpet_tok', 'peaked'): 1.27e-05, ('dpet_tok', 'low'): 6.42e-05, ('dpet_tok', 'high'): 3.68e-05, ('dpet_tok.reserved', 'flat'): 4.83e-06, ('dpet_tok.reserved', 'peaked'): 4.02e-06, ('dpet_tok.reserved', 'low'): 5.67e-06, ('dpet_tok.reserved', 'high'): 2.92e-06, ('i0.dwq', 'rows'): 1.11e-06, ('i0.dwkv', 'rows'): 9.06e-06, ('i0.dwo', 'rows'): 1.74e-05, ('i0.dw1', 'rows'): 2.71e-05, ('i0.dw2', 'rows'): 1.12e-05, ('i0.small', 'b2'): 1.44e-06, ('i0.small', 'b2.reserved'): 6.45e-07, ('i0.small', 'b1'): 1.33e-06, ('i0.small', 'bo'): 1.29e-06, ('i0.small', 'bo.reserved'): 6.18e-07, ('i0.small', 'ln2_g'): 1.46e-06, ('i0.small', 'ln2_g.reserved'): 1.52e-06, ('i0.small', 'ln2_b'): 1.20e-06, ('i0.small', 'ln2_b.reserved'): 7.23e-07, ('i0.small', 'ln1_g'): 4.38e-08, ('i0.small', 'ln1_g.reserved'): 1.86e-07, ('i0.small', 'ln1_b'): 3.59e-08, ('i0.small', 'ln1_b.reserved'): 8.31e-08, ('i0.lnf', 'lnf_g'): 1.21e-07, ('i0.lnf', 'lnf_g.reserved'): 3.01e-07, ('i0.lnf', 'lnf_b'): 1.12e-07, ('i0.lnf', 'lnf_b.reserved'): 2.32e-07, ('i1.dwq', 'rows'): 3.72e-06, ('i1.dwkv', 'rows'): 5.85e-06, ('i1.dwo', 'rows'): 1.93e-05, ('i1.dw1', 'rows'): 2.67e-05, ('i1.dw2', 'rows'): 1.26e-05, ('i1.small', 'b2'): 6.21e-07, ('i1.small', 'b2.reserved'): 5.36e-07, ('i1.small', 'b1'): 1.29e-06, ('i1.small', 'bo'): 7.76e-07, ('i1.small', 'bo.reserved'): 6.78e-07, ('i1.small', 'ln2_g'): 1.41e-06, ('i1.small', 'ln2_g.reserved'): 7.49e-07, ('i1.small', 'ln2_b'): 1.01e-06, ('i1.small', 'ln2_b.reserved'): 1.06e-06, ('i1.small', 'ln1_g'): 1.05e-07, ('i1.small', 'ln1_g.reserved'): 2.77e-07, ('i1.small', 'ln1_b'): 1.08e-07, ('i1.small', 'ln1_b.reserved'): 1.29e-07, ('i1.lnf', 'lnf_g'): 2.80e-06, ('i1.lnf', 'lnf_g.reserved'): 2.51e-07, ('i1.lnf', 'lnf_b'): 2.35e-06, ('i1.lnf', 'lnf_b.reserved'): 1.22e-06},
    ((1, 145, 1, False), 8): {('cls', 'mean'): 3.09e-07, ('cls', 'max'): 3.85e-07, ('dmri_tok', 'flat'): 9.62e-06, ('dmri_tok', 'peaked'): 7.01e-06, ('dmri_tok', 'low'): 8.05e-06, ('dmri_tok', 'high'): 1.35e-05, ('dmri_tok.reserved', 'flat'): 2.05e-06, ('dmri_tok.reserved', 'peaked'): 2.70e-06, ('dmri_tok.reserved', 'low'): 1.64e-06, ('dmri_tok.reserved', 'high'): 2.40e-06, ('dpet_tok', 'flat'): 4.65e-06, ('dpet_tok', 'peaked'): 7.08e-06, ('dpet_tok', 'low'): 1.61e-05, ('dpet_tok', 'high'): 1.46e-05, ('dpet_tok.reserved', 'flat'): 1.14e-06, ('dpet_tok.reserved', 'peaked'): 1.31e-06, ('dpet_tok.reserved', 'low'): 1.43e-06, ('dpet_tok.reserved', 'high'): 1.55e-06, ('i0.dwq', 'rows'): 5.76e-07, ('i0.dwkv', 'rows'): 3.81e-06, ('i0.dwo', 'rows'): 1.09e-05, ('i0.dw1', 'rows'): 1.15e-05, ('i0.dw2', 'rows'): 7.14e-06, ('i0.small', 'b2'): 7.75e-07, ('i0.small', 'b2.reserved'): 3.53e-07, ('i0.small', 'b1'): 6.51e-07, ('i0.small', 'bo'): 7.41e-07, ('i0.small', 'bo.reserved'): 3.39e-07, ('i0.small', 'ln2_g'): 5.68e-07, ('i0.small', 'ln2_g.reserved'): 4.64e-07, ('i0.small', 'ln2_b'): 5.14e-07, ('i0.small', 'ln2_b.reserved'): 4.71e-07, ('i0.small', 'ln1_g'): 3.24e-08, ('i0.small', 'ln1_g.reserved'): 5.47e-08, ('i0.small', 'ln1_b'): 2.80e-08, ('i0.small', 'ln1_b.reserved'): 2.54e-08, ('i0.lnf', 'lnf_g'): 5.63e-08, ('i0.lnf', 'lnf_g.reserved'): 1.04e-07, ('i0.lnf', 'lnf_b'): 6.49e-08, ('i0.lnf', 'lnf_b.reserved'): 1.18e-07, ('i1.dwq', 'rows'): 8.89e-07, ('i1.dwkv', 'rows'): 2.94e-06, ('i1.dwo', 'rows'): 6.00e-06, ('i1.dw1', 'rows'): 7.32e-06, ('i1.dw2', 'rows'): 4.14e-06, ('i1.small', 'b2'): 5.06e-07, ('i1.small', 'b2.reserved'): 1.82e-07, ('i1.small', 'b1'): 5.02e-07, ('i1.small', 'bo'): 4.58e-07, ('i1.small', 'bo.reserved'): 3.20e-07, ('i1.small', 'ln2_g'): 5.89e-07, ('i1.small', 'ln2_g.reserved'): 4.08e-07, ('i1.small', 'ln2_b'): 4.44e-07, ('i1.small', 'ln2_b.reserved'): 3.74e-07, ('i1.small', 'ln1_g'): 6.40e-08, ('i1.small', 'ln1_g.reserved'): 1.33e-07, ('i1.small', 'ln1_b'): 4.60e-08, ('i1.small', 'ln1_b.reserved'): 4.60e-08, ('i1.lnf', 'lnf_g'): 1.12e-06, ('i1.lnf', 'lnf_g.reserved'): 3.92e-07, ('i1.lnf', 'lnf_b'): 3.77e-06, ('i1.lnf', 'lnf_b.reserved'): 1.78e-06},
    ((1, 160, 1, True), 4): {('cls', 'mean'): 7.83e-07, ('cls', 'max'): 1.35e-06, ('dmri_tok', 'flat'): 1.28e-05, ('dmri_tok', 'peaked'): 1.61e-05, ('dmri_tok', 'low'): 2.68e-05, ('dmri_tok', 'high'): 1.93e-05, ('dmri_tok.reserved', 'flat'): 5.01e-06, ('dmri_tok.reserved', 'peaked'): 7.68e-06, ('dmri_tok.reserved', 'low'): 6.56e-06, ('dmri_tok.reserved', 'high'): 6.57e-06, ('dpet_tok', 'flat'): 1.12e-05, ('dpet_tok', 'peaked'): 2.17e-05, ('dpet_tok', 'low'): 3.85e-05, ('dpet_tok', 'high'): 4.03e-05, ('dpet_tok.reserved', 'flat'): 5.35e-06, ('dpet_tok.reserved', 'peaked'): 4.51e-06, ('dpet_tok.reserved', 'low'): 5.66e-06, ('dpet_tok.reserved', 'high'): 4.07e-06, ('i0.dwq', 'rows'): 1.08e-06, ('i0.dwkv', 'rows'): 9.04e-06, ('i0.dwo', 'rows'): 2.73e-05, ('i0.dw1', 'rows'): 3.05e-05, ('i0.dw2', 'rows'): 1.74e-05, ('i0.small', 'b2'): 1.92e-06, ('i0.small', 'b2.reserved'): 1.15e-06, ('i0.small', 'b1'): 1.10e-06, ('i0.small', 'bo'): 1.02e-06, ('i0.small', 'bo.reserved'): 6.02e-07, ('i0.small', 'ln2_g'): 9.69e-07, ('i0.small', 'ln2_g.reserved'): 4.81e-07, ('i0.small', 'ln2_b'): 8.12e-07, ('i0.small', 'ln2_b.reserved'): 5.19e-07, ('i0.small', 'ln1_g'): 5.74e-08, ('i0.small', 'ln1_g.reserved'): 1.47e-07, ('i0.small', 'ln1_b'): 5.71e-08, ('i0.small', 'ln1_b.reserved'): 1.25e-07, ('i0.lnf', 'lnf_g'): 1.53e-07, ('i0.lnf', 'lnf_g.reserved'): 2.49e-07, ('i0.lnf', 'lnf_b'): 9.99e-08, ('i0.lnf', 'lnf_b.reserved'): 1.96e-07, ('i1.dwq', 'rows'): 1.87e-06, ('i1.dwkv', 'rows'): 4.60e-06, ('i1.dwo', 'rows'): 1.51e-05, ('i1.dw1', 'rows'): 2.52e-05, ('i1.dw2', 'rows'): 9.05e-06, ('i1.small', 'b2'): 1.10e-06, ('i1.small', 'b2.reserved'): 4.51e-07, ('i1.small', 'b1'): 1.34e-06, ('i1.small', 'bo'): 7.51e-07, ('i1.small', 'bo.reserved'): 9.67e-07, ('i1.small', 'ln2_g'): 2.29e-06, ('i1.small', 'ln2_g.reserved'): 1.59e-06, ('i1.small', 'ln2_b'): 9.18e-07, ('i1.small', 'ln2_b.reserved'): 8.14e-07, ('i1.small', 'ln1_g'): 8.77e-08, ('i1.small', 'ln1_g.reserved'): 2.77e-07, ('i1.small', 'ln1_b'): 8.24e-08, ('i1.small', 'ln1_b.reserved'): 1.20e-07, ('i1.lnf', 'lnf_g'): 2.21e-06, ('i1.lnf', 'lnf_g.reserved'): 2.86e-07, ('i1.lnf', 'lnf_b'): 2.37e-06, ('i1.lnf', 'lnf_b.reserved'): 6.26e-06},
    ((1, 160, 1, True), 8): {('cls', 'mean'): 4.64e-07, ('cls', 'max'): 6.15e-07, ('dmri_tok', 'flat'): 6.53e-06, ('dmri_tok', 'peaked'): 9.05e-06, ('dmri_tok', 'low'): 1.22e-05, ('dmri_tok', 'high'): 6.63e-06, ('dmri_tok.reserved', 'flat'): 1.93e-06, ('dmri_tok.reserved', 'peaked'): 1.73e-06, ('dmri_tok.reserved', 'low'): 2.25e-06, ('dmri_tok.reserved', 'high'): 1.75e-06, ('dpet_tok', 'flat'): 5.07e-06, ('dpet_tok', 'peaked'): 9.19e-06, ('dpet_tok', 'low'): 1.22e-05, ('dpet_tok', 'high'): 1.92e-05, ('dpet_tok.reserved', 'flat'): 1.20e-06, ('dpet_tok.reserved', 'peaked'): 1.28e-06, ('dpet_tok.reserved', 'low'): 1.51e-06, ('dpet_tok.reserved', 'high'): 1.35e-06, ('i0.dwq', 'rows'): 5.50e-07, ('i0.dwkv', 'rows'): 6.90e-06, ('i0.dwo', 'rows'): 9.20e-06, ('i0.dw1', 'rows'): 1.19e-05, ('i0.dw2', 'rows'): 1.13e-05, ('i0.small', 'b2'): 1.71e-06, ('i0.small', 'b2.reserved'): 4.12e-07, ('i0.small', 'b1'): 7.76e-07, ('i0.small', 'bo'): 9.08e-07, ('i0.small', 'bo.reserved'): 2.54e-07, ('i0.small', 'ln2_g'): 6.64e-07, ('i0.small', 'ln2_g.reserved'): 4.36e-07, ('i0.small', 'ln2_b'): 4.92e-07, ('i0.small', 'ln2_b.reserved'): 5.70e-07, ('i0.small', 'ln1_g'): 3.04e-08, ('i0.small', 'ln1_g.reserved'): 8.72e-08, ('i0.small', 'ln1_b'): 2.74e-08, ('i0.small', 'ln1_b.reserved'): 2.43e-08, ('i0.lnf', 'lnf_g'): 5.83e-08, ('i0.lnf', 'lnf_g.reserved'): 7.84e-08, ('i0.lnf', 'lnf_b'): 7.46e-08, ('i0.lnf', 'lnf_b.reserved'): 6.56e-08, ('i1.dwq', 'rows'): 1.48e-06, ('i1.dwkv', 'rows'): 3.77e-06, ('i1.dwo', 'rows'): 8.83e-06, ('i1.dw1', 'rows'): 1.47e-05, ('i1.dw2', 'rows'): 5.52e-06, ('i1.small', 'b2'): 4.66e-07, ('i1.small', 'b2.reserved'): 3.08e-07, ('i1.small', 'b1'): 9.17e-07, ('i1.small', 'bo'): 6.36e-07, ('i1.small', 'bo.reserved'): 5.03e-07, ('i1.small', 'ln2_g'): 9.42e-07, ('i1.small', 'ln2_g.reserved'): 3.75e-07, ('i1.small', 'ln2_b'): 6.97e-07, ('i1.small', 'ln2_b.reserved'): 4.02e-07, ('i1.small', 'ln1_g'): 6.53e-08, ('i1.small', 'ln1_g.reserved'): 8.12e-08, ('i1.small', 'ln1_b'): 4.40e-08, ('i1.small', 'ln1_b.reserved'): 4.48e-08, ('i1.lnf', 'lnf_g'): 1.59e-06, ('i1.lnf', 'lnf_g.reserved'): 3.76e-07, ('i1.lnf', 'lnf_b'): 3.07e-06, ('i1.lnf', 'lnf_b.reserved'): 1.08e-06},
    ((1, 161, 1, False), 4): {('cls', 'mean'): 4.04e-07, ('cls', 'max'): 8.31e-07, ('dmri_tok', 'flat'): 2.06e-05, ('dmri_tok', 'peaked'): 1.31e-05, ('dmri_tok', 'low'): 2.10e-05, ('dmri_tok', 'high'): 2.76e-05, ('dmri_tok.reserved', 'flat'): 5.60e-06, ('dmri_tok.reserved', 'peaked'): 5.36e-06, ('dmri_tok.reserved', 'low'): 6.82e-06, ('dmri_tok.reserved', 'high'): 5.17e-06, ('dpet_tok', 'flat'): 1.35e-05, ('dpet_tok', 'peaked'): 1.20e-05, ('dpet_tok', 'low'): 2.28e-05, ('dpet_tok', 'high'): 4.36e-05, ('dpet_tok.reserved', 'flat'): 3.58e-06, ('dpet_tok.reserved', 'peaked'): 4.62e-06, ('dpet_tok.reserved', 'low'): 4.05e-06, ('dpet_tok.reserved', 'high'): 2.86e-06, ('i0.dwq', 'rows'): 1.17e-06, ('i0.dwkv', 'rows'): 6.80e-06, ('i0.dwo', 'rows'): 1.83e-05, ('i0.dw1', 'rows'): 2.51e-05, ('i0.dw2', 'rows'): 1.08e-05, ('i0.small', 'b2'): 1.47e-06, ('i0.small', 'b2.reserved'): 1.16e-06, ('i0.small', 'b1'): 1.04e-06, ('i0.small', 'bo'): 1.19e-06, ('i0.small', 'bo.reserved'): 1.12e-06, ('i0.small', 'ln2_g'): 9.00e-07, ('i0.small', 'ln2_g.reserved'): 6.71e-07, ('i0.small', 'ln2_b'): 9.50e-07, ('i0.small', 'ln2_b.reserved'): 8.36e-07, ('i0.small', 'ln1_g'): 6.58e-08, ('i0.small', 'ln1_g.reserved'): 1.53e-07, ('i0.small', 'ln1_b'): 3.91e-08, ('i0.small', 'ln1_b.reserved'): 6.35e-08, ('i0.lnf', 'lnf_g'): 9.08e-08, ('i0.lnf', 'lnf_g.reserved'): 4.03e-07, ('i0.lnf', 'lnf_b'): 9.49e-08, ('i0.lnf', 'lnf_b.reserved'): 2.02e-07, ('i1.dwq', 'rows'): 1.92e-06, ('i1.dwkv', 'rows'): 6.92e-06, ('i1.dwo', 'rows'): 2.22e-05, ('i1.dw1', 'rows'): 2.01e-05, ('i1.dw2', 'rows'): 9.12e-06, ('i1.small', 'b2'): 6.08e-07, ('i1.small', 'b2.reserved'): 4.32e-07, ('i1.small', 'b1'): 1.21e-06, ('i1.small', 'bo'): 9.15e-07, ('i1.small', 'bo.reserved'): 4.69e-07, ('i1.small', 'ln2_g'): 1.44e-06, ('i1.small', 'ln2_g.reserved'): 1.92e-06, ('i1.small', 'ln2_b'): 9.82e-07, ('i1.small', 'ln2_b.reserved'): 5.64e-07, ('i1.small', 'ln1_g'): 8.88e-08, ('i1.small', 'ln1_g.reserved'): 2.79e-07, ('i1.small', 'ln1_b'): 7.62e-08, ('i1.small', 'ln1_b.reserved'): 2.16e-07, ('i1.lnf', 'lnf_g'): 2.49e-06, ('i1.lnf', 'lnf_g.reserved'): 2.09e-07, ('i1.lnf', 'lnf_b'): 3.13e-06, ('i1.lnf', 'lnf_b.reserved'): 2.58e-06},
    ((1, 161, 1, False), 8): {('cls', 'mean'): 6.94e-07, ('cls', 'max'): 3.26e-07, ('dmri_tok', 'flat'): 6.58e-06, ('dmri_tok', 'peaked'): 1.16e-05, ('dmri_tok', 'low'): 1.23e-05, ('dmri_tok', 'high'): 7.80e-06, ('dmri_tok.reserved', 'flat'): 2.37e-06, ('dmri_tok.reserved', 'peaked'): 1.95e-06, ('dmri_tok.reserved', 'low'): 1.86e-06, ('dmri_tok.reserved', 'high'): 1.77e-06, ('dpet_tok', 'flat'): 5.94e-06, ('dpet_tok', 'peaked'): 6.96e-06, ('dpet_tok', 'low'): 1.09e-05, ('dpet_tok', 'high'): 1.13e-05, ('dpet_tok.reserved', 'flat'): 1.42e-06, ('dpet_tok.reserved', 'peaked'): 1.40e-06, ('dpet_tok.reserved', 'low'): 1.81e-06, ('dpet_tok.reserved', 'high'): 1.98e-06, ('i0.dwq', 'rows'): 4.98e-07, ('i0.dwkv', 'rows'): 9.49e-06, ('i0.dwo', 'rows'): 8.74e-06, ('i0.dw1', 'rows'): 8.92e-06, ('i0.dw2', 'rows'): 9.58e-06, ('i0.small', 'b2'): 1.32e-06, ('i0.small', 'b2.reserved'): 4.99e-07, ('i0.small', 'b1'): 9.66e-07, ('i0.small', 'bo'): 1.08e-06, ('i0.small', 'bo.reserved'): 5.18e-07, ('i0.small', 'ln2_g'): 8.85e-07, ('i0.small', 'ln2_g.reserved'): 5.03e-07, ('i0.small', 'ln2_b'): 7.53e-07, ('i0.small', 'ln2_b.reserved'): 4.20e-07, ('i0.small', 'ln1_g'): 3.52e-08, ('i0.small', 'ln1_g.reserved'): 4.70e-08, ('i0.small', 'ln1_b'): 2.45e-08, ('i0.small', 'ln1_b.reserved'): 2.09e-08, ('i0.lnf', 'lnf_g'): 5.14e-08, ('i0.lnf', 'lnf_g.reserved'): 1.68e-07, ('i0.lnf', 'lnf_b'): 1.01e-07, ('i0.lnf', 'lnf_b.reserved'): 1.48e-07, ('i1.dwq', 'rows'): 8.78e-07, ('i1.dwkv', 'rows'): 5.20e-06, ('i1.dwo', 'rows'): 1.08e-05, ('i1.dw1', 'rows'): 1.28e-05, ('i1.dw2', 'rows'): 4.53e-06, ('i1.small', 'b2'): 2.93e-07, ('i1.small', 'b2.reserved'): 5.11e-07, ('i1.small', 'b1'): 6.59e-07, ('i1.small', 'bo'): 2.47e-07, ('i1.small', 'bo.reserved'): 3.85e-07, ('i1.small', 'ln2_g'): 7.08e-07, ('i1.small', 'ln2_g.reserved'): 3.31e-07, ('i1.small', 'ln2_b'): 3.76e-07, ('i1.small', 'ln2_b.reserved'): 2.54e-07, ('i1.small', 'ln1_g'): 8.49e-08, ('i1.small', 'ln1_g.reserved'): 1.66e-07, ('i1.small', 'ln1_b'): 5.25e-08, ('i1.small', 'ln1_b.reserved'): 5.59e-08, ('i1.lnf', 'lnf_g'): 1.89e-06, ('i1.lnf', 'lnf_g.reserved'): 5.84e-07, ('i1.lnf', 'lnf_b'): 2.94e-06, ('i1.lnf', 'lnf_b.reserved'): 1.40e-06},
    ((1, 208, 1, False), 4): {('cls', 'mean'): 1.62e-06, ('cls', 'max'): 9.75e-07, ('dmri_tok', 'flat'): 2.26e-05, ('dmri_tok', 'peaked'): 1.93e-05, ('dmri_tok', 'low'): 1.68e-05, ('dmri_tok', 'high'): 2.45e-05, ('dmri_tok.reserved', 'flat'): 5.90e-06, ('dmri_tok.reserved', 'peaked'): 7.70e-06, ('dmri_tok.reserved', 'low'): 7.32e-06, ('dmri_tok.reserved', 'high'): 5.59e-06, ('dpet_tok', 'flat'): 1.05e-05, ('dpet_tok', 'peaked'): 1.81e-05, ('dpet_tok', 'low'): 2.56e-05, ('dpet_tok', 'high'): 2.62e-05, ('dpet_tok.reserved', 'flat'): 4.40e-06, ('dpet_tok.reserved', 'peaked'): 3.96e-06, ('dpet_tok.reserved', 'low'): 3.30e-06, ('dpet_tok.reserved', 'high'): 2.98e-06, ('i0.dwq', 'rows'): 6.65e-07, ('i0.dwkv', 'rows'): 6.21e-06, ('i0.dwo', 'rows'): 1.51e-05, ('i0.dw1', 'rows'): 1.75e-05, ('i0.dw2', 'rows'): 1.15e-05, ('i0.small', 'b2'): 1.43e-06, ('i0.small', 'b2.reserved'): 4.53e-07, ('i0.small', 'b1'): 1.00e-06, ('i0.small', 'bo'): 1.09e-06, ('i0.small', 'bo.reserved'): 4.44e-07, ('i0.small', 'ln2_g'): 8.15e-07, ('i0.small', 'ln2_g.reserved'): 7.71e-07, ('i0.small', 'ln2_b'): 8.36e-07, ('i0.small', 'ln2_b.reserved'): 6.39e-07, ('i0.small', 'ln1_g'): 3.85e-08, ('i0.small', 'ln1_g.reserved'): 1.03e-07, ('i0.small', 'ln1_b'): 4.34e-08, ('i0.small', 'ln1_b.reserved'): 4.47e-08, ('i0.lnf', 'lnf_g'): 8.28e-08, ('i0.lnf', 'lnf_g.reserved'): 3.39e-07, ('i0.lnf', 'lnf_b'): 6.78e-08, ('i0.lnf', 'lnf_b.reserved'): 3.91e-07, ('i1.dwq', 'rows'): 1.35e-06, ('i1.dwkv', 'rows'): 5.54e-06, ('i1.dwo', 'rows'): 1.70e-05, ('i1.dw1', 'rows'): 3.62e-05, ('i1.dw2', 'rows'): 9.70e-06, ('i1.small', 'b2'): 6.44e-07, ('i1.small', 'b2.reserved'): 4.86e-07, ('i1.small', 'b1'): 1.09e-06, ('i1.small', 'bo'): 6.49e-07, ('i1.small', 'bo.reserved'): 3.99e-07, ('i1.small', 'ln2_g'): 1.58e-06, ('i1.small', 'ln2_g.reserved'): 5.71e-07, ('i1.small', 'ln2_b'): 1.02e-06, ('i1.small', 'ln2_b.reserved'): 3.79e-07, ('i1.small', 'ln1_g'): 6.08e-08, ('i1.small', 'ln1_g.reserved'): 4.20e-07, ('i1.small', 'ln1_b'): 4.79e-08, ('i1.small', 'ln1_b.reserved'): 8.79e-08, ('i1.lnf', 'lnf_g'): 2.09e-06, ('i1.lnf', 'lnf_g.reserved'): 1.46e-07, ('i1.lnf', 'lnf_b'): 3.42e-06, ('i1.lnf', 'lnf_b.reserved'): 1.57e-06},
    ((1, 208, 1, False), 8): {('cls', 'mean'): 9.47e-07, ('cls', 'max'): 3.51e-07, ('dmri_tok', 'flat'): 9.62e-06, ('dmri_tok', 'peaked'): 1.02e-05, ('dmri_tok', 'low'): 1.56e-05, ('dmri_tok', 'high'): 1.15e-05, ('dmri_tok.reserved', 'flat'): 1.85e-06, ('dmri_tok.reserved', 'peaked'): 1.70e-06, ('dmri_tok.reserved', 'low'): 2.23e-06, ('dmri_tok.reserved', 'high'): 1.64e-06, ('dpet_tok', 'flat'): 4.16e-06, ('dpet_tok', 'peaked'): 5.89e-06, ('dpet_tok', 'low'): 1.44e-05, ('dpet_tok', 'high'): 1.75e-05, ('dpet_tok.reserved', 'flat'): 1.36e-06, ('dpet_tok.reserved', 'peaked'): 1.12e-06, ('dpet_tok.reserved', 'low'): 1.33e-06, ('dpet_tok.reserved', 'high'): 1.53e-06, ('i0.dwq', 'rows'): 3.59e-07, ('i0.dwkv', 'rows'): 7.33e-06, ('i0.dwo', 'rows'): 8.86e-06, ('i0.dw1', 'rows'): 1.80e-05, ('i0.dw2', 'rows'): 7.33e-06, ('i0.small', 'b2'): 1.05e-06, ('i0.small', 'b2.reserved'): 2.95e-07, ('i0.small', 'b1'): 6.92e-07, ('i0.small', 'bo'): 8.73e-07, ('i0.small', 'bo.reserved'): 3.06e-07, ('i0.small', 'ln2_g'): 9.66e-07, ('i0.small', 'ln2_g.reserved'): 3.10e-07, ('i0.small', 'ln2_b'): 6.27e-07, ('i0.small', 'ln2_b.reserved'): 3.63e-07, ('i0.small', 'ln1_g'): 2.53e-08, ('i0.small', 'ln1_g.reserved'): 4.40e-08, ('i0.small', 'ln1_b'): 1.92e-08, ('i0.small', 'ln1_b.reserved'): 2.63e-08, ('i0.lnf', 'lnf_g'): 4.81e-08, ('i0.lnf', 'lnf_g.reserved'): 6.05e-08, ('i0.lnf', 'lnf_b'): 6.15e-08, ('i0.lnf', 'lnf_b.reserved'): 5.78e-08, ('i1.dwq', 'rows'): 7.27e-07, ('i1.dwkv', 'rows'): 3.00e-06, ('i1.dwo', 'rows'): 8.84e-06, ('i1.dw1', 'rows'): 1.25e-05, ('i1.dw2', 'rows'): 3.57e-06, ('i1.small', 'b2'): 3.74e-07, ('i1.small', 'b2.reserved'): 1.51e-07, ('i1.small', 'b1'): 5.38e-07, ('i1.small', 'bo'): 3.74e-07, ('i1.small', 'bo.reserved'): 2.29e-07, ('i1.small', 'ln2_g'): 8.88e-07, ('i1.small', 'ln2_g.reserved'): 3.68e-07, ('i1.small', 'ln2_b'): 4.94e-07, ('i1.small', 'ln2_b.reserved'): 2.74e-07, ('i1.small', 'ln1_g'): 4.83e-08, ('i1.small', 'ln1_g.reserved'): 5.81e-08, ('i1.small', 'ln1_b'): 2.29e-08, ('i1.small', 'ln1_b.reserved'): 2.90e-08, ('i1.lnf', 'lnf_g'): 6.95e-07, ('i1.lnf', 'lnf_g.reserved'): 2.41e-07, ('i1.lnf', 'lnf_b'): 4.26e-06, ('i1.lnf', 'lnf_b.reserved'): 1.37e-06},
    ((1, 209, 1, False), 4): {('cls', 'mean'): 4.46e-07, ('cls', 'max'): 6.73e-07, ('dmri_tok', 'flat'): 2.13e-05, ('dmri_tok', 'peaked'): 2.96e-05, ('dmri_tok', 'low'): 2.00e-05, ('dmri_tok', 'high'): 2.34e-05, ('dmri_tok.reserved', 'flat'): 6.58e-06, ('dmri_tok.reserved', 'peaked'): 5.86e-06, ('dmri_tok.reserved', 'low'): 9.24e-06, ('dmri_tok.reserved', 'high'): 5.13e-06, ('dpet_tok', 'flat'): 1.27e-05, ('dpet_tok', 'peaked'): 1.50e-05, ('dpet_tok', 'low'): 3.47e-05, ('dpet_tok', 'high'): 2.47e-05, ('dpet_tok.reserved', 'flat'): 3.49e-06, ('dpet_tok.reserved', 'peaked'): 3.88e-06, ('dpet_tok.reserved', 'low'): 2.96e-06, ('dpet_tok.reserved', 'high'): 4.41e-06, ('i0.dwq', 'rows'): 1.05e-06, ('i0.dwkv', 'rows'): 5.14e-06, ('i0.dwo', 'rows'): 1.59e-05, ('i0.dw1', 'rows'): 1.35e-05, ('i0.dw2', 'rows'): 9.61e-06, ('i0.small', 'b2'): 1.42e-06, ('i0.small', 'b2.reserved'): 6.64e-07, ('i0.small', 'b1'): 1.01e-06, ('i0.small', 'bo'): 1.12e-06, ('i0.small', 'bo.reserved'): 6.60e-07, ('i0.small', 'ln2_g'): 1.11e-06, ('i0.small', 'ln2_g.reserved'): 6.96e-07, ('i0.small', 'ln2_b'): 8.59e-07, ('i0.small', 'ln2_b.reserved'): 8.64e-07, ('i0.small', 'ln1_g'): 5.63e-08, ('i0.small', 'ln1_g.reserved'): 1.31e-07, ('i0.small', 'ln1_b'): 4.36e-08, ('i0.small', 'ln1_b.reserved'): 5.99e-08, ('i0.lnf', 'lnf_g'): 7.10e-08, ('i0.lnf', 'lnf_g.reserved'): 6.46e-07, ('i0.lnf', 'lnf_b'): 9.36e-08, ('i0.lnf', 'lnf_b.reserved'): 4.47e-07, ('i1.dwq', 'rows'): 1.76e-06, ('i1.dwkv', 'rows'): 5.12e-06, ('i1.dwo', 'rows'): 1.73e-05, ('i1.dw1', 'rows'): 1.71e-05, ('i1.dw2', 'rows'): 9.91e-06, ('i1.small', 'b2'): 8.18e-07, ('i1.small', 'b2.reserved'): 4.35e-07, ('i1.small', 'b1'): 1.16e-06, ('i1.small', 'bo'): 6.68e-07, ('i1.small', 'bo.reserved'): 4.74e-07, ('i1.small', 'ln2_g'): 1.08e-06, ('i1.small', 'ln2_g.reserved'): 7.10e-07, ('i1.small', 'ln2_b'): 6.75e-07, ('i1.small', 'ln2_b.reserved'): 3.53e-07, ('i1.small', 'ln1_g'): 8.44e-08, ('i1.small', 'ln1_g.reserved'): 4.80e-07, ('i1.small', 'ln1_b'): 6.17e-08, ('i1.small', 'ln1_b.reserved'): 1.21e-07, ('i1.lnf', 'lnf_g'): 1.97e-06, ('i1.lnf', 'lnf_g.reserved'): 1.75e-07, ('i1.lnf', 'lnf_b'): 2.52e-06, ('i1.lnf', 'lnf_b.reserved'): 1.16e-06},
    ((1, 209, 1, False), 8): {('cls', 'mean'): 6.91e-07, ('cls', 'max'): 5.03e-07, ('dmri_tok', 'flat'): 8.47e-06, ('dmri_tok', 'peaked'): 1.13e-05, ('dmri_tok', 'low'): 1.00e-05, ('dmri_tok', 'high'): 1.02e-05, ('dmri_tok.reserved', 'flat'): 2.43e-06, ('dmri_tok.reserved', 'peaked'): 1.83e-06, ('dmri_tok.reserved', 'low'): 1.93e-06, ('dmri_tok.reserved', 'high'): 1.54e-06, ('dpet_tok', 'flat'): 5.81e-06, ('dpet_tok', 'peaked'): 8.37e-06, ('dpet_tok', 'low'): 1.20e-05, ('dpet_tok', 'high'): 1.26e-05, ('dpet_tok.reserved', 'flat'): 1.05e-06, ('dpet_tok.reserved', 'peaked'): 2.23e-06, ('dpet_tok.reserved', 'low'): 1.07e-06, ('dpet_tok.reserved', 'high'): 1.16e-06, ('i0.dwq', 'rows'): 4.57e-07, ('i0.dwkv', 'rows'): 6.28e-06, ('i0.dwo', 'rows'): 9.12e-06, ('i0.dw1', 'rows'): 8.36e-06, ('i0.dw2', 'rows'): 6.10e-06, ('i0.small', 'b2'): 1.05e-06, ('i0.small', 'b2.reserved'): 2.27e-07, ('i0.small', 'b1'): 6.98e-07, ('i0.small', 'bo'): 8.11e-07, ('i0.small', 'bo.reserved'): 2.25e-07, ('i0.small', 'ln2_g'): 6.06e-07, ('i0.small', 'ln2_g.reserved'): 2.97e-07, ('i0.small', 'ln2_b'): 9.39e-07, ('i0.small', 'ln2_b.reserved'): 3.84e-07, ('i0.small', 'ln1_g'): 2.54e-08, ('i0.small', 'ln1_g.reserved'): 4.64e-08, ('i0.small', 'ln1_b'): 2.41e-08, ('i0.small', 'ln1_b.reserved'): 2.26e-08, ('i0.lnf', 'lnf_g'): 5.72e-08, ('i0.lnf', 'lnf_g.reserved'): 5.82e-08, ('i0.lnf', 'lnf_b'): 7.77e-08, ('i0.lnf', 'lnf_b.reserved'): 5.46e-08, ('i1.dwq', 'rows'): 6.76e-07, ('i1.dwkv', 'rows'): 3.93e-06, ('i1.dwo', 'rows'): 1.25e-05, ('i1.dw1', 'rows'): 1.19e-05, ('i1.dw2', 'rows'): 6.57e-06, ('i1.small', 'b2'): 2.70e-07, ('i1.small', 'b2.reserved'): 1.69e-07, ('i1.small', 'b1'): 4.50e-07, ('i1.small', 'bo'): 3.85e-07, ('i1.small', 'bo.reserved'): 2.31e-07, ('i1.small', 'ln2_g'): 6.48e-07, ('i1.small', 'ln2_g.reserved'): 3.38e-07, ('i1.small', 'ln2_b'): 4.32e-07, ('i1.small', 'ln2_b.reserved'): 2.91e-07, ('i1.small', 'ln1_g'): 3.97e-08, ('i1.small', 'ln1_g.reserved'): 7.66e-08, ('i1.small', 'ln1_b'): 4.29e-08, ('i1.small', 'ln1_b.reserved'): 3.52e-08, ('i1.lnf', 'lnf_g'): 6.28e-07, ('i1.lnf', 'lnf_g.reserved'): 1.15e-07, ('i1.lnf', 'lnf_b'): 3.19e-06, ('i1.lnf', 'lnf_b.reserved'): 2.19e-06},
    ((2, 216, 2, True), 4): {('cls', 'mean'): 8.49e-07, ('cls', 'max'): 1.28e-06, ('dmri_tok', 'flat'): 2.38e-05, ('dmri_tok', 'peaked'): 2.88e-05, ('dmri_tok', 'low'): 1.84e-05, ('dmri_tok', 'high'): 2.21e-05, ('dmri_tok.reserved', 'flat'): 9.28e-06, ('dmri_tok.reserved', 'peaked'): 5.16e-06, ('dmri_tok.reserved', 'low'): 4.97e-06, ('dmri_tok.reserved', 'high'): 5.85e-06, ('dpet_tok', 'flat'): 1.50e-05, ('dpet_tok', 'peaked'): 1.52e-05, ('dpet_tok', 'low'): 5.16e-05, ('dpet_tok', 'high'): 5.49e-05, ('dpet_tok.reserved', 'flat'): 3.00e-06, ('dpet_tok.reserved', 'peaked'): 3.72e-06, ('dpet_tok.reserved', 'low'): 4.07e-06, ('dpet_tok.reserved', 'high'): 4.20e-06, ('i2.dwq', 'rows'): 2.46e-07, ('i2.dwkv', 'rows'): 1.58e-06, ('i2.dwo', 'rows'): 8.54e-06, ('i2.dw1', 'rows'): 8.94e-06, ('i2.dw2', 'rows'): 5.77e-06, ('i2.small', 'b2'): 4.21e-07, ('i2.small', 'b2.reserved'): 2.31e-07, ('i2.small', 'b1'): 5.12e-07, ('i2.small', 'bo'): 4.04e-07, ('i2.small', 'bo.reserved'): 3.58e-07, ('i2.small', 'ln2_g'): 6.59e-07, ('i2.small', 'ln2_g.reserved'): 2.12e-07, ('i2.small', 'ln2_b'): 3.47e-07, ('i2.small', 'ln2_b.reserved'): 1.88e-07, ('i2.small', 'ln1_g'): 2.60e-08, ('i2.small', 'ln1_g.reserved'): 1.90e-08, ('i2.small', 'ln1_b'): 1.76e-08, ('i2.small', 'ln1_b.reserved'): 1.53e-08, ('i2.lnf', 'lnf_g'): 7.68e-07, ('i2.lnf', 'lnf_g.reserved'): 2.61e-07, ('i2.lnf', 'lnf_b'): 4.04e-07, ('i2.lnf', 'lnf_b.reserved'): 2.14e-07, ('i3.dwq', 'rows'): 4.92e-07, ('i3.dwkv', 'rows'): 1.53e-06, ('i3.dwo', 'rows'): 8.27e-06, ('i3.dw1', 'rows'): 1.31e-05, ('i3.dw2', 'rows'): 8.16e-06, ('i3.small', 'b2'): 4.12e-07, ('i3.small', 'b2.reserved'): 1.66e-07, ('i3.small', 'b1'): 5.88e-07, ('i3.small', 'bo'): 4.89e-07, ('i3.small', 'bo.reserved'): 1.88e-07, ('i3.small', 'ln2_g'): 8.15e-07, ('i3.small', 'ln2_g.reserved'): 4.20e-07, ('i3.small', 'ln2_b'): 4.90e-07, ('i3.small', 'ln2_b.reserved'): 3.08e-07, ('i3.small', 'ln1_g'): 2.54e-08, ('i3.small', 'ln1_g.reserved'): 2.71e-08, ('i3.small', 'ln1_b'): 2.42e-08, ('i3.small', 'ln1_b.reserved'): 1.15e-08, ('i3.lnf', 'lnf_g'): 1.11e-06, ('i3.lnf', 'lnf_g.reserved'): 2.70e-07, ('i3.lnf', 'lnf_b'): 6.43e-06, ('i3.lnf', 'lnf_b.reserved'): 3.88e-06, ('i0.dwq', 'rows'): 5.20e-07, ('i0.dwkv', 'rows'): 8.04e-06, ('i0.dwo', 'rows'): 1.33e-05, ('i0.dw1', 'rows'): 2.46e-05, ('i0.dw2', 'rows'): 1.22e-05, ('i0.small', 'b2'): 1.18e-06, ('i0.small', 'b2.reserved'): 5.93e-07, ('i0.small', 'b1'): 7.80e-07, ('i0.small', 'bo'): 8.41e-07, ('i0.small', 'bo.reserved'): 4.92e-07, ('i0.small', 'ln2_g'): 8.67e-07, ('i0.small', 'ln2_g.reserved'): 4.52e-07, ('i0.small', 'ln2_b'): 9.65e-07, ('i0.small', 'ln2_b.reserved'): 4.66e-07, ('i0.small', 'ln1_g'): 4.02e-08, ('i0.small', 'ln1_g.reserved'): 7.08e-08, ('i0.small', 'ln1_b'): 2.29e-08, ('i0.small', 'ln1_b.reserved'): 3.15e-08, ('i0.lnf', 'lnf_g'): 6.19e-08, ('i0.lnf', 'lnf_g.reserved'): 1.33e-07, ('i0.lnf', 'lnf_b'): 7.49e-08, ('i0.lnf', 'lnf_b.reserved'): 1.08e-07, ('i1.dwq', 'rows'): 9.35e-07, ('i1.dwkv', 'rows'): 2.62e-06, ('i1.dwo', 'rows'): 1.70e-05, ('i1.dw1', 'rows'): 3.71e-05, ('i1.dw2', 'rows'): 1.05e-05, ('i1.small', 'b2'): 6.67e-07, ('i1.small', 'b2.reserved'): 5.01e-07, ('i1.small', 'b1'): 7.29e-07, ('i1.small', 'bo'): 8.06e-07, ('i1.small', 'bo.reserved'): 6.48e-07, ('i1.small', 'ln2_g'): 1.34e-06, ('i1.small', 'ln2_g.reserved'): 4.85e-07, ('i1.small', 'ln2_b'): 8.55e-07, ('i1.small', 'ln2_b.reserved'): 4.79e-07, ('i1.small', 'ln1_g'): 9.05e-08, ('i1.small', 'ln1_g.reserved'): 1.43e-07, ('i1.small', 'ln1_b'): 4.82e-08, ('i1.small', 'ln1_b.reserved'): 1.67e-07, ('i1.lnf', 'lnf_g'): 1.72e-06, ('i1.lnf', 'lnf_g.reserved'): 5.48e-07, ('i1.lnf', 'lnf_b'): 5.52e-07, ('i1.lnf', 'lnf_b.reserved'): 3.35e-07},
    ((2, 216, 2, True), 8): {('cls', 'mean'): 2.99e-07, ('cls', 'max'): 5.73e-07, ('dmri_tok', 'flat'): 9.82e-06, ('dmri_tok', 'peaked'): 9.40e-06, ('dmri_tok', 'low'): 1.32e-05, ('dmri_tok', 'high'): 1.25e-05, ('dmri_tok.reserved', 'flat'): 2.57e-06, ('dmri_tok.reserved', 'peaked'): 1.96e-06, ('dmri_tok.reserved', 'low'): 2.47e-06, ('dmri_tok.reserved', 'high'): 2.94e-06, ('dpet_tok', 'flat'): 6.08e-06, ('dpet_tok', 'peaked'): 9.52e-06, ('dpet_tok', 'low'): 2.33e-05, ('dpet_tok', 'high'): 2.97e-05, ('dpet_tok.reserved', 'flat'): 1.28e-06, ('dpet_tok.reserved', 'peaked'): 2.07e-06, ('dpet_tok.reserved', 'low'): 1.68e-06, ('dpet_tok.reserved', 'high'): 1.52e-06, ('i2.dwq', 'rows'): 1.60e-07, ('i2.dwkv', 'rows'): 8.48e-07, ('i2.dwo', 'rows'): 3.49e-06, ('i2.dw1', 'rows'): 6.01e-06, ('i2.dw2', 'rows'): 2.97e-06, ('i2.small', 'b2'): 2.63e-07, ('i2.small', 'b2.reserved'): 1.27e-07, ('i2.small', 'b1'): 3.21e-07, ('i2.small', 'bo'): 2.19e-07, ('i2.small', 'bo.reserved'): 1.53e-07, ('i2.small', 'ln2_g'): 3.00e-07, ('i2.small', 'ln2_g.reserved'): 1.86e-07, ('i2.small', 'ln2_b'): 2.88e-07, ('i2.small', 'ln2_b.reserved'): 1.15e-07, ('i2.small', 'ln1_g'): 1.04e-08, ('i2.small', 'ln1_g.reserved'): 7.02e-09, ('i2.small', 'ln1_b'): 1.35e-08, ('i2.small', 'ln1_b.reserved'): 4.81e-09, ('i2.lnf', 'lnf_g'): 4.00e-07, ('i2.lnf', 'lnf_g.reserved'): 2.22e-07, ('i2.lnf', 'lnf_b'): 2.91e-07, ('i2.lnf', 'lnf_b.reserved'): 1.44e-07, ('i3.dwq', 'rows'): 3.12e-07, ('i3.dwkv', 'rows'): 1.06e-06, ('i3.dwo', 'rows'): 4.40e-06, ('i3.dw1', 'rows'): 7.31e-06, ('i3.dw2', 'rows'): 3.13e-06, ('i3.small', 'b2'): 3.10e-07, ('i3.small', 'b2.reserved'): 1.10e-07, ('i3.small', 'b1'): 3.92e-07, ('i3.small', 'bo'): 2.97e-07, ('i3.small', 'bo.reserved'): 1.49e-07, ('i3.small', 'ln2_g'): 4.86e-07, ('i3.small', 'ln2_g.reserved'): 3.78e-07, ('i3.small', 'ln2_b'): 3.76e-07, ('i3.small', 'ln2_b.reserved'): 2.08e-07, ('i3.small', 'ln1_g'): 2.07e-08, ('i3.small', 'ln1_g.reserved'): 9.40e-09, ('i3.small', 'ln1_b'): 1.53e-08, ('i3.small', 'ln1_b.reserved'): 6.79e-09, ('i3.lnf', 'lnf_g'): 7.24e-07, ('i3.lnf', 'lnf_g.reserved'): 2.07e-07, ('i3.lnf', 'lnf_b'): 3.71e-06, ('i3.lnf', 'lnf_b.reserved'): 1.48e-06, ('i0.dwq', 'rows'): 2.88e-07, ('i0.dwkv', 'rows'): 2.62e-06, ('i0.dwo', 'rows'): 6.85e-06, ('i0.dw1', 'rows'): 1.27e-05, ('i0.dw2', 'rows'): 5.66e-06, ('i0.small', 'b2'): 4.74e-07, ('i0.small', 'b2.reserved'): 2.31e-07, ('i0.small', 'b1'): 5.04e-07, ('i0.small', 'bo'): 4.21e-07, ('i0.small', 'bo.reserved'): 2.22e-07, ('i0.small', 'ln2_g'): 3.96e-07, ('i0.small', 'ln2_g.reserved'): 3.09e-07, ('i0.small', 'ln2_b'): 4.62e-07, ('i0.small', 'ln2_b.reserved'): 2.62e-07, ('i0.small', 'ln1_g'): 1.94e-08, ('i0.small', 'ln1_g.reserved'): 3.17e-08, ('i0.small', 'ln1_b'): 1.83e-08, ('i0.small', 'ln1_b.reserved'): 1.39e-08, ('i0.lnf', 'lnf_g'): 4.05e-08, ('i0.lnf', 'lnf_g.reserved'): 7.79e-08, ('i0.lnf', 'lnf_b'): 3.77e-08, ('i0.lnf', 'lnf_b.reserved'): 6.66e-08, ('i1.dwq', 'rows'): 5.53e-07, ('i1.dwkv', 'rows'): 2.34e-06, ('i1.dwo', 'rows'): 6.64e-06, ('i1.dw1', 'rows'): 1.62e-05, ('i1.dw2', 'rows'): 4.65e-06, ('i1.small', 'b2'): 4.91e-07, ('i1.small', 'b2.reserved'): 1.64e-07, ('i1.small', 'b1'): 5.03e-07, ('i1.small', 'bo'): 4.72e-07, ('i1.small', 'bo.reserved'): 2.28e-07, ('i1.small', 'ln2_g'): 6.85e-07, ('i1.small', 'ln2_g.reserved'): 5.19e-07, ('i1.small', 'ln2_b'): 4.41e-07, ('i1.small', 'ln2_b.reserved'): 2.87e-07, ('i1.small', 'ln1_g'): 2.78e-08, ('i1.small', 'ln1_g.reserved'): 6.93e-08, ('i1.small', 'ln1_b'): 2.80e-08, ('i1.small', 'ln1_b.reserved'): 2.97e-08, ('i1.lnf', 'lnf_g'): 1.12e-06, ('i1.lnf', 'lnf_g.reserved'): 2.07e-07, ('i1.lnf', 'lnf_b'): 4.12e-07, ('i1.lnf', 'lnf_b.reserved'): 2.62e-07},
    ((1, 225, 1, False), 4): {('cls', 'mean'): 1.59e-06, ('cls', 'max'): 9.87e-07, ('dmri_tok', 'flat'): 1.64e-05, ('dmri_tok', 'peaked'): 2.11e-05, ('dmri_tok', 'low'): 2.16e-05, ('dmri_tok', 'high'): 2.49e-05, ('dmri_tok.reserved', 'flat'): 8.17e-06, ('dmri_tok.reserved', 'peaked'): 6.58e-06, ('dmri_tok.reserved', 'low'): 6.70e-06, ('dmri_tok.reserved', 'high'): 6.25e-06, ('dpet_tok', 'flat'): 1.39e-05, ('dpet_tok', 'peaked'): 1.77e-05, ('dpet_tok', 'low'): 1.83e-05, ('dpet_tok', 'high'): 1.86e-05, ('dpet_tok.reserved', 'flat'): 4.49e-06, ('dpet_tok.reserved', 'peaked'): 2.86e-06, ('dpet_tok.reserved', 'low'): 5.14e-06, ('dpet_tok.reserved', 'high'): 3.77e-06, ('i0.dwq', 'rows'): 8.44e-07, ('i0.dwkv', 'rows'): 1.23e-05, ('i0.dwo', 'rows'): 1.29e-05, ('i0.dw1', 'rows'): 2.06e-05, ('i0.dw2', 'rows'): 1.45e-05, ('i0.small', 'b2'): 2.09e-06, ('i0.small', 'b2.reserved'): 8.64e-07, ('i0.small', 'b1'): 8.90e-07, ('i0.small', 'bo'): 1.04e-06, ('i0.small', 'bo.reserved'): 1.03e-06, ('i0.small', 'ln2_g'): 9.70e-07, ('i0.small', 'ln2_g.reserved'): 7.17e-07, ('i0.small', 'ln2_b'): 1.24e-06, ('i0.small', 'ln2_b.reserved'): 5.38e-07, ('i0.small', 'ln1_g'): 4.63e-08, ('i0.small', 'ln1_g.reserved'): 1.14e-07, ('i0.small', 'ln1_b'): 3.06e-08, ('i0.small', 'ln1_b.reserved'): 6.14e-08, ('i0.lnf', 'lnf_g'): 7.90e-08, ('i0.lnf', 'lnf_g.reserved'): 1.65e-07, ('i0.lnf', 'lnf_b'): 1.15e-07, ('i0.lnf', 'lnf_b.reserved'): 4.40e-07, ('i1.dwq', 'rows'): 1.85e-06, ('i1.dwkv', 'rows'): 3.96e-06, ('i1.dwo', 'rows'): 1.78e-05, ('i1.dw1', 'rows'): 3.57e-05, ('i1.dw2', 'rows'): 1.31e-05, ('i1.small', 'b2'): 5.61e-07, ('i1.small', 'b2.reserved'): 6.17e-07, ('i1.small', 'b1'): 1.33e-06, ('i1.small', 'bo'): 6.52e-07, ('i1.small', 'bo.reserved'): 7.50e-07, ('i1.small', 'ln2_g'): 1.87e-06, ('i1.small', 'ln2_g.reserved'): 1.45e-06, ('i1.small', 'ln2_b'): 9.93e-07, ('i1.small', 'ln2_b.reserved'): 5.34e-07, ('i1.small', 'ln1_g'): 9.69e-08, ('i1.small', 'ln1_g.reserved'): 4.84e-07, ('i1.small', 'ln1_b'): 9.06e-08, ('i1.small', 'ln1_b.reserved'): 3.25e-07, ('i1.lnf', 'lnf_g'): 6.29e-06, ('i1.lnf', 'lnf_g.reserved'): 9.76e-08, ('i1.lnf', 'lnf_b'): 2.78e-06, ('i1.lnf', 'lnf_b.reserved'): 2.62e-06},
    ((1, 225, 1, False), 8): {('cls', 'mean'): 1.37e-06, ('cls', 'max'): 5.75e-07, ('dmri_tok', 'flat'): 1.01e-05, ('dmri_tok', 'peaked'): 1.57e-05, ('dmri_tok', 'low'): 1.21e-05, ('dmri_tok', 'high'): 1.39e-05, ('dmri_tok.reserved', 'flat'): 2.84e-06, ('dmri_tok.reserved', 'peaked'): 2.60e-06, ('dmri_tok.reserved', 'low'): 2.68e-06, ('dmri_tok.reserved', 'high'): 2.64e-06, ('dpet_tok', 'flat'): 6.24e-06, ('dpet_tok', 'peaked'): 6.34e-06, ('dpet_tok', 'low'): 1.07e-05, ('dpet_tok', 'high'): 1.56e-05, ('dpet_tok.reserved', 'flat'): 1.44e-06, ('dpet_tok.reserved', 'peaked'): 9.63e-07, ('dpet_tok.reserved', 'low'): 1.22e-06, ('dpet_tok.reserved', 'high'): 1.36e-06, ('i0.dwq', 'rows'): 3.51e-07, ('i0.dwkv', 'rows'): 6.18e-06, ('i0.dwo', 'rows'): 6.22e-06, ('i0.dw1', 'rows'): 9.30e-06, ('i0.dw2', 'rows'): 1.03e-05, ('i0.small', 'b2'): 9.05e-07, ('i0.small', 'b2.reserved'): 2.65e-07, ('i0.small', 'b1'): 7.60e-07, ('i0.small', 'bo'): 6.81e-07, ('i0.small', 'bo.reserved'): 2.60e-07, ('i0.small', 'ln2_g'): 7.24e-07, ('i0.small', 'ln2_g.reserved'): 2.89e-07, ('i0.small', 'ln2_b'): 5.50e-07, ('i0.small', 'ln2_b.reserved'): 4.87e-07, ('i0.small', 'ln1_g'): 2.21e-08, ('i0.small', 'ln1_g.reserved'): 6.59e-08, ('i0.small', 'ln1_b'): 2.60e-08, ('i0.small', 'ln1_b.reserved'): 2.40e-08, ('i0.lnf', 'lnf_g'): 5.39e-08, ('i0.lnf', 'lnf_g.reserved'): 7.52e-08, ('i0.lnf', 'lnf_b'): 4.42e-08, ('i0.lnf', 'lnf_b.reserved'): 6.53e-08, ('i1.dwq', 'rows'): 7.58e-07, ('i1.dwkv', 'rows'): 3.60e-06, ('i1.dwo', 'rows'): 1.06e-05, ('i1.dw1', 'rows'): 1.27e-05, ('i1.dw2', 'rows'): 5.49e-06, ('i1.small', 'b2'): 3.53e-07, ('i1.small', 'b2.reserved'): 1.96e-07, ('i1.small', 'b1'): 4.97e-07, ('i1.small', 'bo'): 3.98e-07, ('i1.small', 'bo.reserved'): 3.22e-07, ('i1.small', 'ln2_g'): 9.74e-07, ('i1.small', 'ln2_g.reserved'): 4.15e-07, ('i1.small', 'ln2_b'): 5.32e-07, ('i1.small', 'ln2_b.reserved'): 4.64e-07, ('i1.small', 'ln1_g'): 4.13e-08, ('i1.small', 'ln1_g.reserved'): 8.27e-08, ('i1.small', 'ln1_b'): 3.21e-08, ('i1.small', 'ln1_b.reserved'): 7.16e-08, ('i1.lnf', 'lnf_g'): 1.25e-06, ('i1.lnf', 'lnf_g.reserved'): 2.51e-07, ('i1.lnf', 'lnf_b'): 3.63e-06, ('i1.lnf', 'lnf_b.reserved'): 2.41e-06},
    ((1, 256, 1, False), 4): {('cls', 'mean'): 1.02e-06, ('cls', 'max'): 6.46e-07, ('dmri_tok', 'flat'): 2.56e-05, ('dmri_tok', 'peaked'): 1.93e-05, ('dmri_tok', 'low'): 2.06e-05, ('dmri_tok', 'high'): 3.29e-05, ('dmri_tok.reserved', 'flat'): 3.80e-06, ('dmri_tok.reserved', 'peaked'): 4.50e-06, ('dmri_tok.reserved', 'low'): 6.39e-06, ('dmri_tok.reserved', 'high'): 6.53e-06, ('dpet_tok', 'flat'): 1.61e-05, ('dpet_tok', 'peaked'): 1.71e-05, ('dpet_tok', 'low'): 2.07e-05, ('dpet_tok', 'high'): 1.93e-05, ('dpet_tok.reserved', 'flat'): 5.39e-06, ('dpet_tok.reserved', 'peaked'): 3.96e-06, ('dpet_tok.reserved', 'low'): 3.69e-06, ('dpet_tok.reserved', 'high'): 5.45e-06, ('i0.dwq', 'rows'): 9.55e-07, ('i0.dwkv', 'rows'): 4.71e-06, ('i0.dwo', 'rows'): 1.39e-05, ('i0.dw1', 'rows'): 1.48e-05, ('i0.dw2', 'rows'): 9.46e-06, ('i0.small', 'b2'): 1.24e-06, ('i0.small', 'b2.reserved'): 4.43e-07, ('i0.small', 'b1'): 8.85e-07, ('i0.small', 'bo'): 8.52e-07, ('i0.small', 'bo.reserved'): 3.83e-07, ('i0.small', 'ln2_g'): 9.36e-07, ('i0.small', 'ln2_g.reserved'): 4.76e-07, ('i0.small', 'ln2_b'): 7.75e-07, ('i0.small', 'ln2_b.reserved'): 7.18e-07, ('i0.small', 'ln1_g'): 4.63e-08, ('i0.small', 'ln1_g.reserved'): 8.22e-08, ('i0.small', 'ln1_b'): 4.07e-08, ('i0.small', 'ln1_b.reserved'): 3.99e-08, ('i0.lnf', 'lnf_g'): 7.24e-08, ('i0.lnf', 'lnf_g.reserved'): 2.30e-07, ('i0.lnf', 'lnf_b'): 7.38e-08, ('i0.lnf', 'lnf_b.reserved'): 2.59e-07, ('i1.dwq', 'rows'): 9.38e-07, ('i1.dwkv', 'rows'): 4.41e-06, ('i1.dwo', 'rows'): 3.12e-05, ('i1.dw1', 'rows'): 1.79e-05, ('i1.dw2', 'rows'): 7.09e-06, ('i1.small', 'b2'): 6.40e-07, ('i1.small', 'b2.reserved'): 3.67e-07, ('i1.small', 'b1'): 8.02e-07, ('i1.small', 'bo'): 7.40e-07, ('i1.small', 'bo.reserved'): 3.69e-07, ('i1.small', 'ln2_g'): 1.76e-06, ('i1.small', 'ln2_g.reserved'): 4.17e-07, ('i1.small', 'ln2_b'): 9.17e-07, ('i1.small', 'ln2_b.reserved'): 4.78e-07, ('i1.small', 'ln1_g'): 7.11e-08, ('i1.small', 'ln1_g.reserved'): 2.85e-07, ('i1.small', 'ln1_b'): 6.33e-08, ('i1.small', 'ln1_b.reserved'): 7.07e-08, ('i1.lnf', 'lnf_g'): 2.49e-06, ('i1.lnf', 'lnf_g.reserved'): 9.53e-07, ('i1.lnf', 'lnf_b'): 3.61e-06, ('i1.lnf', 'lnf_b.reserved'): 5.22e-06},
    ((1, 256, 1, False), 8): {('cls', 'mean'): 1.01e-06, ('cls', 'max'): 3.82e-07, ('dmri_tok', 'flat'): 9.88e-06, ('dmri_tok', 'peaked'): 1.02e-05, ('dmri_tok', 'low'): 1.07e-05, ('dmri_tok', 'high'): 1.99e-05, ('dmri_tok.reserved', 'flat'): 2.46e-06, ('dmri_tok.reserved', 'peaked'): 3.12e-06, ('dmri_tok.reserved', 'low'): 3.29e-06, ('dmri_tok.reserved', 'high'): 4.20e-06, ('dpet_tok', 'flat'): 5.82e-06, ('dpet_tok', 'peaked'): 6.90e-06, ('dpet_tok', 'low'): 1.50e-05, ('dpet_tok', 'high'): 9.75e-06, ('dpet_tok.reserved', 'flat'): 1.00e-06, ('dpet_tok.reserved', 'peaked'): 1.27e-06, ('dpet_tok.reserved', 'low'): 1.40e-06, ('dpet_tok.reserved', 'high'): 9.86e-07, ('i0.dwq', 'rows'): 5.25e-07, ('i0.dwkv', 'rows'): 5.99e-06, ('i0.dwo', 'rows'): 1.07e-05, ('i0.dw1', 'rows'): 9.09e-06, ('i0.dw2', 'rows'): 6.17e-06, ('i0.small', 'b2'): 8.92e-07, ('i0.small', 'b2.reserved'): 5.86e-07, ('i0.small', 'b1'): 7.06e-07, ('i0.small', 'bo'): 5.84e-07, ('i0.small', 'bo.reserved'): 2.98e-07, ('i0.small', 'ln2_g'): 5.65e-07, ('i0.small', 'ln2_g.reserved'): 3.91e-07, ('i0.small', 'ln2_b'): 6.26e-07, ('i0.small', 'ln2_b.reserved'): 4.35e-07, ('i0.small', 'ln1_g'): 2.52e-08, ('i0.small', 'ln1_g.reserved'): 4.12e-08, ('i0.small', 'ln1_b'): 2.63e-08, ('i0.small', 'ln1_b.reserved'): 1.98e-08, ('i0.lnf', 'lnf_g'): 4.67e-08, ('i0.lnf', 'lnf_g.reserved'): 7.77e-08, ('i0.lnf', 'lnf_b'): 4.95e-08, ('i0.lnf', 'lnf_b.reserved'): 6.84e-08, ('i1.dwq', 'rows'): 7.15e-07, ('i1.dwkv', 'rows'): 3.00e-06, ('i1.dwo', 'rows'): 8.73e-06, ('i1.dw1', 'rows'): 1.04e-05, ('i1.dw2', 'rows'): 5.37e-06, ('i1.small', 'b2'): 3.24e-07, ('i1.small', 'b2.reserved'): 1.73e-07, ('i1.small', 'b1'): 6.72e-07, ('i1.small', 'bo'): 4.26e-07, ('i1.small', 'bo.reserved'): 2.21e-07, ('i1.small', 'ln2_g'): 8.16e-07, ('i1.small', 'ln2_g.reserved'): 3.14e-07, ('i1.small', 'ln2_b'): 5.61e-07, ('i1.small', 'ln2_b.reserved'): 3.56e-07, ('i1.small', 'ln1_g'): 6.04e-08, ('i1.small', 'ln1_g.reserved'): 4.95e-08, ('i1.small', 'ln1_b'): 3.35e-08, ('i1.small', 'ln1_b.reserved'): 2.47e-08, ('i1.lnf', 'lnf_g'): 7.56e-07, ('i1.lnf', 'lnf_g.reserved'): 1.39e-06, ('i1.lnf', 'lnf_b'): 3.94e-06, ('i1.lnf', 'lnf_b.reserved'): 8.03e-07},
    ((1, 257, 1, False), 4): {('cls', 'mean'): 1.97e-06, ('cls', 'max'): 1.31e-06, ('dmri_tok', 'flat'): 2.79e-05, ('dmri_tok', 'peaked'): 1.77e-05, ('dmri_tok', 'low'): 2.25e-05, ('dmri_tok', 'high'): 3.36e-05, ('dmri_tok.reserved', 'flat'): 5.77e-06, ('dmri_tok.reserved', 'peaked'): 5.60e-06, ('dmri_tok.reserved', 'low'): 5.15e-06, ('dmri_tok.reserved', 'high'): 4.79e-06, ('dpet_tok', 'flat'): 1.30e-05, ('dpet_tok', 'peaked'): 1.32e-05, ('dpet_tok', 'low'): 1.74e-05, ('dpet_tok', 'high'): 3.52e-05, ('dpet_tok.reserved', 'flat'): 4.16e-06, ('dpet_tok.reserved', 'peaked'): 3.74e-06, ('dpet_tok.reserved', 'low'): 4.14e-06, ('dpet_tok.reserved', 'high'): 3.20e-06, ('i0.dwq', 'rows'): 6.57e-07, ('i0.dwkv', 'rows'): 4.73e-06, ('i0.dwo', 'rows'): 1.09e-05, ('i0.dw1', 'rows'): 2.00e-05, ('i0.dw2', 'rows'): 7.83e-06, ('i0.small', 'b2'): 1.16e-06, ('i0.small', 'b2.reserved'): 4.39e-07, ('i0.small', 'b1'): 8.48e-07, ('i0.small', 'bo'): 9.08e-07, ('i0.small', 'bo.reserved'): 6.24e-07, ('i0.small', 'ln2_g'): 8.33e-07, ('i0.small', 'ln2_g.reserved'): 5.23e-07, ('i0.small', 'ln2_b'): 8.79e-07, ('i0.small', 'ln2_b.reserved'): 6.41e-07, ('i0.small', 'ln1_g'): 5.95e-08, ('i0.small', 'ln1_g.reserved'): 1.12e-07, ('i0.small', 'ln1_b'): 3.79e-08, ('i0.small', 'ln1_b.reserved'): 4.95e-08, ('i0.lnf', 'lnf_g'): 1.01e-07, ('i0.lnf', 'lnf_g.reserved'): 1.87e-07, ('i0.lnf', 'lnf_b'): 6.64e-08, ('i0.lnf', 'lnf_b.reserved'): 2.32e-07, ('i1.dwq', 'rows'): 9.84e-07, ('i1.dwkv', 'rows'): 5.46e-06, ('i1.dwo', 'rows'): 1.66e-05, ('i1.dw1', 'rows'): 2.85e-05, ('i1.dw2', 'rows'): 1.04e-05, ('i1.small', 'b2'): 5.36e-07, ('i1.small', 'b2.reserved'): 4.57e-07, ('i1.small', 'b1'): 1.13e-06, ('i1.small', 'bo'): 7.17e-07, ('i1.small', 'bo.reserved'): 4.08e-07, ('i1.small', 'ln2_g'): 1.41e-06, ('i1.small', 'ln2_g.reserved'): 7.17e-07, ('i1.small', 'ln2_b'): 8.58e-07, ('i1.small', 'ln2_b.reserved'): 5.84e-07, ('i1.small', 'ln1_g'): 6.15e-08, ('i1.small', 'ln1_g.reserved'): 2.53e-07, ('i1.small', 'ln1_b'): 4.61e-08, ('i1.small', 'ln1_b.reserved'): 9.49e-08, ('i1.lnf', 'lnf_g'): 1.25e-06, ('i1.lnf', 'lnf_g.reserved'): 1.95e-07, ('i1.lnf', 'lnf_b'): 7.00e-06, ('i1.lnf', 'lnf_b.reserved'): 5.84e-07},
    ((1, 257, 1, False), 8): {('cls', 'mean'): 8.55e-07, ('cls', 'max'): 3.50e-07, ('dmri_tok', 'flat'): 1.46e-05, ('dmri_tok', 'peaked'): 1.27e-05, ('dmri_tok', 'low'): 9.53e-06, ('dmri_tok', 'high'): 9.75e-06, ('dmri_tok.reserved', 'flat'): 2.45e-06, ('dmri_tok.reserved', 'peaked'): 3.32e-06, ('dmri_tok.reserved', 'low'): 1.90e-06, ('dmri_tok.reserved', 'high'): 1.70e-06, ('dpet_tok', 'flat'): 5.08e-06, ('dpet_tok', 'peaked'): 8.04e-06, ('dpet_tok', 'low'): 1.75e-05, ('dpet_tok', 'high'): 1.63e-05, ('dpet_tok.reserved', 'flat'): 1.65e-06, ('dpet_tok.reserved', 'peaked'): 1.29e-06, ('dpet_tok.reserved', 'low'): 1.14e-06, ('dpet_tok.reserved', 'high'): 1.85e-06, ('i0.dwq', 'rows'): 3.84e-07, ('i0.dwkv', 'rows'): 4.87e-06, ('i0.dwo', 'rows'): 7.33e-06, ('i0.dw1', 'rows'): 1.43e-05, ('i0.dw2', 'rows'): 6.78e-06, ('i0.small', 'b2'): 1.02e-06, ('i0.small', 'b2.reserved'): 3.26e-07, ('i0.small', 'b1'): 5.18e-07, ('i0.small', 'bo'): 6.96e-07, ('i0.small', 'bo.reserved'): 4.42e-07, ('i0.small', 'ln2_g'): 5.24e-07, ('i0.small', 'ln2_g.reserved'): 2.46e-07, ('i0.small', 'ln2_b'): 5.78e-07, ('i0.small', 'ln2_b.reserved'): 3.09e-07, ('i0.small', 'ln1_g'): 2.23e-08, ('i0.small', 'ln1_g.reserved'): 5.30e-08, ('i0.small', 'ln1_b'): 1.44e-08, ('i0.small', 'ln1_b.reserved'): 1.90e-08, ('i0.lnf', 'lnf_g'): 3.76e-08, ('i0.lnf', 'lnf_g.reserved'): 6.74e-08, ('i0.lnf', 'lnf_b'): 6.49e-08, ('i0.lnf', 'lnf_b.reserved'): 7.19e-08, ('i1.dwq', 'rows'): 9.71e-07, ('i1.dwkv', 'rows'): 5.31e-06, ('i1.dwo', 'rows'): 8.47e-06, ('i1.dw1', 'rows'): 1.18e-05, ('i1.dw2', 'rows'): 3.50e-06, ('i1.small', 'b2'): 2.89e-07, ('i1.small', 'b2.reserved'): 1.08e-07, ('i1.small', 'b1'): 6.94e-07, ('i1.small', 'bo'): 3.26e-07, ('i1.small', 'bo.reserved'): 1.55e-07, ('i1.small', 'ln2_g'): 7.81e-07, ('i1.small', 'ln2_g.reserved'): 3.02e-07, ('i1.small', 'ln2_b'): 4.71e-07, ('i1.small', 'ln2_b.reserved'): 2.37e-07, ('i1.small', 'ln1_g'): 5.06e-08, ('i1.small', 'ln1_g.reserved'): 8.24e-08, ('i1.small', 'ln1_b'): 3.91e-08, ('i1.small', 'ln1_b.reserved'): 3.18e-08, ('i1.lnf', 'lnf_g'): 1.02e-06, ('i1.lnf', 'lnf_g.reserved'): 3.01e-07, ('i1.lnf', 'lnf_b'): 5.10e-06, ('i1.lnf', 'lnf_b.reserved'): 2.34e-06},
    ((1, 496, 1, False), 4): {('cls', 'mean'): 3.08e-06, ('cls', 'max'): 1.01e-06, ('dmri_tok', 'flat'): 2.36e-05, ('dmri_tok', 'peaked'): 3.33e-05, ('dmri_tok', 'low'): 2.24e-05, ('dmri_tok', 'high'): 2.45e-05, ('dmri_tok.reserved', 'flat'): 7.11e-06, ('dmri_tok.reserved', 'peaked'): 6.78e-06, ('dmri_tok.reserved', 'low'): 6.42e-06, ('dmri_tok.reserved', 'high'): 6.38e-06, ('dpet_tok', 'flat'): 1.38e-05, ('dpet_tok', 'peaked'): 3.16e-05, ('dpet_tok', 'low'): 2.60e-05, ('dpet_tok', 'high'): 2.52e-05, ('dpet_tok.reserved', 'flat'): 4.30e-06, ('dpet_tok.reserved', 'peaked'): 4.15e-06, ('dpet_tok.reserved', 'low'): 4.52e-06, ('dpet_tok.reserved', 'high'): 5.66e-06, ('i0.dwq', 'rows'): 4.57e-07, ('i0.dwkv', 'rows'): 4.65e-06, ('i0.dwo', 'rows'): 1.09e-05, ('i0.dw1', 'rows'): 1.46e-05, ('i0.dw2', 'rows'): 1.23e-05, ('i0.small', 'b2'): 1.18e-06, ('i0.small', 'b2.reserved'): 3.94e-07, ('i0.small', 'b1'): 7.58e-07, ('i0.small', 'bo'): 7.91e-07, ('i0.small', 'bo.reserved'): 3.49e-07, ('i0.small', 'ln2_g'): 5.32e-07, ('i0.small', 'ln2_g.reserved'): 5.77e-07, ('i0.small', 'ln2_b'): 6.30e-07, ('i0.small', 'ln2_b.reserved'): 4.35e-07, ('i0.small', 'ln1_g'): 2.97e-08, ('i0.small', 'ln1_g.reserved'): 8.11e-08, ('i0.small', 'ln1_b'): 3.05e-08, ('i0.small', 'ln1_b.reserved'): 5.32e-08, ('i0.lnf', 'lnf_g'): 7.32e-08, ('i0.lnf', 'lnf_g.reserved'): 2.88e-07, ('i0.lnf', 'lnf_b'): 7.35e-08, ('i0.lnf', 'lnf_b.reserved'): 2.43e-07, ('i1.dwq', 'rows'): 8.52e-07, ('i1.dwkv', 'rows'): 2.25e-06, ('i1.dwo', 'rows'): 1.71e-05, ('i1.dw1', 'rows'): 2.35e-05, ('i1.dw2', 'rows'): 5.91e-06, ('i1.small', 'b2'): 4.94e-07, ('i1.small', 'b2.reserved'): 3.84e-07, ('i1.small', 'b1'): 6.43e-07, ('i1.small', 'bo'): 6.94e-07, ('i1.small', 'bo.reserved'): 6.92e-07, ('i1.small', 'ln2_g'): 8.46e-07, ('i1.small', 'ln2_g.reserved'): 4.46e-07, ('i1.small', 'ln2_b'): 8.51e-07, ('i1.small', 'ln2_b.reserved'): 3.71e-07, ('i1.small', 'ln1_g'): 4.88e-08, ('i1.small', 'ln1_g.reserved'): 2.73e-07, ('i1.small', 'ln1_b'): 5.37e-08, ('i1.small', 'ln1_b.reserved'): 7.39e-08, ('i1.lnf', 'lnf_g'): 1.77e-06, ('i1.lnf', 'lnf_g.reserved'): 4.24e-07, ('i1.lnf', 'lnf_b'): 6.09e-06, ('i1.lnf', 'lnf_b.reserved'): 1.13e-05},
    ((1, 496, 1, False), 8): {('cls', 'mean'): 2.04e-06, ('cls', 'max'): 2.34e-07, ('dmri_tok', 'flat'): 1.30e-05, ('dmri_tok', 'peaked'): 1.51e-05, ('dmri_tok', 'low'): 1.30e-05, ('dmri_tok', 'high'): 1.41e-05, ('dmri_tok.reserved', 'flat'): 2.35e-06, ('dmri_tok.reserved', 'peaked'): 3.23e-06, ('dmri_tok.reserved', 'low'): 2.39e-06, ('dmri_tok.reserved', 'high'): 2.14e-06, ('dpet_tok', 'flat'): 6.96e-06, ('dpet_tok', 'peaked'): 1.07e-05, ('dpet_tok', 'low'): 1.38e-05, ('dpet_tok', 'high'): 1.46e-05, ('dpet_tok.reserved', 'flat'): 1.56e-06, ('dpet_tok.reserved', 'peaked'): 1.61e-06, ('dpet_tok.reserved', 'low'): 1.82e-06, ('dpet_tok.reserved', 'high'): 1.72e-06, ('i0.dwq', 'rows'): 3.08e-07, ('i0.dwkv', 'rows'): 4.13e-06, ('i0.dwo', 'rows'): 6.38e-06, ('i0.dw1', 'rows'): 1.05e-05, ('i0.dw2', 'rows'): 9.40e-06, ('i0.small', 'b2'): 9.55e-07, ('i0.small', 'b2.reserved'): 1.90e-07, ('i0.small', 'b1'): 4.98e-07, ('i0.small', 'bo'): 6.27e-07, ('i0.small', 'bo.reserved'): 1.35e-07, ('i0.small', 'ln2_g'): 4.66e-07, ('i0.small', 'ln2_g.reserved'): 4.60e-07, ('i0.small', 'ln2_b'): 5.02e-07, ('i0.small', 'ln2_b.reserved'): 3.21e-07, ('i0.small', 'ln1_g'): 1.99e-08, ('i0.small', 'ln1_g.reserved'): 2.63e-08, ('i0.small', 'ln1_b'): 1.98e-08, ('i0.small', 'ln1_b.reserved'): 1.27e-08, ('i0.lnf', 'lnf_g'): 5.41e-08, ('i0.lnf', 'lnf_g.reserved'): 1.13e-07, ('i0.lnf', 'lnf_b'): 5.65e-08, ('i0.lnf', 'lnf_b.reserved'): 8.61e-08, ('i1.dwq', 'rows'): 3.87e-07, ('i1.dwkv', 'rows'): 4.07e-06, ('i1.dwo', 'rows'): 6.60e-06, ('i1.dw1', 'rows'): 1.14e-05, ('i1.dw2', 'rows'): 2.95e-06, ('i1.small', 'b2'): 5.12e-07, ('i1.small', 'b2.reserved'): 1.66e-07, ('i1.small', 'b1'): 4.29e-07, ('i1.small', 'bo'): 3.16e-07, ('i1.small', 'bo.reserved'): 2.69e-07, ('i1.small', 'ln2_g'): 6.09e-07, ('i1.small', 'ln2_g.reserved'): 5.54e-07, ('i1.small', 'ln2_b'): 4.76e-07, ('i1.small', 'ln2_b.reserved'): 2.92e-07, ('i1.small', 'ln1_g'): 3.19e-08, ('i1.small', 'ln1_g.reserved'): 9.50e-08, ('i1.small', 'ln1_b'): 2.68e-08, ('i1.small', 'ln1_b.reserved'): 2.48e-08, ('i1.lnf', 'lnf_g'): 9.85e-07, ('i1.lnf', 'lnf_g.reserved'): 1.93e-07, ('i1.lnf', 'lnf_b'): 7.87e-06, ('i1.lnf', 'lnf_b.reserved'): 2.25e-06},
    ((1, 497, 1, False), 4): {('cls', 'mean'): 3.31e-06, ('cls', 'max'): 4.93e-07, ('dmri_tok', 'flat'): 1.94e-05, ('dmri_tok', 'peaked'): 3.44e-05, ('dmri_tok', 'low'): 3.53e-05, ('dmri_tok', 'high'): 2.56e-05, ('dmri_tok.reserved', 'flat'): 8.97e-06, ('dmri_tok.reserved', 'peaked'): 8.46e-06, ('dmri_tok.reserved', 'low'): 7.45e-06, ('dmri_tok.reserved', 'high'): 5.54e-06, ('dpet_tok', 'flat'): 1.27e-05, ('dpet_tok', 'peaked'): 1.80e-05, ('dpet_tok', 'low'): 1.96e-05, ('dpet_tok', 'high'): 2.32e-05, ('dpet_tok.reserved', 'flat'): 3.15e-06, ('dpet_tok.reserved', 'peaked'): 4.49e-06, ('dpet_tok.reserved', 'low'): 4.31e-06, ('dpet_tok.reserved', 'high'): 3.87e-06, ('i0.dwq', 'rows'): 6.13e-07, ('i0.dwkv', 'rows'): 4.99e-06, ('i0.dwo', 'rows'): 1.22e-05, ('i0.dw1', 'rows'): 1.51e-05, ('i0.dw2', 'rows'): 8.17e-06, ('i0.small', 'b2'): 9.40e-07, ('i0.small', 'b2.reserved'): 5.64e-07, ('i0.small', 'b1'): 5.87e-07, ('i0.small', 'bo'): 8.67e-07, ('i0.small', 'bo.reserved'): 4.06e-07, ('i0.small', 'ln2_g'): 6.41e-07, ('i0.small', 'ln2_g.reserved'): 3.50e-07, ('i0.small', 'ln2_b'): 5.16e-07, ('i0.small', 'ln2_b.reserved'): 3.64e-07, ('i0.small', 'ln1_g'): 2.94e-08, ('i0.small', 'ln1_g.reserved'): 8.67e-08, ('i0.small', 'ln1_b'): 2.32e-08, ('i0.small', 'ln1_b.reserved'): 3.37e-08, ('i0.lnf', 'lnf_g'): 6.05e-08, ('i0.lnf', 'lnf_g.reserved'): 1.18e-07, ('i0.lnf', 'lnf_b'): 4.89e-08, ('i0.lnf', 'lnf_b.reserved'): 1.03e-07, ('i1.dwq', 'rows'): 7.77e-07, ('i1.dwkv', 'rows'): 3.20e-06, ('i1.dwo', 'rows'): 1.19e-05, ('i1.dw1', 'rows'): 1.71e-05, ('i1.dw2', 'rows'): 1.06e-05, ('i1.small', 'b2'): 4.59e-07, ('i1.small', 'b2.reserved'): 1.84e-07, ('i1.small', 'b1'): 4.96e-07, ('i1.small', 'bo'): 5.18e-07, ('i1.small', 'bo.reserved'): 2.14e-07, ('i1.small', 'ln2_g'): 9.81e-07, ('i1.small', 'ln2_g.reserved'): 5.17e-07, ('i1.small', 'ln2_b'): 4.88e-07, ('i1.small', 'ln2_b.reserved'): 3.26e-07, ('i1.small', 'ln1_g'): 4.98e-08, ('i1.small', 'ln1_g.reserved'): 1.14e-07, ('i1.small', 'ln1_b'): 3.98e-08, ('i1.small', 'ln1_b.reserved'): 7.69e-08, ('i1.lnf', 'lnf_g'): 2.34e-06, ('i1.lnf', 'lnf_g.reserved'): 2.22e-07, ('i1.lnf', 'lnf_b'): 1.08e-05, ('i1.lnf', 'lnf_b.reserved'): 3.98e-06},
    ((1, 497, 1, False), 8): {('cls', 'mean'): 4.03e-06, ('cls', 'max'): 3.22e-07, ('dmri_tok', 'flat'): 1.64e-05, ('dmri_tok', 'peaked'): 1.14e-05, ('dmri_tok', 'low'): 1.50e-05, ('dmri_tok', 'high'): 1.50e-05, ('dmri_tok.reserved', 'flat'): 3.86e-06, ('dmri_tok.reserved', 'peaked'): 2.50e-06, ('dmri_tok.reserved', 'low'): 1.99e-06, ('dmri_tok.reserved', 'high'): 3.41e-06, ('dpet_tok', 'flat'): 8.16e-06, ('dpet_tok', 'peaked'): 7.57e-06, ('dpet_tok', 'low'): 1.53e-05, ('dpet_tok', 'high'): 3.22e-05, ('dpet_tok.reserved', 'flat'): 1.35e-06, ('dpet_tok.reserved', 'peaked'): 1.74e-06, ('dpet_tok.reserved', 'low'): 1.41e-06, ('dpet_tok.reserved', 'high'): 1.65e-06, ('i0.dwq', 'rows'): 3.64e-07, ('i0.dwkv', 'rows'): 3.52e-06, ('i0.dwo', 'rows'): 5.80e-06, ('i0.dw1', 'rows'): 7.30e-06, ('i0.dw2', 'rows'): 6.09e-06, ('i0.small', 'b2'): 1.09e-06, ('i0.small', 'b2.reserved'): 3.78e-07, ('i0.small', 'b1'): 5.73e-07, ('i0.small', 'bo'): 7.14e-07, ('i0.small', 'bo.reserved'): 3.59e-07, ('i0.small', 'ln2_g'): 4.16e-07, ('i0.small', 'ln2_g.reserved'): 4.00e-07, ('i0.small', 'ln2_b'): 5.60e-07, ('i0.small', 'ln2_b.reserved'): 5.44e-07, ('i0.small', 'ln1_g'): 1.95e-08, ('i0.small', 'ln1_g.reserved'): 2.92e-08, ('i0.small', 'ln1_b'): 1.89e-08, ('i0.small', 'ln1_b.reserved'): 8.60e-09, ('i0.lnf', 'lnf_g'): 5.00e-08, ('i0.lnf', 'lnf_g.reserved'): 7.16e-08, ('i0.lnf', 'lnf_b'): 5.91e-08, ('i0.lnf', 'lnf_b.reserved'): 4.95e-08, ('i1.dwq', 'rows'): 4.53e-07, ('i1.dwkv', 'rows'): 3.57e-06, ('i1.dwo', 'rows'): 1.05e-05, ('i1.dw1', 'rows'): 1.08e-05, ('i1.dw2', 'rows'): 3.50e-06, ('i1.small', 'b2'): 3.85e-07, ('i1.small', 'b2.reserved'): 1.19e-07, ('i1.small', 'b1'): 3.13e-07, ('i1.small', 'bo'): 3.10e-07, ('i1.small', 'bo.reserved'): 1.69e-07, ('i1.small', 'ln2_g'): 5.86e-07, ('i1.small', 'ln2_g.reserved'): 2.58e-07, ('i1.small', 'ln2_b'): 2.98e-07, ('i1.small', 'ln2_b.reserved'): 2.03e-07, ('i1.small', 'ln1_g'): 3.56e-08, ('i1.small', 'ln1_g.reserved'): 6.19e-08, ('i1.small', 'ln1_b'): 3.14e-08, ('i1.small', 'ln1_b.reserved'): 3.28e-08, ('i1.lnf', 'lnf_g'): 1.30e-06, ('i1.lnf', 'lnf_g.reserved'): 4.88e-07, ('i1.lnf', 'lnf_b'): 5.06e-06, ('i1.lnf', 'lnf_b.reserved'): 5.90e-06},
    ((1, 512, 1, True), 4): {('cls', 'mean'): 3.28e-06, ('cls', 'max'): 6.34e-07, ('dmri_tok', 'flat'): 2.63e-05, ('dmri_tok', 'peaked'): 2.83e-05, ('dmri_tok', 'low'): 3.19e-05, ('dmri_tok', 'high'): 2.92e-05, ('dmri_tok.reserved', 'flat'): 5.11e-06, ('dmri_tok.reserved', 'peaked'): 4.75e-06, ('dmri_tok.reserved', 'low'): 5.99e-06, ('dmri_tok.reserved', 'high'): 7.41e-06, ('dpet_tok', 'flat'): 1.75e-05, ('dpet_tok', 'peaked'): 2.64e-05, ('dpet_tok', 'low'): 2.66e-05, ('dpet_tok', 'high'): 2.10e-05, ('dpet_tok.reserved', 'flat'): 4.34e-06, ('dpet_tok.reserved', 'peaked'): 6.94e-06, ('dpet_tok.reserved', 'low'): 5.74e-06, ('dpet_tok.reserved', 'high'): 6.54e-06, ('i0.dwq', 'rows'): 4.96e-07, ('i0.dwkv', 'rows'): 5.53e-06, ('i0.dwo', 'rows'): 1.32e-05, ('i0.dw1', 'rows'): 1.78e-05, ('i0.dw2', 'rows'): 9.48e-06, ('i0.small', 'b2'): 9.55e-07, ('i0.small', 'b2.reserved'): 8.04e-07, ('i0.small', 'b1'): 6.87e-07, ('i0.small', 'bo'): 6.87e-07, ('i0.small', 'bo.reserved'): 4.70e-07, ('i0.small', 'ln2_g'): 6.01e-07, ('i0.small', 'ln2_g.reserved'): 3.36e-07, ('i0.small', 'ln2_b'): 5.09e-07, ('i0.small', 'ln2_b.reserved'): 3.50e-07, ('i0.small', 'ln1_g'): 3.67e-08, ('i0.small', 'ln1_g.reserved'): 8.08e-08, ('i0.small', 'ln1_b'): 2.62e-08, ('i0.small', 'ln1_b.reserved'): 3.57e-08, ('i0.lnf', 'lnf_g'): 6.66e-08, ('i0.lnf', 'lnf_g.reserved'): 1.43e-07, ('i0.lnf', 'lnf_b'): 6.01e-08, ('i0.lnf', 'lnf_b.reserved'): 1.21e-07, ('i1.dwq', 'rows'): 8.99e-07, ('i1.dwkv', 'rows'): 2.59e-06, ('i1.dwo', 'rows'): 1.12e-05, ('i1.dw1', 'rows'): 1.58e-05, ('i1.dw2', 'rows'): 6.22e-06, ('i1.small', 'b2'): 3.15e-07, ('i1.small', 'b2.reserved'): 2.58e-07, ('i1.small', 'b1'): 6.37e-07, ('i1.small', 'bo'): 4.31e-07, ('i1.small', 'bo.reserved'): 4.23e-07, ('i1.small', 'ln2_g'): 1.17e-06, ('i1.small', 'ln2_g.reserved'): 5.07e-07, ('i1.small', 'ln2_b'): 6.39e-07, ('i1.small', 'ln2_b.reserved'): 3.89e-07, ('i1.small', 'ln1_g'): 4.87e-08, ('i1.small', 'ln1_g.reserved'): 9.10e-08, ('i1.small', 'ln1_b'): 3.45e-08, ('i1.small', 'ln1_b.reserved'): 4.28e-08, ('i1.lnf', 'lnf_g'): 1.01e-06, ('i1.lnf', 'lnf_g.reserved'): 4.66e-07, ('i1.lnf', 'lnf_b'): 9.56e-06, ('i1.lnf', 'lnf_b.reserved'): 2.61e-06},
    ((1, 512, 1, True), 8): {('cls', 'mean'): 2.50e-06, ('cls', 'max'): 2.47e-07, ('dmri_tok', 'flat'): 1.22e-05, ('dmri_tok', 'peaked'): 1.37e-05, ('dmri_tok', 'low'): 1.02e-05, ('dmri_tok', 'high'): 1.60e-05, ('dmri_tok.reserved', 'flat'): 2.82e-06, ('dmri_tok.reserved', 'peaked'): 2.19e-06, ('dmri_tok.reserved', 'low'): 2.30e-06, ('dmri_tok.reserved', 'high'): 3.58e-06, ('dpet_tok', 'flat'): 7.75e-06, ('dpet_tok', 'peaked'): 9.84e-06, ('dpet_tok', 'low'): 1.59e-05, ('dpet_tok', 'high'): 2.41e-05, ('dpet_tok.reserved', 'flat'): 1.31e-06, ('dpet_tok.reserved', 'peaked'): 1.18e-06, ('dpet_tok.reserved', 'low'): 1.36e-06, ('dpet_tok.reserved', 'high'): 2.04e-06, ('i0.dwq', 'rows'): 2.82e-07, ('i0.dwkv', 'rows'): 5.03e-06, ('i0.dwo', 'rows'): 6.24e-06, ('i0.dw1', 'rows'): 8.82e-06, ('i0.dw2', 'rows'): 8.90e-06, ('i0.small', 'b2'): 7.87e-07, ('i0.small', 'b2.reserved'): 8.91e-07, ('i0.small', 'b1'): 5.63e-07, ('i0.small', 'bo'): 6.64e-07, ('i0.small', 'bo.reserved'): 2.30e-07, ('i0.small', 'ln2_g'): 5.19e-07, ('i0.small', 'ln2_g.reserved'): 6.34e-07, ('i0.small', 'ln2_b'): 5.06e-07, ('i0.small', 'ln2_b.reserved'): 2.60e-07, ('i0.small', 'ln1_g'): 1.80e-08, ('i0.small', 'ln1_g.reserved'): 2.38e-08, ('i0.small', 'ln1_b'): 1.26e-08, ('i0.small', 'ln1_b.reserved'): 1.26e-08, ('i0.lnf', 'lnf_g'): 4.69e-08, ('i0.lnf', 'lnf_g.reserved'): 5.70e-08, ('i0.lnf', 'lnf_b'): 5.70e-08, ('i0.lnf', 'lnf_b.reserved'): 4.78e-08, ('i1.dwq', 'rows'): 6.68e-07, ('i1.dwkv', 'rows'): 2.45e-06, ('i1.dwo', 'rows'): 7.27e-06, ('i1.dw1', 'rows'): 9.72e-06, ('i1.dw2', 'rows'): 3.73e-06, ('i1.small', 'b2'): 5.06e-07, ('i1.small', 'b2.reserved'): 1.28e-07, ('i1.small', 'b1'): 6.06e-07, ('i1.small', 'bo'): 3.60e-07, ('i1.small', 'bo.reserved'): 3.36e-07, ('i1.small', 'ln2_g'): 4.48e-07, ('i1.small', 'ln2_g.reserved'): 2.29e-07, ('i1.small', 'ln2_b'): 2.94e-07, ('i1.small', 'ln2_b.reserved'): 2.69e-07, ('i1.small', 'ln1_g'): 2.01e-08, ('i1.small', 'ln1_g.reserved'): 5.24e-08, ('i1.small', 'ln1_b'): 2.26e-08, ('i1.small', 'ln1_b.reserved'): 1.99e-08, ('i1.lnf', 'lnf_g'): 8.00e-07, ('i1.lnf', 'lnf_g.reserved'): 2.71e-07, ('i1.lnf', 'lnf_b'): 7.04e-06, ('i1.lnf', 'lnf_b.reserved'): 9.21e-07},
}
# END TABLES
