"""References of the attention-map tests (tests/test_host_attention_maps.py, tests/test_gpu_attention_maps.py):
tmf_xattn_probs of csrc/attention.hip on the cases, inputs and classes of tests/_attn_inputs.py.

    P[b, h, i, j] = softmax_j(q k^T scale),        recv[b, h, j] = (1 / N) sum_i P[b, h, i, j]

fp64 for the reference; two fp32 restatements of what the kernel computes - exp2(s c - lse) with c = scale log2(e) as a float
and lse the fp64 base-2 log-sum-exp rounded to fp32, every sum in tree and in chain order - are the yardstick of a tolerance
(ATTN_MAP_DISTANCE, as ATTN_DISTANCE).  Nothing here touches a GPU or reads a file.

    python tests/_attn_map_inputs.py        # prints the table below"""
import torch

import _attn_inputs as ai
from _attn_inputs import ATTN_CASES, MARGIN, attn_class, attn_inputs, attn_ref, floor_distance, row_error  # noqa: F401
from _attn_inputs import LOG2E, _dots
from _token_inputs import _sum_axis

MAP_WRONG = ("pad_rows", "ln_lse", "pad_div")


def map_ref(inp):
    """fp64 -> dict(probs (B, heads, N, M), recv (B, heads, M), lse (B, heads, N) base 2)."""
    q, k = inp["q"].double(), inp["k"].double()
    P = torch.softmax(_dots(q, k, torch.float64, "tree") * inp["scale"], -1)
    return dict(probs=P, recv=P.mean(-2), lse=attn_ref(inp)["lse"])


def map_restatement(inp, order, lse=None, wrong=None):
    """What the kernel computes, in fp32 with every sum in the fixed order `order`: s = q k^T (rounded products),
    p = exp2(s c - lse), recv = (sum_i p) / N.  lse: (B, heads, N) float32, default the fp64 value rounded to fp32.
    `wrong`: a deliberately WRONG result for the host test that shows the tolerances reject it -
      "pad_rows": the zero-filled query rows of the last 32-row tile counted in recv with p = 1 (s = 0, staged lse 0);
      "ln_lse":   lse taken as a natural logarithm;
      "pad_div":  recv divided by N rounded up to a multiple of 32."""
    q, k = inp["q"].float(), inp["k"].float()
    N = q.shape[2]
    npad = (N + 31) // 32 * 32
    if lse is None:
        lse = map_ref(inp)["lse"].float()
    if wrong == "ln_lse":
        lse = (lse.double() / LOG2E).float()
    c = torch.tensor(inp["scale"], dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    P = torch.exp2(_dots(q, k, torch.float32, order) * c - lse.unsqueeze(-1))
    total = _sum_axis(P, -2, order)
    if wrong == "pad_rows":
        total = total + float(npad - N)
    return dict(probs=P, recv=total / float(npad if wrong == "pad_div" else N))


def map_distances(got, ref64, case):
    """{("probs", query class): worst row_error over the query rows of the class, ("recv", "all"): worst row_error over the
    (b, h) rows}: max |got - fp64| of a row over max |fp64| of the row.  A quantity missing from `got` is left out."""
    cls = attn_class(case[2])
    res = {}
    if got.get("probs") is not None:
        rel = row_error(got["probs"], ref64["probs"])
        for c, cname in enumerate(ai.ATTN_CLASSES):
            if bool((cls == c).any()):
                res[("probs", cname)] = float(rel[:, :, cls == c].max())
    if got.get("recv") is not None:
        res[("recv", "all")] = float(row_error(got["recv"].unsqueeze(2), ref64["recv"].unsqueeze(2)).max())
    return res


def map_ratios(got, ref64, case):
    """{(quantity, class): worst row_error over its tolerance MARGIN x floor_distance(recorded distance)}; above 1 fails."""
    rec = ATTN_MAP_DISTANCE[tuple(case)]
    return {key: d / (MARGIN * floor_distance(rec[key])) for key, d in map_distances(got, ref64, case).items()}


def sum_ratios(got, case):
    """The sums that are 1 exactly - of every probs row over the keys, of every recv row over the keys - taken in fp64, as
    |sum - 1| over the tolerance of the quantity (the fp64 value of the sum, 1, in the place of max |fp64| of the row).
    Why the same tolerance holds: the error of p_ij is p_ij times the error of its base-2 logit s_ij c - lse_i (times ln 2),
    the distance of a class bounds that relative error for the row's largest entry, and every entry of a row has a logit
    error of the same size (|s c| <= |lse| + 60 wherever p matters); so |sum_j p_ij - 1| = |sum_j p_ij e_ij| <= max_j |e_ij|.
    -> {("probs", class) / ("recv", "all"): ratio}."""
    rec = ATTN_MAP_DISTANCE[tuple(case)]
    cls = attn_class(case[2])
    res = {}
    if got.get("probs") is not None:
        dev = (got["probs"].double().sum(-1) - 1).abs()
        for c, cname in enumerate(ai.ATTN_CLASSES):
            if bool((cls == c).any()):
                res[("probs", cname)] = float(dev[:, :, cls == c].max()) / (MARGIN * floor_distance(rec[("probs", cname)]))
    if got.get("recv") is not None:
        dev = (got["recv"].double().sum(-1) - 1).abs()
        res[("recv", "all")] = float(dev.max()) / (MARGIN * floor_distance(rec[("recv", "all")]))
    return res


def map_restatement_distance(case):
    """The larger of the two restatements' distances from fp64 (tree and chain order of every sum), per (quantity, class)."""
    inp = attn_inputs(case)
    r64 = map_ref(inp)
    lse = r64["lse"].float()
    a = map_distances(map_restatement(inp, "tree", lse), r64, case)
    b = map_distances(map_restatement(inp, "chain", lse), r64, case)
    return {key: max(a[key], b[key]) for key in a}


# ---------------------------------------------------------------------------------------------------------------------
# recorded restatement distances (torch 2.x CPU, fp32 against fp64); tests/test_host_attention_maps.py measures them again
# and fails on a drift beyond 2x.  A value enters a tolerance through floor_distance().
# ---------------------------------------------------------------------------------------------------------------------
# BEGIN TABLES
ATTN_MAP_DISTANCE = {      # case -> {(quantity, query class or "all"): distance}
    (1, 1, 1, 1, 0, 8): {('probs', 'flat'): 0.00e+00, ('recv', 'all'): 0.00e+00},
    (2, 3, 33, 31, 0, 8): {('probs', 'flat'): 3.55e-07, ('probs', 'peaked'): 5.25e-06, ('probs', 'low'): 2.75e-05, ('probs', 'high'): 1.76e-05, ('recv', 'all'): 1.87e-06},
    (1, 2, 65, 129, 0, 16): {('probs', 'flat'): 6.66e-07, ('probs', 'peaked'): 1.32e-05, ('probs', 'low'): 2.10e-05, ('probs', 'high'): 2.07e-05, ('recv', 'all'): 2.54e-06},
    (1, 1, 64, 512, 0, 32): {('probs', 'flat'): 6.28e-07, ('probs', 'peaked'): 1.06e-05, ('probs', 'low'): 4.66e-05, ('probs', 'high'): 4.66e-05, ('recv', 'all'): 3.70e-06},
    (1, 1, 70, 513, 0, 32): {('probs', 'flat'): 7.20e-07, ('probs', 'peaked'): 7.93e-06, ('probs', 'low'): 4.00e-05, ('probs', 'high'): 4.57e-05, ('recv', 'all'): 1.95e-06},
    (2, 2, 40, 257, 0, 64): {('probs', 'flat'): 1.04e-06, ('probs', 'peaked'): 2.38e-05, ('probs', 'low'): 4.58e-05, ('probs', 'high'): 4.88e-05, ('recv', 'all'): 7.19e-06},
    (1, 2, 257, 40, 0, 64): {('probs', 'flat'): 7.81e-07, ('probs', 'peaked'): 2.65e-05, ('probs', 'low'): 5.81e-05, ('probs', 'high'): 5.81e-05, ('recv', 'all'): 1.56e-06},
    (1, 1, 513, 70, 0, 16): {('probs', 'flat'): 6.65e-07, ('probs', 'peaked'): 1.32e-05, ('probs', 'low'): 3.14e-05, ('probs', 'high'): 2.08e-05, ('recv', 'all'): 1.23e-06},
    (1, 4, 216, 216, 0, 32): {('probs', 'flat'): 9.94e-07, ('probs', 'peaked'): 1.59e-05, ('probs', 'low'): 6.36e-05, ('probs', 'high'): 4.97e-05, ('recv', 'all'): 4.05e-06},
    (1, 2, 37, 1, 1, 8): {('probs', 'flat'): 2.24e-07, ('probs', 'peaked'): 2.62e-06, ('probs', 'low'): 2.11e-05, ('probs', 'high'): 1.40e-05, ('recv', 'all'): 1.67e-06},
    (2, 2, 50, 33, 30, 16): {('probs', 'flat'): 3.56e-07, ('probs', 'peaked'): 7.93e-06, ('probs', 'low'): 2.41e-05, ('probs', 'high'): 2.75e-05, ('recv', 'all'): 3.11e-06},
    (1, 1, 64, 255, 2, 64): {('probs', 'flat'): 6.98e-07, ('probs', 'peaked'): 2.11e-05, ('probs', 'low'): 4.32e-05, ('probs', 'high'): 3.46e-05, ('recv', 'all'): 2.29e-06},
    (1, 4, 216, 216, 216, 32): {('probs', 'flat'): 1.46e-06, ('probs', 'peaked'): 1.32e-05, ('probs', 'low'): 6.16e-05, ('probs', 'high'): 5.65e-05, ('recv', 'all'): 2.81e-06},
}
# END TABLES


if __name__ == "__main__":
    print("ATTN_MAP_DISTANCE = {      # case -> {(quantity, query class or \"all\"): distance}")
    for case_ in ATTN_CASES:
        d_ = map_restatement_distance(case_)
        print(f"    {case_}: {{" + ", ".join(f"{k}: {v:.2e}" for k, v in d_.items()) + "},")
    print("}")
