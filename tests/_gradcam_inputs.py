"""Cases, fp64 formulas and tolerances of the class-activation-map tests (tests/test_host_gradcam.py,
tests/test_gpu_gradcam.py): tmf_cam of csrc/cam.hip on a channels-last activation A (B, V, C) and its gradient G.

    "gradcam":  w[b, c] = (1 / V) sum_v G[b, v, c],   cam[b, v] = sum_c w[b, c] A[b, v, c]
    "hirescam": cam[b, v] = sum_c G[b, v, c] A[b, v, c]
    RELU clamps at 0; NORMALIZE divides each sample by its maximum, zeros where that is <= 0; peak = that maximum.

fp64 for the reference; the fp32 torch formula `(A * G.mean(1, keepdim=True)).sum(-1)` on the same case is the yardstick of a
tolerance: per sample row  |kernel - fp64| <= MARGIN x D x max |fp64 row|,  D = the worst such row distance of the fp32 formula
from fp64 on that case, recorded in CAM_DISTANCE, never below CAM_FLOOR.  A row whose fp64 maximum is 0 (a sample without
gradient; an all-non-positive map after RELU) enters no distance and is judged as exact zeros.  Nothing here touches a GPU or
reads a file.

    python tests/_gradcam_inputs.py        # prints the table below"""
import torch

from _bn_inputs import COND_MARGIN

MARGIN = COND_MARGIN        # = 4: a kernel may differ from fp64 by this many distances of the fp32 formula (another order, FMA)
# A recorded distance of 0 (one voxel, eight channels: the fp32 formula can hit the fp64 value) says nothing about another
# order of the same additions: ONE correctly rounded fp32 result is already up to 2^-24 of its magnitude away from fp64, the
# division by the maximum is a second rounding.
CAM_FLOOR = 2.0 ** -23      # two unit roundoffs = one fp32 ulp of the row's maximum
METHODS = ("gradcam", "hirescam")
RELU, NORMALIZE = 1, 2      # TMF_CAM_RELU, TMF_CAM_NORMALIZE
FLAG_SETS = (0, RELU, RELU | NORMALIZE)

# (B, V, C, roles): role of each sample - "mixed": A, G and the channel means of G of mixed signs; "nonpos": A >= 0 and
# G <= 0, both maps are <= 0 everywhere; "zerograd": G == 0.  Every C the encoders of sNet(32 ... 256) have a relative of (one
# channel quad per lane, 3 of 4 lanes, both quads of the 64-lane rows), V below and above one workgroup's row pass (256 / lanes
# rows), its tile (four passes) and one column-sum workgroup's share (16 passes), 11 * 13 * 11 from the ADNI shape; the last
# case is the smallest at which a map workgroup walks more than one tile and the column sums hit their cap of 64 workgroups.
_M, _N, _Z = "mixed", "nonpos", "zerograd"
CAM_CASES = [
    (1, 1, 8, (_M,)), (3, 7, 8, (_M, _N, _Z)), (1, 216, 8, (_N,)), (3, 1573, 8, (_Z, _M, _N)),
    (3, 1, 12, (_M, _N, _Z)), (1, 27, 12, (_M,)), (3, 1000, 12, (_N, _Z, _M)),
    (1, 7, 16, (_Z,)), (3, 216, 16, (_M, _N, _Z)),
    (3, 27, 32, (_M, _Z, _N)), (1, 1573, 32, (_M,)),
    (1, 1, 64, (_N,)), (3, 1000, 64, (_M, _N, _Z)),
    (3, 7, 128, (_N, _M, _Z)), (1, 216, 128, (_M,)), (3, 1573, 128, (_M, _N, _Z)),
    (1, 27, 256, (_M,)), (3, 1000, 256, (_Z, _N, _M)),
    (3, 1, 512, (_M, _N, _Z)), (1, 1000, 512, (_M,)), (3, 1573, 512, (_M, _N, _Z)),
    (8, 4200, 256, (_M, _N, _Z, _M, _M, _N, _Z, _M)),
]


def cam_inputs(case):
    """-> (A, G) float32 (B, V, C)."""
    B, V, C, roles = case
    g = torch.Generator().manual_seed(7 + 1000003 * B + 1009 * V + C)
    A = torch.randn((B, V, C), generator=g)
    mean = torch.randn((C,), generator=g) * 0.05                      # the channel means of G: mixed signs, small against G
    G = torch.randn((B, V, C), generator=g) * 0.1 + mean
    for b, role in enumerate(roles):
        if role == "nonpos":
            A[b], G[b] = A[b].abs(), -G[b].abs()
        elif role == "zerograd":
            G[b] = 0.0
    return A, G


def _finish(cam, flags):
    if flags & RELU:
        cam = cam.clamp_min(0)
    peak, scale = cam.max(1).values, cam.abs().max(1).values
    if flags & NORMALIZE:
        live = (peak > 0).unsqueeze(1)
        cam = torch.where(live, cam / torch.where(live, peak.unsqueeze(1), torch.ones_like(cam[:, :1])), torch.zeros_like(cam))
    return cam, peak, scale


def cam_ref(A, G, method, flags):
    """fp64 -> dict(cam (B, V), weights (B, C) or None, peak (B,), scale (B,) = max |map| before the division)."""
    A, G = A.double(), G.double()
    if method == "gradcam":
        weights = G.sum(1) / A.shape[1]
        cam = torch.einsum("bc,bvc->bv", weights, A)
    else:
        weights = None
        cam = torch.einsum("bvc,bvc->bv", G, A)
    cam, peak, scale = _finish(cam, flags)
    return dict(cam=cam, weights=weights, peak=peak, scale=scale)


def cam_formula32(A, G, method, flags):
    """The torch formula in fp32, as one writes it without the kernel."""
    A, G = A.float(), G.float()
    if method == "gradcam":
        weights = G.mean(1, keepdim=True)
        cam = (A * weights).sum(-1)
        weights = weights[:, 0]
    else:
        weights = None
        cam = (A * G).sum(-1)
    cam, peak, scale = _finish(cam, flags)
    return dict(cam=cam, weights=weights, peak=peak, scale=scale)


def row_errors(got, ref64):
    """Per sample row of (B, n): (max |got - fp64| over max |fp64| of the row, or the absolute error where that is 0;
    whether the row's fp64 maximum is 0).  A non-finite element makes the error inf."""
    ref = ref64.double().reshape(ref64.shape[0], -1)
    got = got.double().reshape(ref.shape)
    err = (got - ref).abs().max(1).values
    scale = ref.abs().max(1).values
    rel = torch.where(scale > 0, err / scale.clamp_min(1e-300), err)
    rel = torch.where(torch.isfinite(got).all(1), rel, torch.full_like(rel, float("inf")))
    return rel, scale == 0


def cam_distances(case):
    """{(method, flags, "cam") / ("gradcam", 0, "weights"): the worst row distance of the fp32 formula from fp64 over the rows
    whose fp64 maximum is not 0 (0.0 where the case has no such row)}."""
    A, G = cam_inputs(case)
    res = {}
    for method in METHODS:
        for flags in FLAG_SETS:
            r64, r32 = cam_ref(A, G, method, flags), cam_formula32(A, G, method, flags)
            rel, dead = row_errors(r32["cam"], r64["cam"])
            res[(method, flags, "cam")] = float(rel[~dead].max()) if bool((~dead).any()) else 0.0
            if method == "gradcam" and flags == 0:
                rel, dead = row_errors(r32["weights"], r64["weights"])
                res[(method, 0, "weights")] = float(rel[~dead].max()) if bool((~dead).any()) else 0.0
    return res


def tolerance(case, method, flags, quantity="cam"):
    """MARGIN x the recorded distance (not below CAM_FLOOR): the relative tolerance of a row against max |fp64 row|."""
    return MARGIN * max(CAM_DISTANCE[case[:3]][(method, flags if quantity == "cam" else 0, quantity)], CAM_FLOOR)


def cam_ratios(got, ref64, case, method, flags):
    """got: dict(cam, weights or None, peak) -> {quantity: worst row error over its tolerance}; above 1 fails.  Rows whose
    fp64 maximum is 0 must be exact zeros: any other value there gives inf.  peak is one element of the map before the
    division: judged against the row's maximum magnitude with the tolerance of the undivided map."""
    res = {}
    rel, dead = row_errors(got["cam"], ref64["cam"])
    exact = (got["cam"].reshape(rel.shape[0], -1) == 0).all(1)
    rel = torch.where(dead, torch.where(exact, torch.zeros_like(rel), torch.full_like(rel, float("inf"))), rel)
    res["cam"] = float(rel.max()) / tolerance(case, method, flags)
    if got.get("weights") is not None:
        rel, dead = row_errors(got["weights"], ref64["weights"])
        exact = (got["weights"] == 0).all(1)
        rel = torch.where(dead, torch.where(exact, torch.zeros_like(rel), torch.full_like(rel, float("inf"))), rel)
        res["weights"] = float(rel.max()) / tolerance(case, "gradcam", 0, "weights")
    if got.get("peak") is not None:
        scale = ref64["scale"]
        err = (got["peak"].double() - ref64["peak"]).abs()
        rel = torch.where(scale > 0, err / scale.clamp_min(1e-300), torch.where(got["peak"] == 0, 0.0, float("inf")).double())
        rel = torch.where(torch.isfinite(got["peak"].double()), rel, torch.full_like(rel, float("inf")))
        res["peak"] = float(rel.max()) / tolerance(case, method, flags & RELU)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# recorded distances of the fp32 formula (torch 2.x CPU, fp32 against fp64); tests/test_host_gradcam.py measures them again and
# fails on a drift beyond 2x.  A value enters a tolerance through tolerance().
# ---------------------------------------------------------------------------------------------------------------------
# BEGIN TABLES
CAM_DISTANCE = {      # (B, V, C) -> {(method, flags, quantity): distance}
    (1, 1, 8): {('gradcam', 0, 'cam'): 4.61e-08, ('gradcam', 0, 'weights'): 0.00e+00, ('gradcam', 1, 'cam'): 4.61e-08, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 4.61e-08, ('hirescam', 1, 'cam'): 4.61e-08, ('hirescam', 3, 'cam'): 0.00e+00},
    (3, 7, 8): {('gradcam', 0, 'cam'): 8.20e-08, ('gradcam', 0, 'weights'): 4.26e-08, ('gradcam', 1, 'cam'): 6.12e-08, ('gradcam', 3, 'cam'): 1.05e-07, ('hirescam', 0, 'cam'): 1.22e-07, ('hirescam', 1, 'cam'): 4.69e-08, ('hirescam', 3, 'cam'): 3.34e-08},
    (1, 216, 8): {('gradcam', 0, 'cam'): 8.84e-08, ('gradcam', 0, 'weights'): 1.05e-07, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 1.07e-07, ('hirescam', 1, 'cam'): 0.00e+00, ('hirescam', 3, 'cam'): 0.00e+00},
    (3, 1573, 8): {('gradcam', 0, 'cam'): 1.26e-07, ('gradcam', 0, 'weights'): 9.20e-08, ('gradcam', 1, 'cam'): 1.03e-07, ('gradcam', 3, 'cam'): 1.29e-07, ('hirescam', 0, 'cam'): 1.14e-07, ('hirescam', 1, 'cam'): 9.13e-08, ('hirescam', 3, 'cam'): 9.24e-08},
    (3, 1, 12): {('gradcam', 0, 'cam'): 6.87e-08, ('gradcam', 0, 'weights'): 0.00e+00, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 6.87e-08, ('hirescam', 1, 'cam'): 0.00e+00, ('hirescam', 3, 'cam'): 0.00e+00},
    (1, 27, 12): {('gradcam', 0, 'cam'): 7.79e-08, ('gradcam', 0, 'weights'): 4.09e-08, ('gradcam', 1, 'cam'): 7.79e-08, ('gradcam', 3, 'cam'): 8.98e-08, ('hirescam', 0, 'cam'): 7.20e-08, ('hirescam', 1, 'cam'): 5.07e-08, ('hirescam', 3, 'cam'): 4.25e-08},
    (3, 1000, 12): {('gradcam', 0, 'cam'): 1.66e-07, ('gradcam', 0, 'weights'): 1.10e-07, ('gradcam', 1, 'cam'): 1.19e-07, ('gradcam', 3, 'cam'): 1.26e-07, ('hirescam', 0, 'cam'): 1.23e-07, ('hirescam', 1, 'cam'): 1.21e-07, ('hirescam', 3, 'cam'): 1.61e-07},
    (1, 7, 16): {('gradcam', 0, 'cam'): 0.00e+00, ('gradcam', 0, 'weights'): 0.00e+00, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 0.00e+00, ('hirescam', 1, 'cam'): 0.00e+00, ('hirescam', 3, 'cam'): 0.00e+00},
    (3, 216, 16): {('gradcam', 0, 'cam'): 9.67e-08, ('gradcam', 0, 'weights'): 9.36e-08, ('gradcam', 1, 'cam'): 7.24e-08, ('gradcam', 3, 'cam'): 7.37e-08, ('hirescam', 0, 'cam'): 1.03e-07, ('hirescam', 1, 'cam'): 7.63e-08, ('hirescam', 3, 'cam'): 6.62e-08},
    (3, 27, 32): {('gradcam', 0, 'cam'): 1.23e-07, ('gradcam', 0, 'weights'): 9.12e-08, ('gradcam', 1, 'cam'): 5.20e-08, ('gradcam', 3, 'cam'): 4.64e-08, ('hirescam', 0, 'cam'): 1.30e-07, ('hirescam', 1, 'cam'): 5.98e-08, ('hirescam', 3, 'cam'): 5.57e-08},
    (1, 1573, 32): {('gradcam', 0, 'cam'): 1.09e-07, ('gradcam', 0, 'weights'): 1.21e-07, ('gradcam', 1, 'cam'): 1.32e-07, ('gradcam', 3, 'cam'): 2.04e-07, ('hirescam', 0, 'cam'): 9.18e-08, ('hirescam', 1, 'cam'): 9.16e-08, ('hirescam', 3, 'cam'): 9.73e-08},
    (1, 1, 64): {('gradcam', 0, 'cam'): 1.28e-08, ('gradcam', 0, 'weights'): 0.00e+00, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 1.28e-08, ('hirescam', 1, 'cam'): 0.00e+00, ('hirescam', 3, 'cam'): 0.00e+00},
    (3, 1000, 64): {('gradcam', 0, 'cam'): 1.55e-07, ('gradcam', 0, 'weights'): 6.14e-08, ('gradcam', 1, 'cam'): 1.10e-07, ('gradcam', 3, 'cam'): 1.79e-07, ('hirescam', 0, 'cam'): 1.17e-07, ('hirescam', 1, 'cam'): 1.17e-07, ('hirescam', 3, 'cam'): 1.10e-07},
    (3, 7, 128): {('gradcam', 0, 'cam'): 2.34e-07, ('gradcam', 0, 'weights'): 9.03e-08, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 6.91e-08, ('hirescam', 1, 'cam'): 3.09e-09, ('hirescam', 3, 'cam'): 0.00e+00},
    (1, 216, 128): {('gradcam', 0, 'cam'): 9.86e-08, ('gradcam', 0, 'weights'): 9.58e-08, ('gradcam', 1, 'cam'): 9.95e-08, ('gradcam', 3, 'cam'): 1.22e-07, ('hirescam', 0, 'cam'): 1.29e-07, ('hirescam', 1, 'cam'): 1.06e-07, ('hirescam', 3, 'cam'): 1.17e-07},
    (3, 1573, 128): {('gradcam', 0, 'cam'): 1.41e-07, ('gradcam', 0, 'weights'): 1.31e-07, ('gradcam', 1, 'cam'): 1.20e-07, ('gradcam', 3, 'cam'): 1.20e-07, ('hirescam', 0, 'cam'): 1.39e-07, ('hirescam', 1, 'cam'): 9.99e-08, ('hirescam', 3, 'cam'): 9.98e-08},
    (1, 27, 256): {('gradcam', 0, 'cam'): 1.12e-07, ('gradcam', 0, 'weights'): 9.26e-08, ('gradcam', 1, 'cam'): 9.94e-08, ('gradcam', 3, 'cam'): 1.42e-07, ('hirescam', 0, 'cam'): 7.16e-08, ('hirescam', 1, 'cam'): 7.16e-08, ('hirescam', 3, 'cam'): 7.34e-08},
    (3, 1000, 256): {('gradcam', 0, 'cam'): 1.50e-07, ('gradcam', 0, 'weights'): 1.13e-07, ('gradcam', 1, 'cam'): 8.97e-08, ('gradcam', 3, 'cam'): 1.12e-07, ('hirescam', 0, 'cam'): 1.44e-07, ('hirescam', 1, 'cam'): 1.36e-07, ('hirescam', 3, 'cam'): 1.69e-07},
    (3, 1, 512): {('gradcam', 0, 'cam'): 3.04e-07, ('gradcam', 0, 'weights'): 0.00e+00, ('gradcam', 1, 'cam'): 0.00e+00, ('gradcam', 3, 'cam'): 0.00e+00, ('hirescam', 0, 'cam'): 3.04e-07, ('hirescam', 1, 'cam'): 0.00e+00, ('hirescam', 3, 'cam'): 0.00e+00},
    (1, 1000, 512): {('gradcam', 0, 'cam'): 1.26e-07, ('gradcam', 0, 'weights'): 8.12e-08, ('gradcam', 1, 'cam'): 1.17e-07, ('gradcam', 3, 'cam'): 1.38e-07, ('hirescam', 0, 'cam'): 1.47e-07, ('hirescam', 1, 'cam'): 1.02e-07, ('hirescam', 3, 'cam'): 1.50e-07},
    (3, 1573, 512): {('gradcam', 0, 'cam'): 1.68e-07, ('gradcam', 0, 'weights'): 9.32e-08, ('gradcam', 1, 'cam'): 1.20e-07, ('gradcam', 3, 'cam'): 1.40e-07, ('hirescam', 0, 'cam'): 1.51e-07, ('hirescam', 1, 'cam'): 1.26e-07, ('hirescam', 3, 'cam'): 1.70e-07},
    (8, 4200, 256): {('gradcam', 0, 'cam'): 2.08e-07, ('gradcam', 0, 'weights'): 1.67e-07, ('gradcam', 1, 'cam'): 1.70e-07, ('gradcam', 3, 'cam'): 2.49e-07, ('hirescam', 0, 'cam'): 1.44e-07, ('hirescam', 1, 'cam'): 1.36e-07, ('hirescam', 3, 'cam'): 2.09e-07},
}
# END TABLES


if __name__ == "__main__":
    print("CAM_DISTANCE = {      # (B, V, C) -> {(method, flags, quantity): distance}")
    for case_ in CAM_CASES:
        d_ = cam_distances(case_)
        print(f"    {case_[:3]}: {{" + ", ".join(f"{k}: {v:.2e}" for k, v in d_.items()) + "},")
    print("}")
