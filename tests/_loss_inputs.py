"""Inputs of the FALoss / SupConLoss fixtures (tests/golden/loss_*.npz), reproducible from a few integers.  Shared by
tests/golden/make_golden_losses.py and the tests."""
import numpy as np

FA_SEED = 11
# name: (B, C, spatial)
FA_CASES = {
    "loss_fa_b2_c128_6":    (2, 128, (6, 6, 6)),
    "loss_fa_b8_c128_6":    (8, 128, (6, 6, 6)),
    "loss_fa_b2_c64_adni":  (2, 64, (5, 6, 5)),          # the ADNI token grid: N = 150, ragged
    "loss_fa_b2_c256_4":    (2, 256, (4, 4, 4)),
    "loss_fa_b1_c32_345":   (1, 32, (3, 4, 5)),
    "loss_fa_b2_c128_12":   (2, 128, (12, 12, 12)),
    "loss_fa_b1_c64_16":    (1, 64, (16, 16, 16)),
    "loss_fa_b1_c64_24":    (1, 64, (24, 24, 24)),       # N = 13 824
}


def fa_inputs(B, C, spatial, seed=FA_SEED):
    """Two encoder-like maps (LeakyReLU-shaped values, the second correlated with the first), float32 (B, C) + spatial."""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal((B, C) + tuple(spatial)).astype(np.float32)
    a = np.where(a > 0, a, np.float32(0.01) * a)
    b0 = rs.standard_normal((B, C) + tuple(spatial)).astype(np.float32)
    b0 = np.where(b0 > 0, b0, np.float32(0.01) * b0)
    b = (np.float32(0.7) * a + np.float32(0.3) * b0).astype(np.float32)
    return a.astype(np.float32), b


def fa_int_inputs(B, C, spatial, seed=5):
    """Integer-valued maps in [-3, 3]: every product and sum of FALoss is exact in fp32."""
    rs = np.random.RandomState(seed)
    shape = (B, C) + tuple(spatial)
    a = rs.randint(-3, 4, shape).astype(np.float32)
    b = rs.randint(-3, 4, shape).astype(np.float32)
    return a, b


SC_SEED = 3
# name: (bs, views, d, positives 'labels' | 'mask' | 'none', contrast_mode, feature shape handed to the loss)
SC_CASES = {
    "loss_sc_lab_8":     (8, 2, 128, "labels", "all", None),
    "loss_sc_lab_16":    (16, 2, 128, "labels", "all", None),
    "loss_sc_lab_64":    (64, 2, 128, "labels", "all", None),       # 128 rows: the kernel's edge
    "loss_sc_lab_5x3":   (5, 3, 40, "labels", "all", None),
    "loss_sc_mask_8":    (8, 2, 128, "mask", "all", None),
    "loss_sc_simclr_8":  (8, 2, 128, "none", "all", None),
    "loss_sc_one_8":     (8, 2, 128, "labels", "one", None),
    "loss_sc_4d_8":      (8, 2, 32, "labels", "all", (8, 2, 4, 8)),
}


def sc_inputs(bs, views, d, positives, shape=None, seed=SC_SEED):
    """(features float32, labels int64 | None, mask float32 | None): unit-norm embeddings, binary labels; the mask case
    has an asymmetric random mask with a unit diagonal (every anchor keeps a positive: its other view)."""
    rs = np.random.RandomState(seed)
    f = rs.standard_normal((bs, views, d))
    f = (f / np.linalg.norm(f, axis=2, keepdims=True)).astype(np.float32)
    labels = rs.randint(0, 2, bs).astype(np.int64)
    mask = None
    if positives == "mask":
        mask = (rs.rand(bs, bs) > 0.5).astype(np.float32)
        np.fill_diagonal(mask, 1.0)
    if shape is not None:
        f = f.reshape(shape)
    return f, (labels if positives == "labels" else None), mask
