#!/usr/bin/env python3
"""Golden fixtures for model_ad at the reference's other `--dim` settings (options/option.py:36): dim 64 and 256 in both
head geometries of its drivers — 4 heads of dim / 4 (kfold_train_adversarial.py:78-79) and 8 heads of dim / 8
(train_adversarial.py:30-31), mlp = 4 dim.  Same recipe and contents as make_golden.py (whose run_case writes them); the
cases are added to its table here so that make_golden.py itself stays as it is.  Structured ("blobs") volumes: the B = 2
train-mode BatchNorm1d head is ill-conditioned on uniform noise (ad_full_b2).  Usage:

    python tests/golden/make_golden_dims.py [case ...]      # default: all cases below
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402


def _ad(dim, heads, size, depth=3):
    return ("model_ad", dict(dim=dim, depth=depth, heads=heads, dim_head=dim // heads, mlp_dim=4 * dim), size, 2, True,
            "blobs")


CASES = {
    "ad_d64_mid":      _ad(64, 4, (48, 48, 48)),
    "ad_d64_h8_mid":   _ad(64, 8, (48, 48, 48)),
    "ad_d256_mid":     _ad(256, 4, (48, 48, 48)),
    "ad_d256_h8_mid":  _ad(256, 8, (48, 48, 48)),
    # 96^3: N = 216 tokens per sample, 27 row tiles of 16 over B = 2
    "ad_d64_full_b2":  _ad(64, 4, (96, 96, 96)),
    "ad_d256_full_b2": _ad(256, 4, (96, 96, 96)),
}


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    make_golden.CASES.update(CASES)
    for c in (sys.argv[1:] or list(CASES)):
        make_golden.run_case(c)
