#!/usr/bin/env python3
"""Golden fixtures for model_ad with the fusion block's Dropout ACTIVE (options/option.py:39 --dropout; networks.py:131,133,
153) at the reference's other `--dim` settings (options/option.py:36): dim 64 with 4 heads of 16 (kfold_train_adversarial.py:
78-79) and dim 256 with 8 heads of 32 (train_adversarial.py:30-31), mlp = 4 dim.  Same recipe as `ad_mid_drop`: the reference
is built with dropout 0.3 and every Transformer Dropout module is forced to the regenerable masks of
oracle/params.make_fusion_masks (make_golden.run_case does both).  The cases are added to make_golden.py's table here so that
make_golden.py and make_golden_dims.py stay as they are.  Usage:

    python tests/golden/make_golden_dims_drop.py [case ...]      # default: all cases below
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden  # noqa: E402


def _ad_drop(dim, heads, size, p=0.3, depth=3):
    return ("model_ad", dict(dim=dim, depth=depth, heads=heads, dim_head=dim // heads, mlp_dim=4 * dim), size, 2, True,
            "blobs", p)


CASES = {
    "ad_d64_mid_drop":     _ad_drop(64, 4, (48, 48, 48)),
    "ad_d256_h8_mid_drop": _ad_drop(256, 8, (48, 48, 48)),
}


if __name__ == "__main__":
    torch.set_num_threads(os.cpu_count())
    make_golden.CASES.update(CASES)
    for c in (sys.argv[1:] or list(CASES)):
        make_golden.run_case(c)
