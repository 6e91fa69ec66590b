"""bench.py end to end on the GPU: a plain run is the headline line alone."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_is_the_headline_alone(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` sets up, warms up, times, dumps and prints: the contract keys, no numerics
    gate, CPU baseline, `also` records or per-launch roofline, and at most 30 s outside its K + W steps."""
    steps, warmup = 3, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path / "d")], capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-4000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["metric"] == "volume-pairs/sec fwd+bwd(+Adam), 96^3 MRI+PET batch=8 per GPU"
    assert out["unit"] == "volume-pairs/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == steps and out["warmup"] == warmup and out["n_gpus"] == 1
    assert out["value"] > 0 and abs(out["value"] * out["ms_per_step"] / 8e3 - 1) < 1e-2
    assert out["cpu_baseline"] is None and "numerics_gate" not in out and "also" not in out
    assert set(out["roofline"]) == {"whole_step"}
    assert np.isfinite(np.load(tmp_path / "d" / "loss.npy")) and np.load(tmp_path / "d" / "logits.npy").shape == (8, 2)
    assert wall - (steps + warmup) * out["ms_per_step"] / 1e3 < 30.0
