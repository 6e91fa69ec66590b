"""The whole-encoder plan (snet_path.hip make_plan) pinned through its three size queries: tmf_snet_saved_bytes,
tmf_snet_bwd_scratch_bytes and tmf_snet_eval_workspace_bytes for a list of descriptors, against the numbers recorded in
tests/golden/snet_plan_sizes.json from the build BEFORE the kernel families of a block came from tmf_conv_block_algo.  Every
choice of the plan moves at least one of them: Winograd weight bytes and statistic rows, the halves of the bf16 layouts and
tensors, the x6 of the split layouts, the Winograd weight-gradient workspace.  No GPU needed.

To record anew (only when a change is MEANT to move the plan): python tests/test_host_snet_plan.py <libtmf_hip.so> > the JSON."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "snet_plan_sizes.json")

# (precision, storage_bf16) x dim x volume x batch x conv_wino (carried by the descriptor: TMF_SNET_ALGO)
PRECISIONS = (("fp32", 0), ("bf16", 0), ("bf16", 1), ("fp32x", 0))
DIMS = (32, 64, 128)
VOLUMES = ((32, 32, 32), (35, 38, 33), (96, 96, 96), (91, 109, 91))
BATCHES = (2, 8)

_PROBE = r"""
import ctypes as C, json, sys
from transmf_ad_amd import _lib
lib = C.CDLL(sys.argv[1])                       # (plain dlopen: the recorded build has fewer symbols than PROTOTYPES)
queries = ("tmf_snet_saved_bytes", "tmf_snet_bwd_scratch_bytes", "tmf_snet_eval_workspace_bytes")
for q in queries:
    getattr(lib, q).restype, getattr(lib, q).argtypes = C.c_size_t, [C.POINTER(_lib.SnetDesc)]
base = lib.tmf_snet_algo_flags() & ~_lib.snet_algo_wino(3)
out = {}
for prec, s16, dim, (D, H, W), B, wino in json.loads(sys.argv[2]):
    d = _lib.SnetDesc(B=B, D=D, H=H, W=W, dim=dim, precision=_lib.PRECISION[prec], storage_bf16=s16,
                      flags=base | _lib.snet_algo_wino(wino))
    out[f"{prec}/{s16} dim {dim} {D}x{H}x{W} B {B} conv_wino {wino}"] = [getattr(lib, q)(C.byref(d)) for q in queries]
print(json.dumps(out, indent=0))
"""


def measure(lib_path):
    cases = [(p, s, dim, v, B, w) for p, s in PRECISIONS for dim in DIMS for v in VOLUMES for B in BATCHES for w in range(4)]
    # no TMF_* option from outside; one statistic row per Winograd workgroup, whatever device (or none) the machine has
    env = {k: v for k, v in os.environ.items() if not k.startswith("TMF_")}
    env["TMF_WINO_CUS"] = "64"
    r = subprocess.run([sys.executable, "-c", _PROBE, lib_path, json.dumps(cases)], env=env, cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert len(out) == len(cases) == 384
    return out


def test_plan_sizes_did_not_move():
    from transmf_ad_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtmf_hip.so not built (python -m transmf_ad_amd.build)"
    with open(GOLDEN) as f:
        want = json.load(f)
    got = measure(_lib.LIB_PATH)
    assert sorted(got) == sorted(want)
    moved = {k: (want[k], got[k]) for k in want if got[k] != want[k]}
    assert not moved, f"{len(moved)} of {len(want)} descriptors changed size, e.g. {sorted(moved.items())[:3]}"
    assert all(min(v) > 0 for v in want.values())
    # the list is no vacuous one: conv_wino moves the fp32 plans (each step of it somewhere) and no other precision's
    heads = sorted({k.rsplit(" ", 1)[0] for k in want})
    for w in range(3):
        assert any(want[f"{h} {w}"] != want[f"{h} {w + 1}"] for h in heads if h.startswith("fp32/")), w
    # (the eval workspace of an fp32x descriptor is the fp32 plan's: tmf_snet_eval_workspace_bytes)
    assert all(want[f"{h} 0"][:2] == want[f"{h} {w}"][:2] for h in heads if not h.startswith("fp32/") for w in range(4))
    assert all(want[f"{h} 0"] == want[f"{h} {w}"] for h in heads if h.startswith("bf16/") for w in range(4))
    key = lambda p: f"{p} dim 128 96x96x96 B 8 conv_wino 3"
    assert len({tuple(want[key(p)]) for p in ("fp32/0", "bf16/0", "bf16/1", "fp32x/0")}) == 4


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    print(json.dumps(measure(sys.argv[1]), indent=0))
