"""tmf_conv_block_algo — the one rule for the kernel family of an encoder block per direction — against transcriptions of the
two rules it replaced: the block-by-block one of ops.ConvBnActPool (the more general) over a grid of channel counts, and
the one of snet_path.hip make_plan for the seven blocks of every dim the one-call entries accept up to 512.  "conv_wino" is
process state, so each of its values is probed in a fresh child process (as tests/test_host_options.py does).  No GPU needed."""
import json
import os
import subprocess
import sys

import pytest

from transmf_ad_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, BF16P, FP32X = _lib.PREC_FP32, _lib.PREC_BF16, _lib.PREC_FP32X
DIRECT, WINO, BF16, SPLIT = _lib.CONV_DIRECT, _lib.CONV_WINO, _lib.CONV_BF16, _lib.CONV_SPLIT
CH = (1, 4, 8, 12, 16, 24, 32, 40, 64, 96, 128, 256)
DIMS = tuple(range(32, 513, 32))

_PROBE = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
wino, ch, shapes = int(sys.argv[2]), json.loads(sys.argv[3]), json.loads(sys.argv[4])
assert lib.tmf_set_option(b"conv_wino", wino) == 0 and lib.tmf_conv_wino_mode() == wino
print(json.dumps(dict(
    ok=[[lib.tmf_conv3d_wino_ok(a, b) for b in ch] for a in ch], wok=[[lib.tmf_conv3d_wgrad_wino_ok(a, b) for b in ch] for a in ch],
    algo=[lib.tmf_conv_block_algo(*s) for s in shapes], bad=lib.tmf_conv_block_algo(7, 8, 8, 3))))
"""


def _blocks(dim):
    q, h = dim // 4, dim // 2
    return [(ci, co, k) for ci, co, k in zip((1, q, q, h, h, dim, 2 * dim), (q, q, h, h, dim, 2 * dim, dim), (3,) * 6 + (1,))]


def _fields(a):
    return a & 15, (a >> 4) & 15, (a >> 8) & 15


def _ops_rule(prec, cin, cout, k, wino, ok, wok):
    """ops.ConvBnActPool.forward / backward before the query: (forward, data gradient, weight gradient)."""
    bf16 = prec if (prec != FP32 and k == 3 and cin % 8 == 0 and cin > 1) else None
    w = wino if (bf16 is None and k == 3 and cin > 1) else 0
    wino_f, wino_d, wino_w = w >= 2 and ok(cin, cout), w >= 1 and ok(cout, cin), w >= 3 and wok(cin, cout)
    fwd = BF16 if bf16 == BF16P else SPLIT if bf16 == FP32X else WINO if wino_f else DIRECT
    dgr = (BF16 if bf16 == BF16P and cout % 8 == 0 else SPLIT if bf16 == FP32X and cout % 8 == 0 else WINO if wino_d else DIRECT)
    wgr = BF16 if bf16 == BF16P else WINO if wino_w else DIRECT
    return fwd, dgr, wgr


def _plan_rule(prec, cin, cout, k, wino, ok, wok):
    """snet_path.hip make_plan's five booleans before the query, as its launches read them."""
    bf = prec == BF16P and k == 3 and cin > 1 and cin % 8 == 0
    sp = prec == FP32X and k == 3 and cin > 1 and cin % 8 == 0 and cout % 8 == 0
    w = wino if (prec == FP32 and k == 3 and cin > 1) else 0
    wgf, wgd, wgw = w >= 2 and ok(cin, cout), w >= 1 and ok(cout, cin), w >= 3 and wok(cin, cout)
    return (BF16 if bf else SPLIT if sp else WINO if wgf else DIRECT, BF16 if bf else SPLIT if sp else WINO if wgd else DIRECT,
            BF16 if bf else WINO if wgw else DIRECT)


@pytest.mark.parametrize("wino", [0, 1, 2, 3])
def test_block_algo_equals_the_two_rules_it_replaced(wino):
    assert os.path.exists(_lib.LIB_PATH), "libtmf_hip.so not built (python -m transmf_ad_amd.build)"
    grid = [(p, ci, co, k) for p in (FP32, BF16P, FP32X) for ci in CH for co in CH for k in (1, 3)]
    enc = [(p, ci, co, k) for p in (FP32, BF16P, FP32X) for dim in DIMS for ci, co, k in _blocks(dim)]
    chans = sorted(set(CH) | {c for _p, ci, co, _k in enc for c in (ci, co)})
    env = {k: v for k, v in os.environ.items() if not k.startswith("TMF_")}
    r = subprocess.run([sys.executable, "-c", _PROBE, _lib.LIB_PATH, str(wino), json.dumps(chans), json.dumps(grid + enc)], env=env,
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    ix = {c: i for i, c in enumerate(chans)}
    ok = lambda a, b: bool(out["ok"][ix[a]][ix[b]])
    wok = lambda a, b: bool(out["wok"][ix[a]][ix[b]])
    assert out["bad"] == -1 and len(out["algo"]) == len(grid) + len(enc)
    for s, a in zip(grid, out["algo"][:len(grid)]):
        assert a >= 0 and a >> 12 == 0 and _fields(a) == _ops_rule(*s, wino, ok, wok), (s, _fields(a))
    seen = set()
    for s, a in zip(enc, out["algo"][len(grid):]):
        assert _fields(a) == _plan_rule(*s, wino, ok, wok) == _ops_rule(*s, wino, ok, wok), (s, _fields(a))
        seen.add(_fields(a))
    # the grid is no vacuous one: every family shows up in every direction it can take
    want = {(DIRECT, DIRECT, DIRECT), (BF16, BF16, BF16), (SPLIT, SPLIT, DIRECT)}
    want |= {(DIRECT, WINO, DIRECT)} if wino == 1 else set()
    want |= {(WINO, DIRECT, DIRECT)} if wino >= 2 else set()            # block dim/4 -> dim/2 at dim 64: 16 -> 32
    want |= {(WINO, WINO, DIRECT)} if wino == 2 else set()
    want |= {(WINO, WINO, WINO)} if wino == 3 else set()
    assert want <= seen, (want - seen)
    mixed = {_fields(a) for s, a in zip(grid, out["algo"]) if s[3] == 3}
    assert (BF16, DIRECT, BF16) in mixed and (SPLIT, DIRECT, DIRECT) in mixed          # cout % 8 != 0: off make_plan's domain
