"""Inputs and host models of the region-Shapley tests (tests/test_host_shap.py, tests/test_gpu_shap.py): the size table and the
coalition sampler restated from include/tmf_hip.h on the host Philox model (_token_inputs.philox4x32), the integer Gram matrix,
the fp64 KKT reference of the constrained fit, brute-force Shapley values, the volumes and atlases, and the case lists."""
import functools
import itertools
import math

import numpy as np
import torch

from _token_inputs import philox4x32

PLAYERS = (2, 3, 31, 32, 33, 64, 65, 257, 1024)         # word seams, more than one pass of 256 lanes, the limit
TABLE_PLAYERS = (2, 3, 4, 33, 232, 1024)
COALITION_COUNTS = (1, 2, 33, 66)
GRAM_COUNTS = (1, 31, 33, 100)                          # one partial block of 32 coalitions ... three blocks and a partial one
GRAM_BATCHES = (1, 3, 9)
SOLVE_PLAYERS = (2, 3, 33, 116, 257)                    # inside one panel of 32 ... nine panels, the last one partial
SEEDS = (0xDEADBEEF12345678, (7 << 32) | 1)             # both with a non-zero high word
SOLVE_MULTIPLE = 16.0                                   # include/tmf_hip.h: |phi - ref| <= 16 P 2^-53 cond_2(M) max|ref|
U = 2.0 ** -53


def words_of(P):
    return (P + 31) // 32


def size_table(P):
    """thr[t] = min(2^32 - 1, floor(2^32 F_{t+1})), F_s = the ascending fp64 partial sum of w_r = 1 / (r (P - r)) over the total."""
    w = [np.float64(1.0) / (np.float64(r) * np.float64(P - r)) for r in range(1, P)]
    total = np.float64(0.0)
    for x in w:
        total = total + x
    thr, part = [], np.float64(0.0)
    for t in range(P - 2):
        part = part + w[t]
        thr.append(min(2 ** 32 - 1, int(math.floor(np.float64(4294967296.0) * (part / total)))))
    return np.asarray(thr, dtype=np.uint64)


def coalition_bits(P, paired, seed, m0, N):
    """The header restated row by row -> (N, P) bool: key (seed_lo ^ 0x53484150, seed_hi ^ 0x636F616C); k = m >> 1 (paired) or
    m; u = word 0 of counter (0, k, 1, 0), s = 1 + #{thr <= u}; key_i = word i & 3 of counter (i >> 2, k, 0, 0); i is a member
    iff fewer than s players j have (key_j, j) < (key_i, i); an odd m of a pair is the complement."""
    key = ((seed & 0xFFFFFFFF) ^ 0x53484150, (seed >> 32) ^ 0x636F616C)
    thr = size_table(P)
    nq = (P + 3) // 4
    z = np.zeros((N, P), bool)
    for r in range(N):
        m = m0 + r
        k = m >> 1 if paired else m
        u = philox4x32([(0, k, 1, 0)], key)[0][0]
        s = 1 + int((thr <= u).sum())
        ctr = np.stack([np.arange(nq), np.full(nq, k), np.zeros(nq, np.int64), np.zeros(nq, np.int64)], 1)
        keys = philox4x32(ctr, key).reshape(-1)[:P]
        idx = np.arange(P)
        less = (keys[None, :] < keys[:, None]) | ((keys[None, :] == keys[:, None]) & (idx[None, :] < idx[:, None]))
        row = less.sum(1) < s
        z[r] = ~row if paired and m & 1 else row
    return z


def pack(z):
    """(N, P) bool -> (N, Wd) int32 tensor: player i is bit i & 31 of word i >> 5, the padding bits 0."""
    N, P = z.shape
    Wd = words_of(P)
    bits = np.zeros((N, Wd * 32), np.int64)
    bits[:, :P] = z
    words = (bits.reshape(N, Wd, 32) << np.arange(32, dtype=np.int64)).sum(2)
    return torch.from_numpy(words.astype(np.uint32).view(np.int32))


def unpack(coal, P):
    """(N, Wd) int32 tensor -> (N, P) bool array, and the padding bits (N, Wd*32 - P)."""
    w = coal.cpu().numpy().view(np.uint32).astype(np.int64)
    bits = ((w[:, :, None] >> np.arange(32)) & 1).reshape(w.shape[0], -1).astype(bool)
    return bits[:, :P], bits[:, P:]


@functools.lru_cache(maxsize=None)
def coalitions(P, paired, seed, m0, N):
    """(N, Wd) int32 of the host model; never modified."""
    return pack(coalition_bits(P, paired, seed, m0, N))


def gram_reference(z, scores, offset):
    """z (N, P) bool, scores (B, N) float32, offset (B,) float32 -> (A (P, P) int64 exact, rhs (B, P) float64 by an ascending
    chain, the bound N 2^-53 sum_m |y_m| per sample)."""
    zf = z.astype(np.float64)                                       # counts below 2^53: the float64 product is exact
    y = scores.numpy().astype(np.float64) - offset.numpy().astype(np.float64)[:, None]
    rhs = np.zeros((y.shape[0], z.shape[1]))
    for m in range(z.shape[0]):
        rhs[:, z[m]] = rhs[:, z[m]] + y[:, m:m + 1]
    return (zf.T @ zf).astype(np.int64), rhs, z.shape[0] * U * np.abs(y).sum(1)


def kkt(A, rhs, delta, ridge=0.0):
    """min |y - Z phi|^2 + ridge |phi|^2 subject to sum phi = delta through its KKT system [[M, 1], [1^T, 0]] in numpy float64
    -> phi (B, P)."""
    P = A.shape[0]
    K = np.zeros((P + 1, P + 1))
    K[:P, :P] = np.asarray(A, dtype=np.float64) + ridge * np.eye(P)
    K[:P, P] = K[P, :P] = 1.0
    r = np.concatenate([np.asarray(rhs, dtype=np.float64), np.asarray(delta, dtype=np.float64)[:, None]], 1)
    return np.linalg.solve(K, r.T).T[:, :P]


def solve_bound(A, ridge, ref):
    """(B,): SOLVE_MULTIPLE * P * 2^-53 * cond_2(M) * max|ref|, and cond_2(M) (M is symmetric: the ratio of its extreme
    eigenvalues in magnitude)."""
    lam = np.abs(np.linalg.eigvalsh(np.asarray(A, dtype=np.float64) + ridge * np.eye(A.shape[0])))
    cond = lam.max() / lam.min()
    return SOLVE_MULTIPLE * A.shape[0] * U * cond * np.abs(ref).max(1), cond


def brute_force_shapley(v, P):
    """v: a function of a tuple of 0 / 1 of length P -> (P,) exact Shapley values by the subset formula."""
    phi = np.zeros(P)
    val = {s: v(s) for s in itertools.product((0, 1), repeat=P)}
    for i in range(P):
        for s, x in val.items():
            if s[i]:
                continue
            n = sum(s)
            w = math.factorial(n) * math.factorial(P - n - 1) / math.factorial(P)
            t = s[:i] + (1,) + s[i + 1:]
            phi[i] += w * (val[t] - x)
    return phi


@functools.lru_cache(maxsize=None)
def scores_for(B, N, seed=5):
    """scores (B, N) and offset (B,) float32 of both signs; never modified."""
    g = torch.Generator().manual_seed(seed + 17 * B + N)
    return torch.randn((B, N), generator=g), torch.randn((B,), generator=g)


@functools.lru_cache(maxsize=None)
def fit_case(P, B, seed=SEEDS[0]):
    """A well-posed fit for the solve tests: N = 4 P + 64 paired coalitions, a game that is additive plus noise.
    -> (A (P, P) int32 tensor, rhs (B, P) float64 tensor, delta (B,) float64 tensor); never modified."""
    N = 4 * P + 64
    z = coalition_bits(P, True, seed, 0, N) if P <= 257 else unpack(_fast_rows(P, seed, N), P)[0]
    g = np.random.default_rng(P * 131 + B)
    a = g.standard_normal((B, P))
    y = a @ z.T.astype(np.float64) + 0.05 * g.standard_normal((B, N))
    zf = z.astype(np.float64)                                       # counts below 2^53: the float64 product is exact
    return (torch.from_numpy((zf.T @ zf).astype(np.int32)), torch.from_numpy(y @ zf), torch.from_numpy(a.sum(1) + 0.01))


def _fast_rows(P, seed, N):
    from transmf_ad_amd import ops
    return ops.shap_coalitions_torch(P, True, seed, 0, N)          # (checked against coalition_bits by the host tests)


@functools.lru_cache(maxsize=None)
def volumes(size, B=3, seed=3):
    """vol (B, 1, D, H, W) in [0.5, 1.5), fill (B,) and a base volume of vol's shape; never modified."""
    g = torch.Generator().manual_seed(seed + size[0] * 131 + size[2])
    vol = torch.rand((B, 1) + tuple(size), generator=g) + 0.5
    fill = torch.tensor([0.25, -1.5, 3.0][:B])
    base = torch.rand((B, 1) + tuple(size), generator=g) * 2 - 1
    return vol, fill, base


@functools.lru_cache(maxsize=None)
def labels_for(size, R, seed=11):
    """(D, H, W) int32 with every label of 0..R and the labels R + 1 and -1 (which play for nobody); never modified."""
    g = torch.Generator().manual_seed(seed + R + size[2])
    lab = torch.randint(-1, R + 2, tuple(size), generator=g, dtype=torch.int32)
    flat = lab.view(-1)
    n = min(R + 3, flat.numel())
    flat[:n] = torch.arange(-1, R + 2, dtype=torch.int32)[:n]
    return lab


def block_atlas(size, n=3):
    """(D, H, W) int32: n x n x n blocks labelled 1 .. n^3, no background."""
    idx = [torch.div(torch.arange(s) * n, s, rounding_mode="floor") for s in size]
    return ((idx[0].view(-1, 1, 1) * n + idx[1].view(1, -1, 1)) * n + idx[2].view(1, 1, -1) + 1).to(torch.int32)
