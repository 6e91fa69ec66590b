"""Inputs and host models of the RISE tests (tests/test_host_rise.py, tests/test_gpu_rise.py): the geometries, the node grids
and shifts restated from include/tmf_hip.h on a host Philox model (_token_inputs.philox4x32), the mask formula restated voxel
by voxel in numpy float32, the volumes, fills, scores and chunkings, and the two error bounds of the header."""
import functools

import numpy as np
import torch

from _token_inputs import philox4x32

# (size, cells): the smallest geometries that still reach every branch of csrc/rise.hip
GEOMETRIES = [
    ((5, 7, 9), (2, 3, 4)),         # odd extents, V % 4 != 0: the scalar path
    ((12, 10, 11), (4, 3, 5)),      # mixed cell sizes
    ((8, 8, 8), (8, 8, 8)),         # cell 1: every shift 0, every weight 0 or 1
    ((6, 6, 13), (1, 1, 2)),        # one cell per axis
    ((16, 16, 32), (4, 4, 4)),      # the 16-byte path; V = 8 tiles of 1024 voxels, a lane's run of 4 crosses cells inside W
    ((14, 14, 14), (14, 14, 14)),   # 16^3 = 4096 node bytes: the largest grid the accumulate kernel stages in LDS
    ((15, 15, 15), (15, 15, 15)),   # 17^3 = 4913 node bytes: the accumulate kernel reads the nodes from global memory
]
# one more for the accumulate kernel alone: more than RISE_ACC_MAX_TILES = 2048 tiles of RISE_TILE = 1024 voxels, so that the
# workgroups stride to a second tile; 129 * 128 * 129 voxels are 2081 tiles, the last one not full
STRIDING = ((129, 128, 129), (3, 2, 2))
SEEDS = (1, 0xDEADBEEF12345678, 77)           # one above 2^32
P = 0.5
MASKS = 11                                    # odd: the halves differ in length
F32 = np.float32


def geom_id(g):
    return "x".join(map(str, g[0])) + "-" + "x".join(map(str, g[1]))


def geometry(size, cells):
    """-> (cell, nodes, G) as the header defines them."""
    cell = tuple(-(-S // s) for S, s in zip(size, cells))
    nodes = tuple(s + 2 for s in cells)
    return cell, nodes, nodes[0] * nodes[1] * nodes[2]


def masks_model(size, cells, p, seed, m0, N):
    """The header restated: key (seed_lo ^ 0x52495345, seed_hi ^ 0x6D61736B); node e takes word e & 3 of counter (e >> 2, m, 0,
    0), 1 iff float32(word >> 8) < float32(p) * 2^24; shift a = (word_a * c_a) >> 32 of counter (0, m, 1, 0).
    -> (nodes (N, n_d, n_h, n_w) uint8, shifts (N, 3) int32)."""
    cell, nn, G = geometry(size, cells)
    key = ((seed & 0xFFFFFFFF) ^ 0x52495345, (seed >> 32) ^ 0x6D61736B)
    nq = (G + 3) // 4
    thr = F32(p) * F32(16777216.0)
    nodes, shifts = np.empty((N, G), np.uint8), np.empty((N, 3), np.int32)
    for k in range(N):
        m = m0 + k
        ctr = np.stack([np.arange(nq), np.full(nq, m), np.zeros(nq, np.int64), np.zeros(nq, np.int64)], 1)
        words = philox4x32(ctr, key).reshape(-1)[:G]
        nodes[k] = (words >> np.uint64(8)).astype(F32) < thr
        w = philox4x32([(0, m, 1, 0)], key)[0]
        shifts[k] = [(int(w[a]) * cell[a]) >> 32 for a in range(3)]
    return torch.from_numpy(nodes.reshape((N,) + nn)), torch.from_numpy(shifts)


def mask_scalar32(nodes, shifts, size, cells):
    """One mask (nodes (n_d, n_h, n_w), shifts (3,), numpy) voxel by voxel in numpy float32 scalars, every operation rounded on
    its own, W first, then H, then D -> (D, H, W) float32."""
    cell, _nn, _G = geometry(size, cells)
    invc = [F32(1.0) / F32(c) for c in cell]
    g = nodes.astype(F32)
    out = np.empty(size, F32)

    def axis(v, a):
        q = v + int(shifts[a])
        i, r = q // cell[a], q % cell[a]
        w1 = F32(F32(r) * invc[a])
        return i, F32(F32(1.0) - w1), w1

    for z in range(size[0]):
        i_d, w0d, w1d = axis(z, 0)
        for y in range(size[1]):
            i_h, w0h, w1h = axis(y, 1)
            for x in range(size[2]):
                i_w, w0w, w1w = axis(x, 2)
                xs = [[F32(F32(g[i_d + a, i_h + b, i_w] * w0w) + F32(g[i_d + a, i_h + b, i_w + 1] * w1w)) for b in (0, 1)]
                      for a in (0, 1)]
                ys = [F32(F32(xs[a][0] * w0h) + F32(xs[a][1] * w1h)) for a in (0, 1)]
                out[z, y, x] = F32(F32(ys[0] * w0d) + F32(ys[1] * w1d))
    return out


MASK_BOUND = 16 * 2.0 ** -24          # |M - M_exact|
MASK_MAX = 1 + 2.0 ** -22


def map_tolerance(scores, scale, terms):
    """(B,): scale * (n + 18) * 2^-24 * sum_m |scores[b][m]| over the `terms` mask indices of the sum."""
    return abs(scale) * (len(terms) + 18) * 2.0 ** -24 * scores.double()[:, list(terms)].abs().sum(1)


def row_errors(got, ref):
    """(B,): max |got - ref| per sample."""
    B = ref.shape[0]
    return (got.double() - ref.double()).abs().reshape(B, -1).amax(1)


@functools.lru_cache(maxsize=None)
def volumes(size, B=3, seed=3):
    """vol (B, 1, D, H, W) in [0.5, 1.5), fill (B,) and a base volume of vol's shape; never modified."""
    g = torch.Generator().manual_seed(seed + size[0] * 131 + size[2])
    vol = torch.rand((B, 1) + tuple(size), generator=g) + 0.5
    fill = torch.tensor([0.25, -1.5, 3.0][:B])
    base = torch.rand((B, 1) + tuple(size), generator=g) * 2 - 1
    return vol, fill, base


@functools.lru_cache(maxsize=None)
def scores_for(B, N, seed=5):
    """(B, N) scores of both signs; never modified."""
    g = torch.Generator().manual_seed(seed + 17 * B + N)
    return torch.randn((B, N), generator=g)


def chunkings(B, N):
    """(j0, K): K = 1, a chunk that crosses into the next sample, the short last chunk."""
    return [(N - 1, 1), (N - 2, 5), (B * N - 3, 3)]
