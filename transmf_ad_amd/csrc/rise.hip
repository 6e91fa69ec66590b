// rise.hip — RISE saliency maps (include/tmf_hip.h states the semantics): the generator of the low-resolution node grids and
// shifts (tmf_rise_masks), the batch writer (tmf_rise_apply: K perturbed copies of volumes in ONE launch, every mask value
// rebuilt from node bytes) and the map builder (tmf_rise_accumulate: sal = scale * sum_m scores * M_m, every mask rebuilt in
// registers, a gather without atomics).  gfx950.  Compiled with -ffp-contract=off: the mask value, the blend and the
// accumulation are chains of separately rounded operations (csrc/rise_mask.h holds the one mask evaluation).
//
// Apply: a streaming write, 16 bytes per lane where D*H*W % 4 == 0 and the pointers are 16-byte aligned, one element per lane
// otherwise.  A lane divides once per item (the voxel's coordinates and the three cells) and then walks its voxels with
// increments; the mask's node bytes come straight from global memory (a grid is a few hundred bytes and stays in cache).
// Accumulate: a workgroup owns a tile of RISE_TILE voxels, RISE_VPL consecutive ones per lane.  Per voxel and axis the lane
// keeps (v / c, v % c); a mask's shift t then gives i = v / c + (v % c + t >= c) and r = v % c + t - (that ? c : 0): no division
// in the mask loop.  Node grids of RISE_LDS_MASKS masks at a time are staged in LDS (grids up to RISE_LDS_GRID bytes; larger
// ones are read from global memory by the same code), each mask value feeds the accumulators of up to RISE_GROUP samples.
#include "tmf_device.h"
#include "rise_mask.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int RISE_THREADS = 256;
constexpr int RISE_ITEMS = 4;               // items a lane of the apply kernel walks at least, the volume permitting
constexpr long RISE_MAX_BLOCKS = 1 << 16;   // workgroups of an apply launch over all jobs; the limit of K and B
constexpr int RISE_VPL = 4;                 // consecutive voxels a lane of the accumulate kernel owns
constexpr int RISE_TILE = RISE_THREADS * RISE_VPL;
constexpr int RISE_ACC_MAX_TILES = 2048;    // workgroups per sample group of an accumulate launch; they stride beyond that
constexpr int RISE_GROUP = 8;               // samples fed by one mask evaluation
constexpr int RISE_LDS_BYTES = 32768;       // node grids staged at a time
constexpr int RISE_LDS_GRID = 4096;         // largest node grid (bytes) that is staged; a larger one is read from global memory
constexpr int RISE_LDS_MASKS = 64;          // masks staged at a time, at most

// ---- nodes and shifts ----

// Item it = k * per + q of mask m0 + k: q < per - 1 is a quad of nodes (one Philox call), q == per - 1 the three shifts.
__global__ __launch_bounds__(RISE_THREADS) void rise_masks_kernel(unsigned char* __restrict__ nodes, int* __restrict__ shifts,
                                                                  int G, int cd, int ch, int cw, float thr, unsigned k0,
                                                                  unsigned k1, int m0, long items, int per) {
    const long step = (long)gridDim.x * RISE_THREADS;
    for (long it = (long)blockIdx.x * RISE_THREADS + threadIdx.x; it < items; it += step) {
        const long k = it / per;
        const int q = (int)(it - k * per);
        const unsigned m = (unsigned)(m0 + (int)k);
        unsigned r[4];
        if (q < per - 1) {
            philox4x32_10((unsigned)q, m, 0u, 0u, k0, k1, r);
            unsigned char* dst = nodes + (size_t)k * G;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j;
                if (e < G) dst[e] = (float)(r[j] >> 8) < thr ? 1 : 0;
            }
        } else {
            philox4x32_10(0u, m, 1u, 0u, k0, k1, r);
            int* dst = shifts + (size_t)k * 3;
            dst[0] = (int)(((unsigned long long)r[0] * (unsigned)cd) >> 32);
            dst[1] = (int)(((unsigned long long)r[1] * (unsigned)ch) >> 32);
            dst[2] = (int)(((unsigned long long)r[2] * (unsigned)cw) >> 32);
        }
    }
}

// ---- apply ----

// A voxel under one mask's shift, walked in element order: (y, x) for the row ends, per axis the cell i and the remainder r.
struct RiseCursor {
    int y, x, id, rd, ih, rh, iw, rw;
};
__device__ __forceinline__ void rise_seek(RiseCursor& c, const RiseGeom& g, int e, int td, int th, int tw) {
    const int HW = g.h.S * g.w.S;
    const int z = e / HW, rem = e - z * HW;
    c.y = rem / g.w.S;
    c.x = rem - c.y * g.w.S;
    const int qd = z + td, qh = c.y + th, qw = c.x + tw;
    c.id = qd / g.d.c; c.rd = qd - c.id * g.d.c;
    c.ih = qh / g.h.c; c.rh = qh - c.ih * g.h.c;
    c.iw = qw / g.w.c; c.rw = qw - c.iw * g.w.c;
}
__device__ __forceinline__ void rise_step(RiseCursor& c, const RiseGeom& g, int td, int th, int tw) {
    ++c.x;
    if (++c.rw == g.w.c) { c.rw = 0; ++c.iw; }
    if (c.x == g.w.S) {
        c.x = 0; c.iw = 0; c.rw = tw;                       // t < c: cell 0
        ++c.y;
        if (++c.rh == g.h.c) { c.rh = 0; ++c.ih; }
        if (c.y == g.h.S) {
            c.y = 0; c.ih = 0; c.rh = th;
            if (++c.rd == g.d.c) { c.rd = 0; ++c.id; }
        }
    }
}
__device__ __forceinline__ float rise_at(const unsigned char* gm, const RiseGeom& g, const RiseCursor& c) {
    float w0d, w1d, w0h, w1h, w0w, w1w;
    rise_weights(c.rd, g.d.invc, w0d, w1d);
    rise_weights(c.rh, g.h.invc, w0h, w1h);
    rise_weights(c.rw, g.w.invc, w0w, w1w);
    return rise_mask_value(gm, (c.id * g.h.n + c.ih) * g.w.n + c.iw, g.h.n * g.w.n, g.w.n, w0d, w1d, w0h, w1h, w0w, w1w);
}

// out[k][e] = f + M_m(e) * (vol[b][e] - f) for job j0 + k = b*N + m, f = base[b][e] or fill[b].  Workgroup blockIdx.x =
// k*nblk + blk strides over the items of job k.
template <bool VEC>
__global__ __launch_bounds__(RISE_THREADS) void rise_apply_kernel(const float* __restrict__ vol,
                                                                  const unsigned char* __restrict__ nodes,
                                                                  const int* __restrict__ shifts, const float* __restrict__ fill,
                                                                  const float* __restrict__ base, float* __restrict__ out,
                                                                  RiseGeom g, int N, int j0, int nblk) {
    const int k = blockIdx.x / nblk, blk = blockIdx.x - k * nblk;
    const int j = j0 + k;
    const int b = j / N, m = j - b * N;
    const unsigned char* gm = nodes + (size_t)m * g.G;
    const int td = shifts[(size_t)m * 3], th = shifts[(size_t)m * 3 + 1], tw = shifts[(size_t)m * 3 + 2];
    const float f0 = base ? 0.f : fill[b];
    const float* src = vol + (size_t)b * g.V;
    const float* bs = base ? base + (size_t)b * g.V : nullptr;
    float* dst = out + (size_t)k * g.V;
    const long step = (long)nblk * RISE_THREADS;
    if (VEC) {
        const long n4 = g.V >> 2;
        for (long i = (long)blk * RISE_THREADS + threadIdx.x; i < n4; i += step) {
            const int e = (int)(i << 2);
            f32x4 v = TmfIO<float, 4>::ld(src + e);
            f32x4 f = {f0, f0, f0, f0};
            if (bs) f = TmfIO<float, 4>::ld(bs + e);
            RiseCursor c;
            rise_seek(c, g, e, td, th, tw);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float M = rise_at(gm, g, c);
                v[q] = f[q] + M * (v[q] - f[q]);
                rise_step(c, g, td, th, tw);
            }
            TmfIO<float, 4>::st(dst + e, v);
        }
    } else {
        for (long i = (long)blk * RISE_THREADS + threadIdx.x; i < g.V; i += step) {
            const int e = (int)i;
            RiseCursor c;
            rise_seek(c, g, e, td, th, tw);
            const float M = rise_at(gm, g, c);
            const float f = bs ? bs[e] : f0;
            dst[e] = f + M * (src[e] - f);
        }
    }
}

// ---- accumulate ----

// One axis of a lane's voxel without a shift: v / c and v % c.
struct RiseSplit {
    int i, r;
};
// ... and under the shift t (0 <= t < c): cell and remainder, no division
__device__ __forceinline__ void rise_shifted(const RiseSplit& s, int t, int c, int& i, int& r) {
    const int q = s.r + t;
    const bool over = q >= c;
    i = s.i + (over ? 1 : 0);
    r = q - (over ? c : 0);
}

// The masks mb, mb + m_step, ... (cnt of them) into LDS, grid k at byte k*Gp (Gp = G rounded up to 4): words where the source
// is 4-byte aligned, bytes otherwise and for the tail.
__device__ __forceinline__ void rise_stage(unsigned char* lds, const unsigned char* __restrict__ nodes, int G, int Gp, int mb,
                                           int m_step, int cnt) {
    for (int k = 0; k < cnt; ++k) {
        const unsigned char* src = nodes + (size_t)(mb + (long)k * m_step) * G;
        unsigned char* dst = lds + k * Gp;
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
            const int nw = G >> 2;
            for (int o = threadIdx.x; o < nw; o += RISE_THREADS)
                reinterpret_cast<unsigned*>(dst)[o] = reinterpret_cast<const unsigned*>(src)[o];
            done = nw << 2;
        }
        for (int o = done + threadIdx.x; o < G; o += RISE_THREADS) dst[o] = src[o];
    }
}

// The tiles of one sample group: NB > 0 samples known at compile time, NB == 0: nb of them (1..RISE_GROUP) at run time.
template <int NB, bool LDS>
__device__ __forceinline__ void rise_accumulate_tiles(const float* __restrict__ scores, const unsigned char* __restrict__ nodes,
                                                      const int* __restrict__ shifts, float* __restrict__ sal, float scale,
                                                      const RiseGeom& g, int N, int m_first, int m_step, int b0, int nb,
                                                      bool vec, unsigned char* lds) {
    const int plane = g.h.n * g.w.n, row = g.w.n;
    const int Gp = (g.G + 3) & ~3;
    const int per = LDS ? min(RISE_LDS_MASKS, RISE_LDS_BYTES / Gp) : RISE_LDS_MASKS;      // masks per batch
    const int HW = g.h.S * g.w.S;
    // W % RISE_VPL == 0: a lane's run starts at a multiple of RISE_VPL inside a row, its voxels share (z, y) - the D and H
    // cells, weights and the node row are computed once per mask, not once per voxel (the same operations on the same
    // operands: the bits do not change).  A wave-uniform test, so the other case costs this one nothing.
    const bool rows = g.w.S % RISE_VPL == 0;
    const long ntiles = ((long)g.V + RISE_TILE - 1) / RISE_TILE;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long e0 = tile * RISE_TILE + (long)threadIdx.x * RISE_VPL;
        RiseSplit vd[RISE_VPL], vh[RISE_VPL], vw[RISE_VPL];
#pragma unroll
        for (int q = 0; q < RISE_VPL; ++q) {
            const int e = (int)min(e0 + q, (long)g.V - 1);          // a voxel past the end: the last one's cells, never stored
            const int z = e / HW, rem = e - z * HW;
            const int y = rem / g.w.S, x = rem - y * g.w.S;
            vd[q].i = z / g.d.c; vd[q].r = z - vd[q].i * g.d.c;
            vh[q].i = y / g.h.c; vh[q].r = y - vh[q].i * g.h.c;
            vw[q].i = x / g.w.c; vw[q].r = x - vw[q].i * g.w.c;
        }
        float acc[RISE_GROUP][RISE_VPL];
#pragma unroll
        for (int s = 0; s < RISE_GROUP; ++s)
#pragma unroll
            for (int q = 0; q < RISE_VPL; ++q) acc[s][q] = 0.0f;

        for (long mb = m_first; mb < N; mb += (long)per * m_step) {
            const int cnt = (int)min((long)per, (N - mb + m_step - 1) / m_step);
            if (LDS) {
                __syncthreads();                                   // the previous batch has been read
                rise_stage(lds, nodes, g.G, Gp, (int)mb, m_step, cnt);
                __syncthreads();
            }
            for (int k = 0; k < cnt; ++k) {
                const int m = (int)(mb + (long)k * m_step);
                const unsigned char* gm = LDS ? lds + k * Gp : nodes + (size_t)m * g.G;
                const int td = shifts[(size_t)m * 3], th = shifts[(size_t)m * 3 + 1], tw = shifts[(size_t)m * 3 + 2];
                float sc[RISE_GROUP];
#pragma unroll
                for (int s = 0; s < RISE_GROUP; ++s)
                    sc[s] = (NB ? s < NB : s < nb) ? scores[(size_t)(b0 + s) * N + m] : 0.0f;
                int at_dh = 0;
                float w0d = 0.f, w1d = 0.f, w0h = 0.f, w1h = 0.f;
#pragma unroll
                for (int q = 0; q < RISE_VPL; ++q) {
                    if (q == 0 || !rows) {
                        int id, rd, ih, rh;
                        rise_shifted(vd[q], td, g.d.c, id, rd);
                        rise_shifted(vh[q], th, g.h.c, ih, rh);
                        rise_weights(rd, g.d.invc, w0d, w1d);
                        rise_weights(rh, g.h.invc, w0h, w1h);
                        at_dh = (id * g.h.n + ih) * g.w.n;
                    }
                    int iw, rw;
                    float w0w, w1w;
                    rise_shifted(vw[q], tw, g.w.c, iw, rw);
                    rise_weights(rw, g.w.invc, w0w, w1w);
                    const float M = rise_mask_value(gm, at_dh + iw, plane, row, w0d, w1d, w0h, w1h, w0w, w1w);
#pragma unroll
                    for (int s = 0; s < RISE_GROUP; ++s)
                        if (NB ? s < NB : s < nb) acc[s][q] = acc[s][q] + sc[s] * M;
                }
            }
        }

#pragma unroll
        for (int s = 0; s < RISE_GROUP; ++s) {
            if (!(NB ? s < NB : s < nb)) continue;
            float* dst = sal + (size_t)(b0 + s) * g.V;
            if (vec) {                                             // V % 4 == 0: the four voxels exist
                if (e0 < g.V)
                    TmfIO<float, 4>::st(dst + e0, f32x4{acc[s][0] * scale, acc[s][1] * scale, acc[s][2] * scale, acc[s][3] * scale});
            } else {
#pragma unroll
                for (int q = 0; q < RISE_VPL; ++q)
                    if (e0 + q < g.V) dst[e0 + q] = acc[s][q] * scale;
            }
        }
    }
}

// sal[b][e] = scale * sum_m scores[b][m] * M_m(e), m = m_first, m_first + m_step, ... < N, for the samples of group blockIdx.y.
template <bool LDS>
__global__ __launch_bounds__(RISE_THREADS) void rise_accumulate_kernel(const float* __restrict__ scores,
                                                                       const unsigned char* __restrict__ nodes,
                                                                       const int* __restrict__ shifts, float* __restrict__ sal,
                                                                       float scale, RiseGeom g, int B, int N, int m_first,
                                                                       int m_step, int vec) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS ? RISE_LDS_BYTES : 16];
    const int b0 = blockIdx.y * RISE_GROUP;
    const int nb = min(RISE_GROUP, B - b0);
    if (nb == RISE_GROUP)
        rise_accumulate_tiles<RISE_GROUP, LDS>(scores, nodes, shifts, sal, scale, g, N, m_first, m_step, b0, nb, vec != 0, lds);
    else if (nb == 1)
        rise_accumulate_tiles<1, LDS>(scores, nodes, shifts, sal, scale, g, N, m_first, m_step, b0, nb, vec != 0, lds);
    else
        rise_accumulate_tiles<0, LDS>(scores, nodes, shifts, sal, scale, g, N, m_first, m_step, b0, nb, vec != 0, lds);
}

// ---- host side ----

int rise_axis(const char* fn, char name, int S, int s, RiseAxis* a) {
    TMF_REQUIRE(S >= 1, TMF_E_SHAPE, "%s: extent %c = %d", fn, name, S);
    TMF_REQUIRE(s >= 1 && s <= S, TMF_E_ARG, "%s: cells %c = %d outside 1..%d", fn, name, s, S);
    a->S = S;
    a->c = (int)(((long)S + s - 1) / s);
    a->n = s + 2;
    a->invc = 1.0f / (float)a->c;
    return TMF_OK;
}

int rise_geom(const char* fn, int D, int H, int W, int sd, int sh, int sw, RiseGeom* g) {
    TMF_REQUIRE(D >= 1 && H >= 1 && W >= 1, TMF_E_SHAPE, "%s: volume %d x %d x %d", fn, D, H, W);
    const long long v = (long long)D * H;            // (two ints: no overflow)
    TMF_REQUIRE(v <= INT_MAX / W, TMF_E_SHAPE, "%s: D*H*W = %d*%d*%d does not stay below 2^31", fn, D, H, W);
    g->V = (int)(v * W);
    TMF_TRY(rise_axis(fn, 'd', D, sd, &g->d));
    TMF_TRY(rise_axis(fn, 'h', H, sh, &g->h));
    TMF_TRY(rise_axis(fn, 'w', W, sw, &g->w));
    const long long n = (long long)g->d.n * g->h.n;
    TMF_REQUIRE(n <= INT_MAX / g->w.n, TMF_E_SHAPE, "%s: a node grid of %d x %d x %d does not stay below 2^31 bytes", fn, g->d.n,
                g->h.n, g->w.n);
    g->G = (int)(n * g->w.n);
    return TMF_OK;
}

int rise_batch(const char* fn, int B, int N) {
    TMF_REQUIRE(B >= 1 && B <= RISE_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", fn, B, RISE_MAX_BLOCKS);
    TMF_REQUIRE(N >= 1, TMF_E_ARG, "%s: N = %d masks", fn, N);
    TMF_REQUIRE((long long)B * N <= INT_MAX, TMF_E_SHAPE, "%s: B * N = %d * %d does not stay below 2^31", fn, B, N);
    return TMF_OK;
}

bool rise_a4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool rise_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" int tmf_rise_geometry(int D, int H, int W, int sd, int sh, int sw, int* cell3, int* nodes3) {
    TMF_REQUIRE_PTR(cell3); TMF_REQUIRE_PTR(nodes3);
    RiseGeom g;
    TMF_TRY(rise_geom(__func__, D, H, W, sd, sh, sw, &g));
    cell3[0] = g.d.c; cell3[1] = g.h.c; cell3[2] = g.w.c;
    nodes3[0] = g.d.n; nodes3[1] = g.h.n; nodes3[2] = g.w.n;
    return g.G;
}

extern "C" int tmf_rise_masks(unsigned char* nodes, int* shifts, int D, int H, int W, int sd, int sh, int sw, float p,
                              unsigned long long seed, int m0, int N, void* stream) {
    TMF_REQUIRE_PTR(nodes); TMF_REQUIRE_PTR(shifts);
    RiseGeom g;
    TMF_TRY(rise_geom(__func__, D, H, W, sd, sh, sw, &g));
    TMF_REQUIRE(isfinite(p) && p > 0.f && p < 1.f, TMF_E_ARG, "%s: p = %g outside (0, 1)", __func__, (double)p);
    TMF_REQUIRE(N >= 1 && m0 >= 0 && (long long)m0 + N <= INT_MAX, TMF_E_ARG, "%s: masks m0 = %d, N = %d", __func__, m0, N);
    TMF_REQUIRE(rise_a4(shifts), TMF_E_ALIGN, "%s: shifts is not 4-byte aligned", __func__);
    const int per = (g.G + 3) / 4 + 1;
    const long items = (long)N * per;
    long blocks = (items + RISE_THREADS - 1) / RISE_THREADS;
    if (blocks > RISE_MAX_BLOCKS) blocks = RISE_MAX_BLOCKS;
    hipLaunchKernelGGL(rise_masks_kernel, dim3((unsigned)blocks), dim3(RISE_THREADS), 0, (hipStream_t)stream, nodes, shifts, g.G,
                       g.d.c, g.h.c, g.w.c, p * 16777216.0f, (unsigned)seed ^ 0x52495345u, (unsigned)(seed >> 32) ^ 0x6D61736Bu, m0,
                       items, per);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_rise_apply(const float* vol, const unsigned char* nodes, const int* shifts, const float* fill,
                              const float* base, float* out, int B, int D, int H, int W, int sd, int sh, int sw, int N, int j0,
                              int K, void* stream) {
    TMF_REQUIRE_PTR(vol); TMF_REQUIRE_PTR(nodes); TMF_REQUIRE_PTR(shifts); TMF_REQUIRE_PTR(out);
    TMF_REQUIRE(fill != nullptr || base != nullptr, TMF_E_NULL, "%s: fill and base are both NULL", __func__);
    RiseGeom g;
    TMF_TRY(rise_geom(__func__, D, H, W, sd, sh, sw, &g));
    TMF_TRY(rise_batch(__func__, B, N));
    TMF_REQUIRE(K >= 1 && K <= RISE_MAX_BLOCKS && j0 >= 0, TMF_E_ARG, "%s: jobs j0 = %d, K = %d (K at most %ld)", __func__, j0, K,
                RISE_MAX_BLOCKS);
    TMF_REQUIRE((long long)j0 + K <= (long long)B * N, TMF_E_ARG, "%s: jobs %d .. %lld of %lld", __func__, j0,
                (long long)j0 + K - 1, (long long)B * N);
    TMF_REQUIRE(rise_a4(vol) && rise_a4(shifts) && rise_a4(fill) && rise_a4(base) && rise_a4(out), TMF_E_ALIGN,
                "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE(out + (size_t)K * g.V <= vol || vol + (size_t)B * g.V <= out, TMF_E_ARG, "%s: out overlaps vol", __func__);
    const bool vec = g.V % 4 == 0 && rise_a16(vol) && rise_a16(out) && rise_a16(base);
    const long items = vec ? g.V / 4 : g.V;
    long nblk = (items + (long)RISE_THREADS * RISE_ITEMS - 1) / ((long)RISE_THREADS * RISE_ITEMS);
    const long cap = RISE_MAX_BLOCKS / K;              // >= 1: K <= RISE_MAX_BLOCKS
    nblk = nblk < 1 ? 1 : nblk > cap ? cap : nblk;
    if (vec)
        hipLaunchKernelGGL(rise_apply_kernel<true>, dim3((unsigned)(K * nblk)), dim3(RISE_THREADS), 0, (hipStream_t)stream, vol,
                           nodes, shifts, fill, base, out, g, N, j0, (int)nblk);
    else
        hipLaunchKernelGGL(rise_apply_kernel<false>, dim3((unsigned)(K * nblk)), dim3(RISE_THREADS), 0, (hipStream_t)stream, vol,
                           nodes, shifts, fill, base, out, g, N, j0, (int)nblk);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_rise_accumulate(const float* scores, const unsigned char* nodes, const int* shifts, float* sal, float scale,
                                   int B, int D, int H, int W, int sd, int sh, int sw, int N, int m_first, int m_step,
                                   void* stream) {
    TMF_REQUIRE_PTR(scores); TMF_REQUIRE_PTR(nodes); TMF_REQUIRE_PTR(shifts); TMF_REQUIRE_PTR(sal);
    RiseGeom g;
    TMF_TRY(rise_geom(__func__, D, H, W, sd, sh, sw, &g));
    TMF_TRY(rise_batch(__func__, B, N));
    TMF_REQUIRE(m_step >= 1 && m_first >= 0 && m_first < N, TMF_E_ARG, "%s: masks m_first = %d, m_step = %d of %d", __func__,
                m_first, m_step, N);
    TMF_REQUIRE(rise_a4(scores) && rise_a4(shifts) && rise_a4(sal), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    const int vec = g.V % 4 == 0 && rise_a16(sal);
    const long ntiles = ((long)g.V + RISE_TILE - 1) / RISE_TILE;
    const dim3 grid((unsigned)(ntiles < RISE_ACC_MAX_TILES ? ntiles : RISE_ACC_MAX_TILES), (unsigned)((B + RISE_GROUP - 1) / RISE_GROUP));
    if (g.G <= RISE_LDS_GRID)
        hipLaunchKernelGGL(rise_accumulate_kernel<true>, grid, dim3(RISE_THREADS), 0, (hipStream_t)stream, scores, nodes, shifts,
                           sal, scale, g, B, N, m_first, m_step, vec);
    else
        hipLaunchKernelGGL(rise_accumulate_kernel<false>, grid, dim3(RISE_THREADS), 0, (hipStream_t)stream, scores, nodes, shifts,
                           sal, scale, g, B, N, m_first, m_step, vec);
    return tmf_launch_result(__func__);
}
