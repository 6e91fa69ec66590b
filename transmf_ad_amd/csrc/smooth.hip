// smooth.hip — separable 3-D Gaussian smoothing of voxel maps, optionally normalised inside a mask (include/tmf_hip.h states the
// taps, the three border modes, the error bound and the mask semantics).  gfx950.
//
// Two launches.  Launch 1 filters W, then H: one workgroup takes a TH x TW tile of one (b, d) plane, loads it with its halo into
// LDS — THE BORDER MODE IS APPLIED HERE, per loaded element, so the filters themselves are plain dot products —, filters the rows
// along W into a second LDS tile and that one along H into the intermediate in the caller's workspace.  Launch 2 filters D: the
// plane is a flat vector of H*W floats there, a workgroup loads TD + 2r rows of TX of them into LDS and every lane walks the taps
// down its column (16 bytes per lane and tap on the fast path).  The taps are staged once per workgroup in LDS.  With a mask,
// launch 1 carries a*m and, in the workgroups of sample 0 alone, m itself (the mask serves all samples, so G_hw(m) is ONE volume);
// launch 2 filters both along D and divides.
//
// Every output element is a chain of fmaf in ascending tap order from 0.0f, the same instruction sequence on the 16-byte and on
// the one-element path: the two paths differ in how tiles are moved, not in what is added.  No atomics, no workgroup waits for
// another; a workgroup walks its tiles in a grid-stride loop, so the grid is bounded whatever the shape.
#include "tmf_device.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_BATCH = 4;                     // items a lane loads before it stores the first of them
constexpr int SM_ROWS = 4;                      // rows a lane filters along W at once
constexpr int SM_TAPS = 2 * TMF_SMOOTH_MAX_RADIUS + 1;
constexpr long SM_MAX_GRID = 1 << 20;           // workgroups of a launch; further tiles are walked by the same workgroups
constexpr size_t SM_LDS_MAX = 64 * 1024;        // tiles shrink until they fit this: no opt-in to more LDS, two workgroups per compute unit

struct SmTaps {                                 // by value in the kernel arguments: [0] D, [1] H, [2] W; taps[axis][i + r], i = -r..r
    float w[3][SM_TAPS];
};

// Source index of tap position j on an axis of extent n, -1 where the tap contributes 0 (TMF_SMOOTH_CONSTANT outside 0..n-1).
__device__ __forceinline__ int sm_map(int j, int n, int mode) {
    if ((unsigned)j < (unsigned)n) return j;
    if (mode == TMF_SMOOTH_CONSTANT) return -1;
    if (mode == TMF_SMOOTH_NEAREST) return j < 0 ? 0 : n - 1;
    // reflect: p = j mod 2n, source p or 2n-1-p.  The pattern d c b a | a b c d is symmetric about -1/2, so j < 0 reads what
    // -1 - j reads, and the modulus stays an unsigned 32-bit division (2n < 2^32).
    const unsigned n2 = 2u * (unsigned)n;
    const unsigned p = (unsigned)(j < 0 ? -1 - j : j) % n2;
    return (int)(p < (unsigned)n ? p : n2 - 1u - p);
}

// The lane's first item of a rows x cols walk (cols > 0) and the step that moves it SM_THREADS items on.
struct SmWalk {
    int y, x, dy, dx, cols;
    __device__ __forceinline__ SmWalk(int cols_) : cols(cols_) {
        y = (int)threadIdx.x / cols;
        x = (int)threadIdx.x - y * cols;
        dy = SM_THREADS / cols;
        dx = SM_THREADS - dy * cols;
    }
    __device__ __forceinline__ void next() {
        y += dy;
        x += dx;
        if (x >= cols) { x -= cols; ++y; }
    }
};

// The taps for the tap loops: copied once per workgroup from the kernel arguments to the head of the dynamic LDS, [3][SM_TAPS]
// floats in SM_TAPS_LDS bytes.  A tap fetched from the kernel arguments inside the loop is a scalar load, and the wait for it
// also drains the LDS reads in flight (one counter), which made every tap cost a memory round trip; a tap in LDS is one more
// read of the same queue, the same address for all lanes.
constexpr int SM_TAPS_LDS = (3 * SM_TAPS * 4 + 15) & ~15;
struct SmAxisTaps {
    const float* t;
    __device__ __forceinline__ float operator[](int i) const { return t[i]; }
};
__device__ __forceinline__ void sm_stage_taps(float* lds, const SmTaps& taps) {
    const float* flat = &taps.w[0][0];
    if (threadIdx.x < 3 * SM_TAPS) lds[threadIdx.x] = flat[threadIdx.x];
    __syncthreads();
}

template <int N> struct SmVec;
template <> struct SmVec<4> { typedef f32x4 F; };
template <> struct SmVec<1> { typedef tmf_f32x1 F; };

template <int N> __device__ __forceinline__ typename SmVec<N>::F sm_lds_ld(const float* p) {
    return *reinterpret_cast<const typename SmVec<N>::F*>(p);
}
template <int N> __device__ __forceinline__ void sm_lds_st(float* p, typename SmVec<N>::F v) {
    *reinterpret_cast<typename SmVec<N>::F*>(p) = v;
}

// acc[q] = fmaf(tap i, p[i*stride + q], acc[q]) for i = 0..n-1 IN THIS ORDER, N columns per lane.  Written out four taps at a time
// so that four LDS reads (and their taps) are in flight before the first is used.
template <int N>
__device__ __forceinline__ void sm_dot(typename SmVec<N>::F& acc, const float* p, int stride, int n, const SmAxisTaps& taps) {
    typedef typename SmVec<N>::F VF;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        VF v[4];
        float w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = sm_lds_ld<N>(p + (i + u) * stride);
            w[u] = taps[i + u];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] = fmaf(w[u], v[u][q], acc[q]);
    }
    for (; i < n; ++i) {
        const VF v = sm_lds_ld<N>(p + i * stride);
        const float w = taps[i];
#pragma unroll
        for (int q = 0; q < N; ++q) acc[q] = fmaf(w, v[q], acc[q]);
    }
}

// The same along a row for SM_ROWS rows at once: acc[q] = fmaf(tap i, base[off[q] + i], acc[q]), two taps at a time.
__device__ __forceinline__ void sm_dot_rows(float (&acc)[SM_ROWS], const float* base, const int (&off)[SM_ROWS], int n,
                                            const SmAxisTaps& taps) {
    int i = 0;
    for (; i + 2 <= n; i += 2) {
        float v[2][SM_ROWS], w[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            w[u] = taps[i + u];
#pragma unroll
            for (int q = 0; q < SM_ROWS; ++q) v[u][q] = base[off[q] + i + u];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < SM_ROWS; ++q) acc[q] = fmaf(w[u], v[u][q], acc[q]);
    }
    for (; i < n; ++i) {
        const float w = taps[i];
#pragma unroll
        for (int q = 0; q < SM_ROWS; ++q) acc[q] = fmaf(w, base[off[q] + i], acc[q]);
    }
}

// Launch 1.  Tile t = ((b*D + d)*tilesH + th)*tilesW + tw.  LDS: taps | in [LH][LW] | tmp [LH][TW] (| the same pair for m), LH = TH + 2 rh,
// LW = TW + 2 RW with RW = rw rounded up to 4: LDS column c is source column w0 - RW + c, so a group of four LDS columns is a
// 16-byte group of the row in memory (W % 4 == 0 on the fast path: such a group lies wholly inside the row or wholly outside).
template <bool VEC, bool MASKED>
__global__ __launch_bounds__(SM_THREADS) void smooth_hw_kernel(const float* __restrict__ a, const int* __restrict__ mask,
                                                               float* __restrict__ inter, float* __restrict__ den, const SmTaps taps,
                                                               int D, int H, int W, int rh, int rw, int TH, int TW, int mode,
                                                               int tilesH, int tilesW, long total) {
    constexpr int N = VEC ? 4 : 1;
    typedef typename SmVec<N>::F VF;
    extern __shared__ __attribute__((aligned(16))) char sm_lds[];
    const int RW = (rw + 3) & ~3, LW = TW + 2 * RW, LH = TH + 2 * rh;
    float* tap_lds = reinterpret_cast<float*>(sm_lds);
    float* in_a = reinterpret_cast<float*>(sm_lds + SM_TAPS_LDS);
    float* tmp_a = in_a + LH * LW;
    float* in_m = tmp_a + LH * TW;
    float* tmp_m = in_m + LH * LW;
    const size_t plane = (size_t)H * W;
    sm_stage_taps(tap_lds, taps);
    const SmAxisTaps taps_h{tap_lds + SM_TAPS}, taps_w{tap_lds + 2 * SM_TAPS};
    for (long t = blockIdx.x; t < total; t += gridDim.x) {
        const int tw = (int)(t % tilesW);
        const long t1 = t / tilesW;
        const int th = (int)(t1 % tilesH);
        const long bd = t1 / tilesH;
        const int d = (int)(bd % D), b = (int)(bd / D);
        const int h0 = th * TH, w0 = tw * TW;
        const float* src = a + (size_t)bd * plane;
        const int* msk = MASKED ? mask + (size_t)d * plane : nullptr;
        const bool with_m = MASKED && b == 0;           // G_hw(m) is one volume for all samples: sample 0's workgroups make it

        // the tile and its halo, border mode applied.  A lane takes SM_BATCH items at a time and loads them all - from a
        // harmless address of the plane where an item has nothing to load - before it stores the first, so that the loads of a
        // batch are in flight together; on the fast path a group that straddles the row's end follows element by element.
        const int gpr = LW / N, items = LH * gpr;
        for (int base = threadIdx.x; base < items; base += SM_THREADS * SM_BATCH) {
            VF va[SM_BATCH], vm[SM_BATCH];
            int at[SM_BATCH], hs[SM_BATCH], j0[SM_BATCH];
            bool edge[SM_BATCH];
#pragma unroll
            for (int u = 0; u < SM_BATCH; ++u) {
                const int idx = base + u * SM_THREADS;
                const bool live = idx < items;
                const int y = live ? idx / gpr : 0, c0 = live ? (idx - y * gpr) * N : 0;
                hs[u] = sm_map(h0 - rh + y, H, mode);
                j0[u] = w0 - RW + c0;
                at[u] = live ? y * LW + c0 : -1;
                if constexpr (VEC) {
                    const bool whole = hs[u] >= 0 && j0[u] >= 0 && j0[u] + 3 < W;
                    const size_t off = whole ? (size_t)hs[u] * W + j0[u] : 0;
                    const f32x4 v4 = TmfIO<float, 4>::ld(src + off);
                    i32x4 m4 = {1, 1, 1, 1};
                    if constexpr (MASKED) m4 = *reinterpret_cast<const i32x4*>(msk + off);
#pragma unroll
                    for (int q = 0; q < N; ++q) {
                        va[u][q] = whole && m4[q] != 0 ? v4[q] : 0.f;
                        vm[u][q] = whole && m4[q] != 0 ? 1.f : 0.f;
                    }
                    edge[u] = live && hs[u] >= 0 && !whole;
                } else {
                    const int ws = sm_map(j0[u], W, mode);
                    const bool ok = hs[u] >= 0 && ws >= 0;
                    const size_t off = ok ? (size_t)hs[u] * W + ws : 0;
                    const float v = src[off];
                    int mm = 1;
                    if constexpr (MASKED) mm = msk[off];
                    va[u][0] = ok && mm != 0 ? v : 0.f;
                    vm[u][0] = ok && mm != 0 ? 1.f : 0.f;
                    edge[u] = false;
                }
            }
            if constexpr (VEC) {
                bool any = false;
#pragma unroll
                for (int u = 0; u < SM_BATCH; ++u) any = any || edge[u];
                if (any) {                               // all offsets, then all loads, then the selects: one round trip
                    size_t eoff[SM_BATCH][N];
                    bool eok[SM_BATCH][N];
                    float ev[SM_BATCH][N];
                    int em[SM_BATCH][N];
#pragma unroll
                    for (int u = 0; u < SM_BATCH; ++u)
#pragma unroll
                        for (int q = 0; q < N; ++q) {
                            const int ws = sm_map(j0[u] + q, W, mode);
                            eok[u][q] = edge[u] && ws >= 0;
                            eoff[u][q] = eok[u][q] ? (size_t)hs[u] * W + ws : 0;
                        }
#pragma unroll
                    for (int u = 0; u < SM_BATCH; ++u)
#pragma unroll
                        for (int q = 0; q < N; ++q) {
                            ev[u][q] = src[eoff[u][q]];
                            em[u][q] = 1;
                            if constexpr (MASKED) em[u][q] = msk[eoff[u][q]];
                        }
#pragma unroll
                    for (int u = 0; u < SM_BATCH; ++u)
#pragma unroll
                        for (int q = 0; q < N; ++q)
                            if (eok[u][q]) {
                                va[u][q] = em[u][q] != 0 ? ev[u][q] : 0.f;
                                vm[u][q] = em[u][q] != 0 ? 1.f : 0.f;
                            }
                }
            }
#pragma unroll
            for (int u = 0; u < SM_BATCH; ++u) {
                if (at[u] < 0) continue;
                sm_lds_st<N>(in_a + at[u], va[u]);
                if (with_m) sm_lds_st<N>(in_m + at[u], vm[u]);
            }
        }
        __syncthreads();

        // along W: tmp[y][x] = sum_i w_w[i] * in[y][RW - rw + x + i], four rows per lane: four independent chains per tap
        const int nw = 2 * rw + 1, nh = 2 * rh + 1;
        for (SmWalk it(TW); it.y * SM_ROWS < LH; it.next()) {
            const int y0 = it.y * SM_ROWS;
            int off[SM_ROWS];
#pragma unroll
            for (int q = 0; q < SM_ROWS; ++q) off[q] = (y0 + q < LH ? y0 + q : LH - 1) * LW + (RW - rw) + it.x;
            float acc[SM_ROWS];
#pragma unroll
            for (int q = 0; q < SM_ROWS; ++q) acc[q] = 0.f;
            sm_dot_rows(acc, in_a, off, nw, taps_w);
#pragma unroll
            for (int q = 0; q < SM_ROWS; ++q)
                if (y0 + q < LH) tmp_a[(y0 + q) * TW + it.x] = acc[q];
            if (with_m) {
#pragma unroll
                for (int q = 0; q < SM_ROWS; ++q) acc[q] = 0.f;
                sm_dot_rows(acc, in_m, off, nw, taps_w);
#pragma unroll
                for (int q = 0; q < SM_ROWS; ++q)
                    if (y0 + q < LH) tmp_m[(y0 + q) * TW + it.x] = acc[q];
            }
        }
        __syncthreads();

        // along H: inter[h0 + y][w0 + x] = sum_i w_h[i] * tmp[y + i][x]
        for (SmWalk it(TW / N); it.y < TH; it.next()) {
            const int x = it.x * N, h = h0 + it.y, w = w0 + x;
            if (h >= H || w >= W) continue;
            const float* p = tmp_a + it.y * TW + x;
            VF acc;
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] = 0.f;
            sm_dot<N>(acc, p, TW, nh, taps_h);
            TmfIO<float, N>::st(inter + (size_t)bd * plane + (size_t)h * W + w, acc);
            if (with_m) {
                const float* pm = tmp_m + it.y * TW + x;
                VF accm;
#pragma unroll
                for (int q = 0; q < N; ++q) accm[q] = 0.f;
                sm_dot<N>(accm, pm, TW, nh, taps_h);
                TmfIO<float, N>::st(den + (size_t)d * plane + (size_t)h * W + w, accm);
            }
        }
        __syncthreads();                                // the next tile overwrites both LDS tiles
    }
}

// Launch 2.  Tile t = (b*tilesD + td)*tilesX + tx over the planes as flat vectors of HW floats.  LDS: taps | rows [LD][TX] (| the same
// for G_hw(m)), LD = TD + 2 rd; LDS row y is source plane d0 - rd + y under the border mode.
template <bool VEC, bool MASKED>
__global__ __launch_bounds__(SM_THREADS) void smooth_d_kernel(const float* __restrict__ inter, const float* __restrict__ den,
                                                              const int* __restrict__ mask, float* __restrict__ out, const SmTaps taps,
                                                              int D, long HW, int rd, int TD, int TX, int mode, int tilesD, long tilesX,
                                                              long total) {
    constexpr int N = VEC ? 4 : 1;
    typedef typename SmVec<N>::F VF;
    extern __shared__ __attribute__((aligned(16))) char sm_lds[];
    const int LD = TD + 2 * rd, nd = 2 * rd + 1;
    float* tap_lds = reinterpret_cast<float*>(sm_lds);
    float* in_a = reinterpret_cast<float*>(sm_lds + SM_TAPS_LDS);
    float* in_m = in_a + LD * TX;
    sm_stage_taps(tap_lds, taps);
    const SmAxisTaps taps_d{tap_lds};
    for (long t = blockIdx.x; t < total; t += gridDim.x) {
        const long tx = t % tilesX, t1 = t / tilesX;
        const int td = (int)(t1 % tilesD), b = (int)(t1 / tilesD);
        const int d0 = td * TD;
        const long x0 = tx * TX;
        const float* src = inter + (size_t)b * D * HW;
        const int gpr = TX / N, items = LD * gpr;
        for (int base = threadIdx.x; base < items; base += SM_THREADS * SM_BATCH) {      // batched as in launch 1
            VF va[SM_BATCH], vm[SM_BATCH];
            int at[SM_BATCH];
#pragma unroll
            for (int u = 0; u < SM_BATCH; ++u) {
                const int idx = base + u * SM_THREADS;
                const bool live = idx < items;
                const int y = live ? idx / gpr : 0, c0 = live ? (idx - y * gpr) * N : 0;
                const int ds = sm_map(d0 - rd + y, D, mode);
                const long x = x0 + c0;
                const bool ok = ds >= 0 && x < HW;              // HW % 4 == 0 on the fast path: x + 3 < HW as well
                const size_t off = ok ? (size_t)ds * HW + x : 0;
                at[u] = live ? y * TX + c0 : -1;
                va[u] = TmfIO<float, N>::ld(src + off);
                if constexpr (MASKED) vm[u] = TmfIO<float, N>::ld(den + off);
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    va[u][q] = ok ? va[u][q] : 0.f;
                    if constexpr (MASKED) vm[u][q] = ok ? vm[u][q] : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < SM_BATCH; ++u) {
                if (at[u] < 0) continue;
                sm_lds_st<N>(in_a + at[u], va[u]);
                if constexpr (MASKED) sm_lds_st<N>(in_m + at[u], vm[u]);
            }
        }
        __syncthreads();
        for (SmWalk it(TX / N); it.y < TD; it.next()) {
            const int c0 = it.x * N, d = d0 + it.y;
            const long x = x0 + c0;
            if (d >= D || x >= HW) continue;
            const float* p = in_a + it.y * TX + c0;
            VF acc;
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] = 0.f;
            sm_dot<N>(acc, p, TX, nd, taps_d);
            if (MASKED) {
                const float* pm = in_m + it.y * TX + c0;
                VF accm;
#pragma unroll
                for (int q = 0; q < N; ++q) accm[q] = 0.f;
                sm_dot<N>(accm, pm, TX, nd, taps_d);
                const int* pk = mask + (size_t)d * HW + x;
                if constexpr (VEC) {
                    const i32x4 m4 = *reinterpret_cast<const i32x4*>(pk);
#pragma unroll
                    for (int q = 0; q < N; ++q) acc[q] = m4[q] != 0 ? acc[q] / accm[q] : 0.f;
                } else {
                    acc[0] = *pk != 0 ? acc[0] / accm[0] : 0.f;
                }
            }
            TmfIO<float, N>::st(out + (size_t)b * D * HW + (size_t)d * HW + x, acc);
        }
        __syncthreads();
    }
}

// ---- host side ----

bool sm_al(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

bool sm_shape_ok(int B, int D, int H, int W) {
    return B >= 1 && B <= 65536 && D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W <= INT_MAX;
}

size_t sm_inter_floats(int B, long V) { return ((size_t)B * (size_t)V + 3) & ~(size_t)3; }      // G_hw(m) starts 16-byte aligned

// The double taps: THE definition (tmf_gaussian_taps rounds them once).  -> r, or TMF_E_ARG with the message set.
int sm_taps_f64(const char* fn, double sigma, double truncate, double* w) {
    TMF_REQUIRE(isfinite(sigma) && sigma >= 0.0, TMF_E_ARG, "%s: sigma = %g is not a finite number >= 0", fn, sigma);
    TMF_REQUIRE(isfinite(truncate) && truncate > 0.0, TMF_E_ARG, "%s: truncate = %g is not a finite number > 0", fn, truncate);
    if (sigma == 0.0) {
        w[0] = 1.0;
        return 0;
    }
    const double reach = truncate * sigma + 0.5;
    TMF_REQUIRE(reach < (double)(TMF_SMOOTH_MAX_RADIUS + 1), TMF_E_ARG,
                "%s: sigma = %g with truncate = %g needs a radius above TMF_SMOOTH_MAX_RADIUS = %d", fn, sigma, truncate,
                TMF_SMOOTH_MAX_RADIUS);
    const int r = (int)reach;
    if (r == 0) {                                       // one tap; a sigma whose square underflows must not reach the division
        w[0] = 1.0;
        return 0;
    }
    double sum = 0.0;
    for (int i = -r; i <= r; ++i) {
        w[i + r] = exp(-0.5 * (double)i * (double)i / (sigma * sigma));
        sum += w[i + r];
    }
    for (int i = 0; i <= 2 * r; ++i) w[i] /= sum;
    return r;
}

struct SmPlan {
    int TH, TW, TD, TX;
    size_t lds_hw, lds_d;
};

SmPlan sm_plan(int D, int H, int W, const int r[3], bool masked) {
    SmPlan p;
    const long HW = (long)H * W;
    p.TH = H < 32 ? H : 32;
    p.TW = W < 128 ? (W + 3) & ~3 : 128;
    p.TD = D < 32 ? D : 32;
    p.TX = HW < 128 ? (int)((HW + 3) & ~3) : 128;
    const int RW = (r[2] + 3) & ~3;
    auto hw_bytes = [&]() { return SM_TAPS_LDS + (size_t)(p.TH + 2 * r[1]) * (size_t)(2 * p.TW + 2 * RW) * sizeof(float) * (masked ? 2 : 1); };
    while (hw_bytes() > SM_LDS_MAX) {                   // ends below it: (1 + 64) * (2 * 16 + 64) floats, twice, and the taps are 50704 bytes
        if (p.TH > 8) p.TH = (p.TH + 1) / 2;
        else if (p.TW > 32) p.TW = ((p.TW / 2) + 3) & ~3;
        else if (p.TH > 1) p.TH = (p.TH + 1) / 2;
        else if (p.TW > 16) p.TW = 16;
        else break;
    }
    auto d_bytes = [&]() { return SM_TAPS_LDS + (size_t)(p.TD + 2 * r[0]) * (size_t)p.TX * sizeof(float) * (masked ? 2 : 1); };
    while (d_bytes() > SM_LDS_MAX) {                    // ends below it: (8 + 64) * 64 floats, twice, and the taps are 37648 bytes
        if (p.TD > 8) p.TD = (p.TD + 1) / 2;
        else if (p.TX > 64) p.TX = 64;
        else break;
    }
    p.lds_hw = hw_bytes();
    p.lds_d = d_bytes();
    return p;
}

}  // namespace

extern "C" int tmf_gaussian_taps_f64(double sigma, double truncate, double* taps, int capacity) {
    TMF_REQUIRE_PTR(taps);
    double w[SM_TAPS];
    const int r = sm_taps_f64(__func__, sigma, truncate, w);
    if (r < 0) return r;
    TMF_REQUIRE(capacity >= 2 * r + 1, TMF_E_ARG, "%s: capacity = %d, %d taps to write", __func__, capacity, 2 * r + 1);
    for (int i = 0; i <= 2 * r; ++i) taps[i] = w[i];
    return r;
}

extern "C" int tmf_gaussian_taps(double sigma, double truncate, float* taps, int capacity) {
    TMF_REQUIRE_PTR(taps);
    double w[SM_TAPS];
    const int r = sm_taps_f64(__func__, sigma, truncate, w);
    if (r < 0) return r;
    TMF_REQUIRE(capacity >= 2 * r + 1, TMF_E_ARG, "%s: capacity = %d, %d taps to write", __func__, capacity, 2 * r + 1);
    for (int i = 0; i <= 2 * r; ++i) taps[i] = (float)w[i];
    return r;
}

extern "C" size_t tmf_smooth_workspace_bytes(int B, int D, int H, int W, int masked) {
    if (!sm_shape_ok(B, D, H, W)) return 0;
    const long V = (long)D * H * W;
    return (sm_inter_floats(B, V) + (masked ? ((size_t)V + 3) & ~(size_t)3 : 0)) * sizeof(float);
}

extern "C" int tmf_gaussian_smooth(const float* a, const int* mask, float* out, double sigma_d, double sigma_h, double sigma_w,
                                   double truncate, int mode, void* workspace, size_t workspace_bytes, int B, int D, int H, int W,
                                   void* stream) {
    TMF_REQUIRE_PTR(a); TMF_REQUIRE_PTR(out); TMF_REQUIRE_PTR(workspace);
    TMF_REQUIRE(B >= 1 && B <= 65536, TMF_E_SHAPE, "%s: B = %d (1 .. 65536)", __func__, B);
    TMF_REQUIRE(D >= 1 && H >= 1 && W >= 1 && (long long)D * H * W <= INT_MAX, TMF_E_SHAPE,
                "%s: D, H, W = %d, %d, %d: extents >= 1 with D*H*W < 2^31", __func__, D, H, W);
    TMF_REQUIRE(mode == TMF_SMOOTH_REFLECT || mode == TMF_SMOOTH_CONSTANT || mode == TMF_SMOOTH_NEAREST, TMF_E_ARG,
                "%s: mode = %d (0 reflect, 1 constant, 2 nearest)", __func__, mode);
    SmTaps taps;
    int r[3];
    const double sigma[3] = {sigma_d, sigma_h, sigma_w};
    for (int k = 0; k < 3; ++k) {
        double w[SM_TAPS];
        r[k] = sm_taps_f64(__func__, sigma[k], truncate, w);
        if (r[k] < 0) return r[k];
        for (int i = 0; i < SM_TAPS; ++i) taps.w[k][i] = i <= 2 * r[k] ? (float)w[i] : 0.f;
    }
    TMF_REQUIRE(sm_al(a, 4) && sm_al(out, 4) && sm_al(mask, 4), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE_ALIGNED(workspace);
    const long V = (long)D * H * W;
    const size_t bytes = (size_t)B * (size_t)V * sizeof(float);
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), po = reinterpret_cast<uintptr_t>(out);
    TMF_REQUIRE(pa + bytes <= po || po + bytes <= pa, TMF_E_ARG, "%s: out overlaps a", __func__);
    const bool masked = mask != nullptr;
    const size_t need = tmf_smooth_workspace_bytes(B, D, H, W, masked ? 1 : 0);
    TMF_REQUIRE(workspace_bytes >= need, TMF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, need);

    float* inter = static_cast<float*>(workspace);
    float* den = masked ? inter + sm_inter_floats(B, V) : nullptr;
    const long HW = (long)H * W;
    const bool vec = W % 4 == 0 && sm_al(a, 16) && sm_al(out, 16) && sm_al(mask, 16);
    const SmPlan p = sm_plan(D, H, W, r, masked);
    TMF_REQUIRE(p.lds_hw <= SM_LDS_MAX && p.lds_d <= SM_LDS_MAX, TMF_E_SHAPE, "%s: tiles of %zu and %zu bytes do not fit the LDS",
                __func__, p.lds_hw, p.lds_d);
    const int tilesH = tmf_cdiv(H, p.TH), tilesW = tmf_cdiv(W, p.TW), tilesD = tmf_cdiv(D, p.TD);
    const long tilesX = (HW + p.TX - 1) / p.TX;
    const long total1 = (long)B * D * tilesH * tilesW, total2 = (long)B * tilesD * tilesX;
    const dim3 grid1((unsigned)(total1 < SM_MAX_GRID ? total1 : SM_MAX_GRID)), grid2((unsigned)(total2 < SM_MAX_GRID ? total2 : SM_MAX_GRID));
    const dim3 block(SM_THREADS);
    hipStream_t s = (hipStream_t)stream;
#define SM_LAUNCH(VEC, MASKED)                                                                                                        \
    do {                                                                                                                              \
        hipLaunchKernelGGL((smooth_hw_kernel<VEC, MASKED>), grid1, block, p.lds_hw, s, a, mask, inter, den, taps, D, H, W, r[1], r[2], \
                           p.TH, p.TW, mode, tilesH, tilesW, total1);                                                                 \
        hipLaunchKernelGGL((smooth_d_kernel<VEC, MASKED>), grid2, block, p.lds_d, s, inter, den, mask, out, taps, D, HW, r[0], p.TD,   \
                           p.TX, mode, tilesD, tilesX, total2);                                                                       \
    } while (0)
    if (vec && masked) SM_LAUNCH(true, true);
    else if (vec) SM_LAUNCH(true, false);
    else if (masked) SM_LAUNCH(false, true);
    else SM_LAUNCH(false, false);
#undef SM_LAUNCH
    return tmf_launch_result(__func__);
}
