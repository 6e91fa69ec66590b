// region_stats.hip — atlas region statistics of voxel maps (include/tmf_hip.h states the semantics): per sample and atlas label
// the count, the sum, the sum of |a|, the sum of max(a, 0), the maximum and the lowest index that attains it
// (tmf_region_stats), and the group accumulator n, sum x, sum x^2 per class and region (tmf_region_group_update).  gfx950.
//
// A label-keyed segmented reduction in INTEGERS: launch 1 finds peak_b = max |a[b]| (an integer atomic max on the bits);
// launch 2 scales every |a| by the power of two 2^(shift-e), 2^(e-1) <= peak_b < 2^e, rounds it once to an integer and adds the
// positive and the negative voxels of a bin apart (sum = P - N, abs_sum = P + N, pos_sum = P: two accumulators give three sums),
// and keeps max / argmax as ONE 64-bit integer max of (fc_key(a) << 32) | ~index; launch 3 turns the integers into the float
// outputs.  Integer addition and max commute, so the bits depend on neither the grid nor the order of arrival.
//
// Atlases are spatially coherent: the lanes of a wave mostly hit one bin, and 64 LDS atomics on one address serialise.  So a
// lane first combines its four voxels where they share a label (else it adds them one by one), then the wave combines every
// RUN of neighbouring lanes with one label by a segmented shuffle reduction, and only the first lane of a run touches LDS.  A
// workgroup keeps the bins in LDS and flushes the non-zero ones by global integer atomics.
#include "tmf_device.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;

constexpr int RS_THREADS = 256;
constexpr int RS_ITEMS = 8;                // items a lane walks at least, the sample permitting
constexpr long RS_MAX_BLOCKS = 1 << 16;    // workgroups of a launch over all samples
constexpr int RS_BINS = TMF_REGION_MAX + 1;

// workspace: acc u64 [B][3][R+1] (P, N, M) | cnt u32 [R+1] | peak u32 [B]
__host__ __device__ inline size_t rs_acc_bytes(int B, int R) { return (size_t)B * 3 * (size_t)(R + 1) * sizeof(u64); }

// e with 2^(e-1) <= |x| < 2^e for the bits of a finite |x| > 0 (0 for x == 0: every scaled value is 0 then)
__device__ __forceinline__ int rs_exp(unsigned bits) {
    if (bits == 0) return 0;
    const unsigned ex = bits >> 23, frac = bits & 0x7FFFFFu;
    return ex ? (int)ex - 126 : (32 - __clz((int)frac)) - 149;
}

// |x| * 2^sh rounded once (half away from zero) for the bits of |x|: x = m * 2^(ea-150) with the 24-bit significand m
__device__ __forceinline__ u64 rs_scaled(unsigned bits, int sh) {
    const unsigned ex = bits >> 23, frac = bits & 0x7FFFFFu;
    const u64 m = ex ? (frac | 0x800000u) : frac;
    int s = (int)(ex ? ex : 1u) - 150 + sh;
    s = s > 62 ? 62 : s;                       // finite input stays at or below shift - 24; only a non-finite one gets here
    if (s >= 0) return m << s;
    const int t = -s;
    return t > 24 ? 0ull : (m + (1ull << (t - 1))) >> t;
}

__device__ __forceinline__ u64 rs_shfl_down(u64 v, int d) {
    const unsigned lo = (unsigned)__shfl_down((int)(unsigned)v, d), hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}

// peak[b] = the largest bits of |a[b][v]|.  Workgroup blockIdx.x = b*nblk + blk.
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void region_peak_kernel(const float* __restrict__ a, unsigned* __restrict__ peak, int V,
                                                                 int nblk) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const float* src = a + (size_t)b * V;
    const long step = (long)nblk * RS_THREADS;
    unsigned m = 0;
    if (VEC) {
        const long n4 = V >> 2;
        for (long i = (long)blk * RS_THREADS + threadIdx.x; i < n4; i += step) {
            const f32x4 v = TmfIO<float, 4>::ld(src + (i << 2));
#pragma unroll
            for (int q = 0; q < 4; ++q) m = max(m, __float_as_uint(v[q]) & 0x7FFFFFFFu);
        }
    } else {
        for (long i = (long)blk * RS_THREADS + threadIdx.x; i < V; i += step) m = max(m, __float_as_uint(src[i]) & 0x7FFFFFFFu);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(&peak[b], m);
}

// The bins of sample b over the voxels the workgroup walks.  N = 4 (16 bytes per lane) or 1.
template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void region_accum_kernel(const float* __restrict__ a, const int* __restrict__ labels,
                                                                  u64* __restrict__ acc, unsigned* __restrict__ cnt,
                                                                  const unsigned* __restrict__ peak, int V, int R, int shift,
                                                                  int nblk) {
    constexpr int N = VEC ? 4 : 1;
    __shared__ u64 sP[RS_BINS], sN[RS_BINS], sM[RS_BINS];
    __shared__ unsigned sC[RS_BINS];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int lane = threadIdx.x & 63;
    const bool counts = b == 0;                 // count is a property of the atlas: the workgroups of sample 0 take it along
    for (int i = threadIdx.x; i <= R; i += RS_THREADS) {
        sP[i] = 0; sN[i] = 0; sM[i] = 0; sC[i] = 0;
    }
    __syncthreads();
    const int sh = shift - rs_exp(peak[b]);
    const float* src = a + (size_t)b * V;
    const long items = VEC ? V >> 2 : V;
    const long step = (long)nblk * RS_THREADS;
    for (long base = (long)blk * RS_THREADS; base < items; base += step) {      // the same trips for every lane: shuffles inside
        const long i = base + threadIdx.x;
        int key = -1;                           // the lane's bin where its voxels share one, else -1 (it has added them itself)
        u64 P = 0, Ng = 0, M = 0;
        if (i < items) {
            float v[N];
            int l[N];
            if (VEC) {
                const f32x4 v4 = TmfIO<float, 4>::ld(src + (i << 2));
                const i32x4 l4 = *reinterpret_cast<const i32x4*>(labels + (i << 2));
#pragma unroll
                for (int q = 0; q < N; ++q) { v[q] = v4[q]; l[q] = l4[q]; }
            } else {
                v[0] = src[i];
                l[0] = labels[i];
            }
            u64 p[N], n[N], m[N];
            bool same = true;
#pragma unroll
            for (int q = 0; q < N; ++q) {
                l[q] = (unsigned)l[q] <= (unsigned)R ? l[q] : 0;        // before any index is formed from it
                const unsigned u = __float_as_uint(v[q]);
                const u64 mag = rs_scaled(u & 0x7FFFFFFFu, sh);
                p[q] = (u >> 31) ? 0ull : mag;
                n[q] = (u >> 31) ? mag : 0ull;
                m[q] = ((u64)fc_key(v[q]) << 32) | (unsigned)~(unsigned)(i * N + q);
                same = same && l[q] == l[0];
            }
            if (same) {
                key = l[0];
#pragma unroll
                for (int q = 0; q < N; ++q) { P += p[q]; Ng += n[q]; M = max(M, m[q]); }
            } else {
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    if (p[q]) atomicAdd(&sP[l[q]], p[q]);
                    if (n[q]) atomicAdd(&sN[l[q]], n[q]);
                    atomicMax(&sM[l[q]], m[q]);
                    if (counts) atomicAdd(&sC[l[q]], 1u);
                }
            }
        }
        // runs of neighbouring lanes with one bin: lane `lane` heads the run lane .. end
        int end = lane;
#ifndef TMF_REGION_NO_RUNS
        const int before = __shfl_up(key, 1);
        const bool head = lane == 0 || key != before || key < 0;
        const u64 heads = __ballot(head);
        if (heads != ~0ull) {
            const u64 after = lane == 63 ? 0ull : heads >> (lane + 1);
            end = after ? lane + __ffsll((long long)after) - 1 : 63;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const u64 tP = rs_shfl_down(P, d), tN = rs_shfl_down(Ng, d), tM = rs_shfl_down(M, d);
                if (lane + d <= end) { P += tP; Ng += tN; M = max(M, tM); }
            }
        }
        if (head && key >= 0) {
#else
        if (key >= 0) {
#endif
            if (P) atomicAdd(&sP[key], P);
            if (Ng) atomicAdd(&sN[key], Ng);
            atomicMax(&sM[key], M);
            if (counts) atomicAdd(&sC[key], (unsigned)(N * (end - lane + 1)));
        }
    }
    __syncthreads();
    u64* g = acc + (size_t)b * 3 * (R + 1);
    for (int i = threadIdx.x; i <= R; i += RS_THREADS) {
        if (sP[i]) atomicAdd(&g[i], sP[i]);
        if (sN[i]) atomicAdd(&g[(R + 1) + i], sN[i]);
        if (sM[i]) atomicMax(&g[2 * (R + 1) + i], sM[i]);
        if (counts && sC[i]) atomicAdd(&cnt[i], sC[i]);
    }
}

// The integers as floats: one thread per (b, r).
__global__ __launch_bounds__(RS_THREADS) void region_finalize_kernel(const u64* __restrict__ acc, const unsigned* __restrict__ cnt,
                                                                     const unsigned* __restrict__ peak, int* __restrict__ count,
                                                                     float* __restrict__ sum, float* __restrict__ abs_sum,
                                                                     float* __restrict__ pos_sum, float* __restrict__ max_value,
                                                                     int* __restrict__ argmax, int B, int R, int shift) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= B * (R + 1)) return;
    const int b = i / (R + 1), r = i - b * (R + 1);
    const u64* g = acc + (size_t)b * 3 * (R + 1);
    const u64 P = g[r], Ng = g[(R + 1) + r], M = g[2 * (R + 1) + r];
    const double back = ldexp(1.0, rs_exp(peak[b]) - shift);
    if (sum) sum[i] = (float)((double)((long long)P - (long long)Ng) * back);
    if (abs_sum) abs_sum[i] = (float)((double)(P + Ng) * back);
    if (pos_sum) pos_sum[i] = (float)((double)P * back);
    if (max_value) max_value[i] = M ? fc_value((unsigned)(M >> 32)) : -INFINITY;       // M == 0: no voxel (~index is never 0)
    if (argmax) argmax[i] = M ? (int)~(unsigned)M : -1;
    if (b == 0) count[r] = (int)cnt[r];
}

// state[c][r] = (n, sum x, sum x^2) += the samples of class c in ascending b: one thread per (c, r), r = first .. R, no atomics.
// values [B][R+1-first]: column j is region first + j.  (x is a float widened to double, so x*x is exact in fp64: a fused
// multiply-add gives the bits of the rounded product plus the sum, and the loop equals its numpy restatement bit for bit.)
__global__ __launch_bounds__(RS_THREADS) void region_group_kernel(const float* __restrict__ values, const long long* __restrict__ cls,
                                                                  double* __restrict__ state, int B, int R, int C, int first) {
    const int cols = R + 1 - first;
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= C * cols) return;
    const int c = i / cols, j = i - c * cols;
    double* st = state + 3 * ((size_t)c * (R + 1) + first + j);
    double n = st[0], sx = st[1], sxx = st[2];
    for (int b = 0; b < B; ++b) {
        if (cls[b] != c) continue;
        const double x = (double)values[(size_t)b * cols + j];
        n += 1.0;
        sx += x;
        sxx += x * x;
    }
    st[0] = n;
    st[1] = sx;
    st[2] = sxx;
}

// ---- host side ----

bool rs_al(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

int rs_blocks(long items, int outer) {
    long n = (items + (long)RS_THREADS * RS_ITEMS - 1) / ((long)RS_THREADS * RS_ITEMS);
    long cap = RS_MAX_BLOCKS / outer;
    if (cap < 1) cap = 1;
    return (int)(n < 1 ? 1 : n > cap ? cap : n);
}

bool rs_takes(int B, long V, int R) { return B >= 1 && B <= RS_MAX_BLOCKS && V >= 1 && V <= INT_MAX && R >= 1 && R <= TMF_REGION_MAX; }

}  // namespace

extern "C" size_t tmf_region_workspace_bytes(int B, long V, int R) {
    if (!rs_takes(B, V, R)) return 0;
    const size_t n = rs_acc_bytes(B, R) + (size_t)(R + 1) * sizeof(unsigned) + (size_t)B * sizeof(unsigned);
    return (n + 15) & ~(size_t)15;
}

extern "C" int tmf_region_stats(const float* a, const int* labels, int* count, float* sum, float* abs_sum, float* pos_sum,
                                float* max_value, int* argmax, void* workspace, size_t workspace_bytes, int B, long V, int R,
                                void* stream) {
    TMF_REQUIRE_PTR(a); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(count); TMF_REQUIRE_PTR(workspace);
    TMF_REQUIRE(B >= 1 && B <= RS_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", __func__, B, RS_MAX_BLOCKS);
    TMF_REQUIRE(V >= 1 && V <= INT_MAX, TMF_E_SHAPE, "%s: V = %ld does not lie in 1 .. 2^31 - 1", __func__, V);
    TMF_REQUIRE(R >= 1 && R <= TMF_REGION_MAX, TMF_E_ARG, "%s: R = %d regions (1 .. %d)", __func__, R, TMF_REGION_MAX);
    TMF_REQUIRE(rs_al(a, 4) && rs_al(labels, 4) && rs_al(count, 4) && rs_al(sum, 4) && rs_al(abs_sum, 4) && rs_al(pos_sum, 4) &&
                    rs_al(max_value, 4) && rs_al(argmax, 4),
                TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE_ALIGNED(workspace);
    const size_t need = tmf_region_workspace_bytes(B, V, R);
    TMF_REQUIRE(workspace_bytes >= need, TMF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    u64* acc = static_cast<u64*>(workspace);
    unsigned* cnt = reinterpret_cast<unsigned*>(static_cast<char*>(workspace) + rs_acc_bytes(B, R));
    unsigned* peak = cnt + (R + 1);
    const int v = (int)V;
    int lg = 0;                                             // ceil(log2 V)
    while (((long)1 << lg) < V) ++lg;
    const int shift = 62 - lg;
    const bool vec = v % 4 == 0 && rs_al(a, 16) && rs_al(labels, 16);
    const int nblk = rs_blocks(vec ? v / 4 : v, B);
    hipError_t e = hipMemsetAsync(workspace, 0, need, s);
    if (e != hipSuccess) {
        tmf_set_error("%s: clearing the workspace failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    const dim3 grid(B * nblk), block(RS_THREADS);
    if (vec) {
        hipLaunchKernelGGL((region_peak_kernel<true>), grid, block, 0, s, a, peak, v, nblk);
        hipLaunchKernelGGL((region_accum_kernel<true>), grid, block, 0, s, a, labels, acc, cnt, peak, v, R, shift, nblk);
    } else {
        hipLaunchKernelGGL((region_peak_kernel<false>), grid, block, 0, s, a, peak, v, nblk);
        hipLaunchKernelGGL((region_accum_kernel<false>), grid, block, 0, s, a, labels, acc, cnt, peak, v, R, shift, nblk);
    }
    hipLaunchKernelGGL(region_finalize_kernel, dim3(tmf_cdiv((long)B * (R + 1), RS_THREADS)), block, 0, s, acc, cnt, peak, count, sum,
                       abs_sum, pos_sum, max_value, argmax, B, R, shift);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_region_group_update(const float* values, const int64_t* cls, double* state, int B, int R, int C, int first,
                                       void* stream) {
    TMF_REQUIRE_PTR(values); TMF_REQUIRE_PTR(cls); TMF_REQUIRE_PTR(state);
    TMF_REQUIRE(B >= 1 && B <= RS_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", __func__, B, RS_MAX_BLOCKS);
    TMF_REQUIRE(R >= 1 && R <= TMF_REGION_MAX, TMF_E_ARG, "%s: R = %d regions (1 .. %d)", __func__, R, TMF_REGION_MAX);
    TMF_REQUIRE(C >= 1 && C <= TMF_REGION_MAX_CLASSES, TMF_E_ARG, "%s: C = %d classes (1 .. %d)", __func__, C, TMF_REGION_MAX_CLASSES);
    TMF_REQUIRE(first == 0 || first == 1, TMF_E_ARG, "%s: first = %d (0: values [B][R+1], 1: values [B][R])", __func__, first);
    TMF_REQUIRE(rs_al(values, 4) && rs_al(cls, 8) && rs_al(state, 8), TMF_E_ALIGN,
                "%s: values is not 4-byte or cls / state not 8-byte aligned", __func__);
    hipLaunchKernelGGL(region_group_kernel, dim3(tmf_cdiv((long)C * (R + 1 - first), RS_THREADS)), dim3(RS_THREADS), 0,
                       (hipStream_t)stream, values, reinterpret_cast<const long long*>(cls), state, B, R, C, first);
    return tmf_launch_result(__func__);
}
