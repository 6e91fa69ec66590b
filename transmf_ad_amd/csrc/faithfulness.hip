// faithfulness.hip — deletion / insertion curves (include/tmf_hip.h states the semantics): the ranking (tmf_rank_thresholds:
// for every count n_k the n_k-th largest attribution of a row and the number of voxels at or above it, by a multi-quantile
// radix select, no sort) and the rank masks (tmf_mask_by_rank: K masked copies of volumes in ONE launch, the bits of
// torch.where).  gfx950.
//
// The select works on the order-preserving uint32 image of a = attr + 0.0f (fc_key) in three digits of 11, 11 and 10 bits,
// from the top.  Per digit one histogram launch over the rows and one small scan launch that walks, a wave per step k, the
// bins from the top down to the one holding rank n_k, and keeps the rank that remains inside it and the count above it.
// Digit 0 counts every voxel (LDS histogram per workgroup, flushed by integer atomics).  Digits 1 and 2 count only voxels whose
// prefix is one of the at most S selected ones: a workgroup keeps the histograms of FC_GROUP of them in LDS and flushes the
// same way, the groups share the row through the second grid dimension.  Integer counting only: two calls give the same
// bits.  Seven stream operations whatever B and V: one memset of the workspace and six launches.
#include "tmf_device.h"
#include <limits.h>

namespace {

constexpr int FC_THREADS = 256;
constexpr int FC_ITEMS = 4;                // items a lane walks at least, the row permitting
constexpr long FC_MAX_BLOCKS = 1 << 16;    // workgroups of a launch over all jobs / rows
constexpr int FC_STEPS = TMF_RANK_MAX_STEPS;
constexpr int FC_BINS = 2048;              // 11-bit digits 0 and 1; digit 2 has FC_BINS / 2
constexpr int FC_GROUP = 4;                // selected prefixes a workgroup of digits 1 and 2 counts in LDS
constexpr int FC_STATE = 4 * FC_STEPS;     // words of a row's state: the prefix after digit 0, after digit 1, rem, above [FC_STEPS] each

static_assert(FC_STEPS == 64, "one lane per step in fc_changes");

struct FcCounts {
    int n[FC_STEPS];
};

// workspace of row b (uint32 words): hist0 [2048] | hist1 [S][2048] | hist2 [S][1024] | state [FC_STATE]
__host__ __device__ inline long fc_row_words(int S) { return FC_BINS + (long)S * FC_BINS + (long)S * (FC_BINS / 2) + FC_STATE; }
__device__ __forceinline__ unsigned* fc_hist(unsigned* row, int S, int digit) {
    return digit == 0 ? row : digit == 1 ? row + FC_BINS : row + FC_BINS + (long)S * FC_BINS;
}
__device__ __forceinline__ unsigned* fc_state(unsigned* row, int S) { return row + FC_BINS + (long)S * FC_BINS + (long)S * (FC_BINS / 2); }

// fc_key / fc_value (tmf_device.h): ascending key <=> ascending a = x + 0.0f as floats

// digit 0: hist0[b][key >> 21] over all voxels of row b.  Workgroup blockIdx.x = b*nblk + blk.
template <bool VEC>
__global__ __launch_bounds__(FC_THREADS) void rank_hist0_kernel(const float* __restrict__ attr, unsigned* __restrict__ ws, int V,
                                                                int S, int nblk) {
    __shared__ unsigned h[FC_BINS];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    for (int i = threadIdx.x; i < FC_BINS; i += FC_THREADS) h[i] = 0;
    __syncthreads();
    const float* src = attr + (size_t)b * V;
    const long step = (long)nblk * FC_THREADS;
    if (VEC) {
        const long n4 = V >> 2;
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < n4; i += step) {
            const f32x4 v = TmfIO<float, 4>::ld(src + (i << 2));
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(&h[fc_key(v[q]) >> 21], 1u);
        }
    } else {
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < V; i += step) atomicAdd(&h[fc_key(src[i]) >> 21], 1u);
    }
    __syncthreads();
    unsigned* g = fc_hist(ws + (size_t)b * fc_row_words(S), S, 0);
    for (int i = threadIdx.x; i < FC_BINS; i += FC_THREADS)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// Digits 1 and 2 (DIGIT 1: prefix = key >> 21, bin = key >> 10 & 2047; DIGIT 2: prefix = key >> 10, bin = key & 1023): per
// selected prefix a histogram of the voxels that carry it.  The distinct prefixes of the previous digit (`prev`, one per k, not
// increasing with k) are numbered in k order: slot(k) = the number of changes up to k.  Workgroup (b*nblk + blk, group) counts
// the slots group*FC_GROUP .. +FC_GROUP-1 of its voxels in LDS (a voxel is compared with FC_GROUP prefixes, no search) and
// flushes the non-zero bins by integer atomics; groups past the last slot leave at once.  attr is read once per group, from
// the caches.
template <int DIGIT> struct FcDigit {
    static constexpr int NB = DIGIT == 1 ? FC_BINS : FC_BINS / 2;
    static __device__ __forceinline__ unsigned prefix(unsigned key) { return DIGIT == 1 ? key >> 21 : key >> 10; }
    static __device__ __forceinline__ unsigned bin(unsigned key) { return DIGIT == 1 ? (key >> 10) & (FC_BINS - 1) : key & (FC_BINS / 2 - 1); }
};

// slot of step k among the distinct values of prev[0..S) and their number, for a whole wave: lane l holds prev[l]
__device__ __forceinline__ unsigned long long fc_changes(const unsigned* __restrict__ prev, int S, int lane, unsigned& mine) {
    mine = lane < S ? prev[lane] : 0u;
    const unsigned before = lane >= 1 && lane < S ? prev[lane - 1] : 0u;
    return __ballot(lane < S && (lane == 0 || mine != before));
}
__device__ __forceinline__ int fc_slot(unsigned long long changes, int k) {
    return __popcll(changes & (~0ull >> (63 - k))) - 1;
}

template <bool VEC, int DIGIT>
__global__ __launch_bounds__(FC_THREADS) void rank_hist_sel_kernel(const float* __restrict__ attr, unsigned* __restrict__ ws,
                                                                   int V, int S, int nblk) {
    constexpr int NB = FcDigit<DIGIT>::NB;
    __shared__ unsigned h[FC_GROUP * NB];
    __shared__ unsigned sel[FC_GROUP];
    __shared__ int nsel_s;
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk, group = blockIdx.y;
    unsigned* row = ws + (size_t)b * fc_row_words(S);
    const unsigned* prev = fc_state(row, S) + (DIGIT - 1) * FC_STEPS;
    if (threadIdx.x < FC_GROUP) sel[threadIdx.x] = 0xFFFFFFFFu;               // no prefix has more than 22 bits
    __syncthreads();
    if (threadIdx.x < 64) {
        unsigned mine;
        const unsigned long long changes = fc_changes(prev, S, threadIdx.x, mine);
        if ((changes >> threadIdx.x) & 1) {
            const int slot = fc_slot(changes, threadIdx.x);
            if (slot / FC_GROUP == group) sel[slot % FC_GROUP] = mine;
        }
        if (threadIdx.x == 0) nsel_s = __popcll(changes);
    }
    for (int i = threadIdx.x; i < FC_GROUP * NB; i += FC_THREADS) h[i] = 0;
    __syncthreads();
    if (group * FC_GROUP >= nsel_s) return;                                      // the whole workgroup
    unsigned s4[FC_GROUP];
#pragma unroll
    for (int g = 0; g < FC_GROUP; ++g) s4[g] = sel[g];
    const float* src = attr + (size_t)b * V;
    const long step = (long)nblk * FC_THREADS;
    auto count = [&](float x) {
        const unsigned key = fc_key(x), p = FcDigit<DIGIT>::prefix(key), bin = FcDigit<DIGIT>::bin(key);
#pragma unroll
        for (int g = 0; g < FC_GROUP; ++g)
            if (p == s4[g]) atomicAdd(&h[g * NB + bin], 1u);
    };
    if (VEC) {
        const long n4 = V >> 2;
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < n4; i += step) {
            const f32x4 v = TmfIO<float, 4>::ld(src + (i << 2));
#pragma unroll
            for (int q = 0; q < 4; ++q) count(v[q]);
        }
    } else {
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < V; i += step) count(src[i]);
    }
    __syncthreads();
    unsigned* hist = fc_hist(row, S, DIGIT) + (size_t)group * FC_GROUP * NB;
    const int live = min(FC_GROUP, S - group * FC_GROUP) * NB;                   // the slots below S: hist is [S][NB]
    for (int i = threadIdx.x; i < live; i += FC_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// After digit STAGE: the bin, from the top, that holds the rank step k still wants inside the prefix selected so far.  One
// wave per (row, k), workgroup b*S + k: lane l sums the NB / 64 bins [(63 - l) * NB / 64, ...) of the step's histogram, a scan over the lanes
// finds the lane that holds the rank, that lane walks its bins.  STAGE 0 and 1 leave the step's new prefix (in an array of
// their own: the other steps' waves read the previous one), the rank that remains and the count above; STAGE 2 writes thr
// and removed.
template <int STAGE>
__global__ __launch_bounds__(64) void rank_scan_kernel(unsigned* __restrict__ ws, FcCounts counts, int S, float* __restrict__ thr,
                                                       int* __restrict__ removed) {
    constexpr int NB = STAGE == 2 ? FC_BINS / 2 : FC_BINS;
    constexpr int PER = NB / 64;
    const int b = blockIdx.x / S, k = blockIdx.x - b * S, lane = threadIdx.x;
    unsigned* row = ws + (size_t)b * fc_row_words(S);
    unsigned* st = fc_state(row, S);
    unsigned *rem = st + 2 * FC_STEPS, *above = st + 3 * FC_STEPS;
    unsigned want = (unsigned)counts.n[k], ab = 0, pf = 0;
    int slot = 0;
    if (STAGE > 0) {
        unsigned mine;
        const unsigned long long changes = fc_changes(st + (STAGE - 1) * FC_STEPS, S, lane, mine);
        slot = fc_slot(changes, k);
        slot = slot < 0 ? 0 : slot >= S ? S - 1 : slot;
        pf = (unsigned)__shfl((int)mine, k);
        want = rem[k];
        ab = above[k];
    }
    const unsigned* h = fc_hist(row, S, STAGE) + (size_t)slot * NB;
    const int base = (63 - lane) * PER;
    unsigned c[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; i += 4) {
        const tmf_u32x4 q = *reinterpret_cast<const tmf_u32x4*>(h + base + i);
        c[i] = q[0]; c[i + 1] = q[1]; c[i + 2] = q[2]; c[i + 3] = q[3];
        sum += q[0] + q[1] + q[2] + q[3];
    }
    unsigned inc = sum;                                  // bins of lanes 0..lane: the top of the histogram down to `base`
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = (unsigned)__shfl_up((int)inc, d);
        if (lane >= d) inc += t;
    }
    const unsigned long long holds = __ballot(inc >= want);
    const int owner = holds ? __ffsll((long long)holds) - 1 : 63;      // (holds != 0: the histogram counts >= want voxels)
    unsigned r = want - (inc - sum), abv = ab + (inc - sum), bin = (unsigned)base, cnt = 0;
    bool done = false;
#pragma unroll
    for (int i = PER - 1; i >= 0; --i) {
        if (!done) {
            if (r <= c[i] || i == 0) {
                bin = (unsigned)(base + i);
                cnt = c[i];
                done = true;
            } else {
                r -= c[i];
                abv += c[i];
            }
        }
    }
    if (lane == owner) {
        if (STAGE == 2) {
            thr[(size_t)b * S + k] = fc_value((pf << 10) | bin);
            removed[(size_t)b * S + k] = (int)(abv + cnt);
        } else {
            st[STAGE * FC_STEPS + k] = STAGE == 0 ? bin : (pf << 11) | bin;
            rem[k] = r;
            above[k] = abv;
        }
    }
}

// out[k][e] for job j0 + k = b*(S+1) + s: m = s > 0 && attr[b][e] >= thr[b][s-1]; INSERT ? (m ? vol : f) : (m ? f : vol) with
// f = base[b][e] (BASE) or fill[b].  Workgroup blockIdx.x = k*nblk + blk strides over the items of job k.
template <bool VEC, bool BASE, bool INSERT>
__global__ __launch_bounds__(FC_THREADS) void mask_by_rank_kernel(const float* __restrict__ vol, const float* __restrict__ attr,
                                                                  const float* __restrict__ thr, const float* __restrict__ fill,
                                                                  const float* __restrict__ basev, float* __restrict__ out, int V,
                                                                  int S, int j0, int nblk) {
    const int k = blockIdx.x / nblk, blk = blockIdx.x - k * nblk;
    const int j = j0 + k;
    const int b = j / (S + 1), s = j - b * (S + 1);
    const bool any = s > 0;
    const float t = any ? thr[(size_t)b * S + (s - 1)] : 0.f;
    const float f = BASE ? 0.f : fill[b];
    const float* src = vol + (size_t)b * V;
    const float* at = attr + (size_t)b * V;
    const float* bs = BASE ? basev + (size_t)b * V : nullptr;
    float* dst = out + (size_t)k * V;
    const long step = (long)nblk * FC_THREADS;
    if (VEC) {
        const long n4 = V >> 2;
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < n4; i += step) {
            const int e = (int)(i << 2);
            const f32x4 v = TmfIO<float, 4>::ld(src + e), a = TmfIO<float, 4>::ld(at + e);
            f32x4 g = {f, f, f, f}, o;
            if (BASE) g = TmfIO<float, 4>::ld(bs + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bool m = any & (a[q] >= t);
                o[q] = (m != INSERT) ? g[q] : v[q];
            }
            TmfIO<float, 4>::st(dst + e, o);
        }
    } else {
        for (long i = (long)blk * FC_THREADS + threadIdx.x; i < V; i += step) {
            const int e = (int)i;
            const bool m = any & (at[e] >= t);
            const float g = BASE ? bs[e] : f;
            dst[e] = (m != INSERT) ? g : src[e];
        }
    }
}

// ---- host side ----

bool fc_f32(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool fc_vec(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// workgroups per job / row: `items` strided by lanes that walk FC_ITEMS each, `outer` jobs share FC_MAX_BLOCKS
int fc_blocks(long items, int outer) {
    long n = (items + (long)FC_THREADS * FC_ITEMS - 1) / ((long)FC_THREADS * FC_ITEMS);
    long cap = FC_MAX_BLOCKS / outer;
    if (cap < 1) cap = 1;
    return (int)(n < 1 ? 1 : n > cap ? cap : n);
}

int fc_shape(const char* fn, int B, long V, int S) {
    TMF_REQUIRE(B >= 1, TMF_E_SHAPE, "%s: B = %d", fn, B);
    TMF_REQUIRE(V >= 1 && V <= INT_MAX, TMF_E_SHAPE, "%s: V = %ld does not lie in 1 .. 2^31 - 1", fn, V);
    TMF_REQUIRE(S >= 1 && S <= FC_STEPS, TMF_E_ARG, "%s: S = %d steps (1 .. %d)", fn, S, FC_STEPS);
    return TMF_OK;
}

}  // namespace

extern "C" size_t tmf_rank_workspace_bytes(int B, long V, int S) {
    if (B < 1 || V < 1 || S < 1 || S > FC_STEPS) return 0;
    return (size_t)B * (size_t)fc_row_words(S) * sizeof(unsigned);
}

extern "C" int tmf_rank_thresholds(const float* attr, const int* counts, float* thr, int* removed, void* workspace,
                                   size_t workspace_bytes, int B, long V, int S, void* stream) {
    TMF_REQUIRE_PTR(attr); TMF_REQUIRE_PTR(counts); TMF_REQUIRE_PTR(thr); TMF_REQUIRE_PTR(removed); TMF_REQUIRE_PTR(workspace);
    TMF_TRY(fc_shape(__func__, B, V, S));
    TMF_REQUIRE(B <= FC_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", __func__, B, FC_MAX_BLOCKS);
    FcCounts c;
    for (int k = 0; k < FC_STEPS; ++k) c.n[k] = 0;
    for (int k = 0; k < S; ++k) {
        TMF_REQUIRE(counts[k] >= 1 && counts[k] <= V, TMF_E_ARG, "%s: counts[%d] = %d does not lie in 1 .. V = %ld", __func__, k,
                    counts[k], V);
        TMF_REQUIRE(k == 0 || counts[k] >= counts[k - 1], TMF_E_ARG, "%s: counts[%d] = %d < counts[%d] = %d: counts must not decrease",
                    __func__, k, counts[k], k - 1, counts[k - 1]);
        c.n[k] = counts[k];
    }
    TMF_REQUIRE(fc_f32(attr) && fc_f32(thr) && fc_f32(removed), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE_ALIGNED(workspace);
    const size_t need = tmf_rank_workspace_bytes(B, V, S);
    TMF_REQUIRE(workspace_bytes >= need, TMF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    unsigned* ws = static_cast<unsigned*>(workspace);
    const int v = (int)V;
    const bool vec = v % 4 == 0 && fc_vec(attr);
    const int nblk = fc_blocks(vec ? v / 4 : v, B);
    const int groups = (S + FC_GROUP - 1) / FC_GROUP;
    hipError_t e = hipMemsetAsync(workspace, 0, need, s);
    if (e != hipSuccess) {
        tmf_set_error("%s: clearing the workspace failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    if (vec) hipLaunchKernelGGL((rank_hist0_kernel<true>), dim3(B * nblk), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    else hipLaunchKernelGGL((rank_hist0_kernel<false>), dim3(B * nblk), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    hipLaunchKernelGGL((rank_scan_kernel<0>), dim3(B * S), dim3(64), 0, s, ws, c, S, thr, removed);
    if (vec) hipLaunchKernelGGL((rank_hist_sel_kernel<true, 1>), dim3(B * nblk, groups), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    else hipLaunchKernelGGL((rank_hist_sel_kernel<false, 1>), dim3(B * nblk, groups), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    hipLaunchKernelGGL((rank_scan_kernel<1>), dim3(B * S), dim3(64), 0, s, ws, c, S, thr, removed);
    if (vec) hipLaunchKernelGGL((rank_hist_sel_kernel<true, 2>), dim3(B * nblk, groups), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    else hipLaunchKernelGGL((rank_hist_sel_kernel<false, 2>), dim3(B * nblk, groups), dim3(FC_THREADS), 0, s, attr, ws, v, S, nblk);
    hipLaunchKernelGGL((rank_scan_kernel<2>), dim3(B * S), dim3(64), 0, s, ws, c, S, thr, removed);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_mask_by_rank(const float* vol, const float* attr, const float* thr, const float* fill, const float* base,
                                float* out, int B, long V, int S, int mode, int j0, int K, void* stream) {
    TMF_REQUIRE_PTR(vol); TMF_REQUIRE_PTR(attr); TMF_REQUIRE_PTR(thr); TMF_REQUIRE_PTR(out);
    TMF_REQUIRE(base != nullptr || fill != nullptr, TMF_E_NULL, "%s: 'fill' and 'base' are both NULL", __func__);
    TMF_TRY(fc_shape(__func__, B, V, S));
    TMF_REQUIRE(mode == TMF_RANK_DELETION || mode == TMF_RANK_INSERTION, TMF_E_ARG, "%s: mode = %d", __func__, mode);
    const long long jobs = (long long)B * (S + 1);
    TMF_REQUIRE(jobs <= INT_MAX, TMF_E_SHAPE, "%s: B * (S + 1) = %d * %d does not stay below 2^31", __func__, B, S + 1);
    TMF_REQUIRE(K >= 1 && j0 >= 0, TMF_E_ARG, "%s: jobs j0 = %d, K = %d", __func__, j0, K);
    TMF_REQUIRE((long long)j0 + K <= jobs, TMF_E_ARG, "%s: jobs %d .. %lld of %lld", __func__, j0, (long long)j0 + K - 1, jobs);
    TMF_REQUIRE(K <= FC_MAX_BLOCKS, TMF_E_ARG, "%s: K = %d jobs in one call (at most %ld)", __func__, K, FC_MAX_BLOCKS);
    TMF_REQUIRE(fc_f32(vol) && fc_f32(attr) && fc_f32(thr) && fc_f32(fill) && fc_f32(base) && fc_f32(out), TMF_E_ALIGN,
                "%s: a pointer is not 4-byte aligned", __func__);
    hipStream_t s = (hipStream_t)stream;
    const int v = (int)V;
    const bool vec = v % 4 == 0 && fc_vec(vol) && fc_vec(attr) && fc_vec(out) && fc_vec(base);
    const int nblk = fc_blocks(vec ? v / 4 : v, K);
    const dim3 grid(K * nblk), block(FC_THREADS);
#define FC_LAUNCH(VEC, BASE, INS) \
    hipLaunchKernelGGL((mask_by_rank_kernel<VEC, BASE, INS>), grid, block, 0, s, vol, attr, thr, fill, base, out, v, S, j0, nblk)
    const int variant = (vec ? 4 : 0) | (base ? 2 : 0) | (mode == TMF_RANK_INSERTION ? 1 : 0);
    switch (variant) {
        case 0: FC_LAUNCH(false, false, false); break;
        case 1: FC_LAUNCH(false, false, true); break;
        case 2: FC_LAUNCH(false, true, false); break;
        case 3: FC_LAUNCH(false, true, true); break;
        case 4: FC_LAUNCH(true, false, false); break;
        case 5: FC_LAUNCH(true, false, true); break;
        case 6: FC_LAUNCH(true, true, false); break;
        default: FC_LAUNCH(true, true, true); break;
    }
#undef FC_LAUNCH
    return tmf_launch_result(__func__);
}
