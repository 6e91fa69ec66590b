// cam.hip — class activation maps on a channels-last activation A[B][V][C] and its gradient G[B][V][C] (tmf_cam): Grad-CAM
// (weights = the mean of G over the voxels, map = the weighted channel sum of A) and HiResCAM (map = the channel sum of G * A).
// gfx950.  A and G are read ONCE from HBM with 16-byte loads along C; no atomics — the column sums over V and the per-sample
// maximum go through per-workgroup partials in the workspace, combined in a fixed order by every workgroup that needs them, so
// two calls give the same bits.  Launches: Grad = column partials, map, normalise; HiRes = map, normalise (the last one only when
// TMF_CAM_NORMALIZE or `peak` asks for it).  tmf_reduce_slabs is not used for the column sums: it would be a launch (two above 64
// slabs) between the partials and the map, and the launch budget of the Grad method is three.
#include "tmf_common.h"
#include <math.h>

namespace {

constexpr int CAM_THREADS = 256;
constexpr int CAM_U = 4;                 // row passes a workgroup keeps in flight (2 x CAM_U 16-byte loads per lane)
constexpr int CAM_COL_BLOCKS = 64;       // most column-sum workgroups per sample (the map kernel re-adds that many partials)
constexpr int CAM_COL_PASSES = 16;       // ... each with at least this many row passes, the volume permitting

// A row of C floats is read by L lanes (a power of two >= C / 4, at most 64), 16 bytes per lane and step: lane cl holds the
// channel quads cl, cl + L (KMAX = 2 only for L == 64, C > 256); quads at or beyond C / 4 read nothing and count as zeros.
// A workgroup covers RP = 256 / L rows per pass.
template <int L> struct CamGeom {
    static constexpr int KMAX = L == 64 ? 2 : 1;
    static constexpr int RP = CAM_THREADS / L;
};

// Pass 1 of the Grad method: colpart[blk][b][c] = sum of G[b][v][c] over the rows v of workgroup blk's chunk, in fp64 (the
// per-channel sums cancel: the means of G have mixed signs and are small against its elements).  Every element is written.
template <int L>
__global__ __launch_bounds__(CAM_THREADS) void cam_colsum_kernel(const float* __restrict__ G, double* __restrict__ colpart,
                                                                 int B, long V, int C, int nblk) {
    constexpr int KMAX = CamGeom<L>::KMAX, RP = CamGeom<L>::RP;
    __shared__ double red[CAM_THREADS / 64][L * KMAX * 4];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int cl = threadIdx.x % L, row = threadIdx.x / L, C4 = C >> 2;
    const long chunk = (V + nblk - 1) / nblk;
    const long r_begin = (long)blk * chunk;
    const long r_end = r_begin + chunk < V ? r_begin + chunk : V;
    const float* Gb = G + (size_t)b * V * C;
    double acc[KMAX][4];
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[j][e] = 0.0;
    for (long r0 = r_begin; r0 < r_end; r0 += RP * CAM_U) {
        f32x4 g[CAM_U][KMAX];
#pragma unroll
        for (int u = 0; u < CAM_U; ++u) {
            const long r = r0 + u * RP + row;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                const int c4 = cl + j * L;
                g[u][j] = (r < r_end && c4 < C4) ? TmfIO<float, 4>::ld_nt(Gb + (size_t)r * C + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int u = 0; u < CAM_U; ++u)
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[j][e] += (double)g[u][j][e];
    }
    // the rows of one wave that hold the same channel quad sit L lanes apart; then the four waves through LDS, in wave order
#pragma unroll
    for (int o = L; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] += __shfl_xor(acc[j][e], o);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane < L) {
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave][(j * L + lane) * 4 + e] = acc[j][e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += CAM_THREADS) {
        double s = red[0][c];
#pragma unroll
        for (int w = 1; w < CAM_THREADS / 64; ++w) s += red[w][c];
        colpart[((size_t)blk * B + b) * C + c] = s;
    }
}

// The map.  HIRES: cam[b][v] = sum_c G * A.  Grad: every workgroup first adds the ncol column partials of its sample in slab order
// (fp64, one rounding) into w[c] = sum / V — workgroup 0 of the sample stores `weights` — then cam[b][v] = sum_c w[c] A[b][v][c].
// The dot over C: four fmas per lane and quad, then a butterfly over the row's L lanes.  relu clamps before the store and
// before the maximum; pmax[b][blk] = the maximum of the workgroup's rows (every workgroup owns at least one row).
template <int L, bool HIRES>
__global__ __launch_bounds__(CAM_THREADS) void cam_map_kernel(const float* __restrict__ A, const float* __restrict__ G,
                                                              const double* __restrict__ colpart, float* __restrict__ cam,
                                                              float* __restrict__ weights, float* __restrict__ pmax, int B, long V,
                                                              int C, int nblk, int ncol, int relu) {
    constexpr int KMAX = CamGeom<L>::KMAX, RP = CamGeom<L>::RP;
    __shared__ __attribute__((aligned(16))) float w_s[HIRES ? 4 : 512];
    __shared__ float m_s[CAM_THREADS / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const int cl = threadIdx.x % L, row = threadIdx.x / L, C4 = C >> 2;
    f32x4 wv[KMAX];
    if (!HIRES) {
        // kg = 256 / C thread groups (1 above 128 channels) share the slabs of a column: group q adds slabs q, q + kg, ... in
        // that order, then one thread per column adds the groups in group order — the loads of a thread are independent, so
        // the chain a workgroup waits for is ncol / kg loads deep instead of ncol
        __shared__ double part_s[CAM_THREADS];
        const int kg = C <= CAM_THREADS ? CAM_THREADS / C : 1;
        for (int c0 = 0; c0 < C; c0 += CAM_THREADS) {
            const int c = c0 + (int)threadIdx.x % (kg > 1 ? C : CAM_THREADS), q = kg > 1 ? (int)threadIdx.x / C : 0;
            double s = 0.0;
            if (c < C && q < kg) {
#pragma unroll 8
                for (int k = q; k < ncol; k += kg) s += colpart[((size_t)k * B + b) * C + c];
            }
            if (c0 > 0) __syncthreads();                    // (C = 512: the second half reuses part_s)
            part_s[threadIdx.x] = s;
            __syncthreads();
            if (q == 0 && c < C) {
                for (int i = 1; i < kg; ++i) s += part_s[i * C + (c - c0)];
                const float w = (float)(s / (double)V);
                w_s[c] = w;
                if (blk == 0 && weights != nullptr) weights[(size_t)b * C + c] = w;
            }
        }
        if (cam == nullptr) return;          // weights alone were asked for (uniform over the grid)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            const int c4 = cl + j * L;
            wv[j] = c4 < C4 ? *reinterpret_cast<const f32x4*>(&w_s[4 * c4]) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    const float* Ab = A + (size_t)b * V * C;
    const float* Gb = G + (size_t)b * V * C;
    float* camb = cam + (size_t)b * V;
    float m = -INFINITY;
    for (long r0 = (long)blk * (RP * CAM_U); r0 < V; r0 += (long)nblk * (RP * CAM_U)) {
        f32x4 a[CAM_U][KMAX], g[CAM_U][KMAX];
#pragma unroll
        for (int u = 0; u < CAM_U; ++u) {
            const long r = r0 + u * RP + row;
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                const int c4 = cl + j * L;
                const bool ok = r < V && c4 < C4;
                a[u][j] = ok ? TmfIO<float, 4>::ld_nt(Ab + (size_t)r * C + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                if (HIRES) g[u][j] = ok ? TmfIO<float, 4>::ld_nt(Gb + (size_t)r * C + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
                else g[u][j] = wv[j];
            }
        }
#pragma unroll
        for (int u = 0; u < CAM_U; ++u) {
            const long r = r0 + u * RP + row;
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < KMAX; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(a[u][j][e], g[u][j][e], s);
#pragma unroll
            for (int o = L / 2; o > 0; o >>= 1) s += __shfl_xor(s, o);
            if (relu) s = fmaxf(s, 0.f);
            if (r < V) {
                if (cl == 0) camb[r] = s;
                m = fmaxf(m, s);
            }
        }
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) m_s[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < CAM_THREADS / 64; ++w) m = fmaxf(m, m_s[w]);
        pmax[(size_t)b * nblk + blk] = m;
    }
}

// peak[b] = the maximum of the sample's nmap workgroup maxima; normalize: cam[b][v] /= peak, zeros where the peak is <= 0.
__global__ __launch_bounds__(CAM_THREADS) void cam_norm_kernel(float* __restrict__ cam, const float* __restrict__ pmax,
                                                               float* __restrict__ peak, long V, int nmap, int nblk, int normalize) {
    __shared__ float m_s[CAM_THREADS / 64];
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nmap; i += CAM_THREADS) m = fmaxf(m, pmax[(size_t)b * nmap + i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) m_s[threadIdx.x >> 6] = m;
    __syncthreads();
    m = m_s[0];
#pragma unroll
    for (int w = 1; w < CAM_THREADS / 64; ++w) m = fmaxf(m, m_s[w]);
    if (blk == 0 && threadIdx.x == 0 && peak != nullptr) peak[b] = m;
    if (!normalize) return;
    float* camb = cam + (size_t)b * V;
    const bool live = m > 0.f;
    for (long i = (long)blk * CAM_THREADS + threadIdx.x; i < V; i += (long)nblk * CAM_THREADS) camb[i] = live ? camb[i] / m : 0.f;
}

int cam_lanes(int C) {
    int L = 2;
    while (L < 64 && L * 4 < C) L <<= 1;
    return L;
}

// Workspace: [colpart: nblk_col x B x C doubles (Grad only)] [pmax: B x nblk_map floats], each on a 256-byte granule.
struct CamPlan {
    int L, nblk_col, nblk_map, nblk_norm;
    size_t off_pmax, bytes;
};

CamPlan cam_plan(int B, long V, int C, int method) {
    CamPlan p;
    p.L = cam_lanes(C);
    const long rp = CAM_THREADS / p.L;
    long n = (V + rp * CAM_COL_PASSES - 1) / (rp * CAM_COL_PASSES);
    p.nblk_col = method == TMF_CAM_GRAD ? (int)(n < 1 ? 1 : n > CAM_COL_BLOCKS ? CAM_COL_BLOCKS : n) : 0;
    long cap = (2048 + B - 1) / B;              // about eight workgroups per compute unit over the whole batch
    if (cap < 8) cap = 8;
    n = (V + rp * CAM_U - 1) / (rp * CAM_U);
    p.nblk_map = (int)(n > cap ? cap : n);
    n = (V + 8 * CAM_THREADS - 1) / (8 * CAM_THREADS);
    p.nblk_norm = (int)(n > 64 ? 64 : n);
    p.off_pmax = up256((size_t)p.nblk_col * B * C * sizeof(double));
    p.bytes = p.off_pmax + up256((size_t)B * p.nblk_map * sizeof(float));
    return p;
}

bool cam_shape_ok(int B, long V, int C, int method) {
    return B >= 1 && V >= 1 && tmf_cam_ok(C) && (method == TMF_CAM_GRAD || method == TMF_CAM_HIRES) &&
           B <= (1 << 20);     // the grids (B x at most max(8, 2048 / B) workgroups) stay far inside 32 bits
}

template <int L>
int cam_launch(const CamPlan& p, const float* act, const float* grad, float* cam, float* weights, float* peak, char* ws, int B,
               long V, int C, int method, int flags, hipStream_t s) {
    double* colpart = reinterpret_cast<double*>(ws);
    float* pmax = reinterpret_cast<float*>(ws + p.off_pmax);
    const int relu = (flags & TMF_CAM_RELU) != 0;
    if (method == TMF_CAM_GRAD) {
        hipLaunchKernelGGL(cam_colsum_kernel<L>, dim3(B * p.nblk_col), dim3(CAM_THREADS), 0, s, grad, colpart, B, V, C, p.nblk_col);
        TMF_TRY(tmf_launch_result("tmf_cam", "(column sums)"));
        const int nblk = cam != nullptr ? p.nblk_map : 1;
        hipLaunchKernelGGL((cam_map_kernel<L, false>), dim3(B * nblk), dim3(CAM_THREADS), 0, s, act, grad,
                           (const double*)colpart, cam, weights, pmax, B, V, C, nblk, p.nblk_col, relu);
        TMF_TRY(tmf_launch_result("tmf_cam", "(grad map)"));
    } else {
        hipLaunchKernelGGL((cam_map_kernel<L, true>), dim3(B * p.nblk_map), dim3(CAM_THREADS), 0, s, act, grad,
                           (const double*)nullptr, cam, (float*)nullptr, pmax, B, V, C, p.nblk_map, 0, relu);
        TMF_TRY(tmf_launch_result("tmf_cam", "(hires map)"));
    }
    const int normalize = (flags & TMF_CAM_NORMALIZE) != 0;
    if (cam != nullptr && (normalize || peak != nullptr)) {
        const int nblk = normalize ? p.nblk_norm : 1;
        hipLaunchKernelGGL(cam_norm_kernel, dim3(B * nblk), dim3(CAM_THREADS), 0, s, cam, (const float*)pmax, peak, V, p.nblk_map,
                           nblk, normalize);
        TMF_TRY(tmf_launch_result("tmf_cam", "(normalise)"));
    }
    return TMF_OK;
}

}  // namespace

extern "C" int tmf_cam_ok(int C) { return C >= 8 && C <= 512 && C % 4 == 0; }

extern "C" size_t tmf_cam_workspace_bytes(int B, long V, int C, int method) {
    if (!cam_shape_ok(B, V, C, method)) return 0;
    return cam_plan(B, V, C, method).bytes;
}

extern "C" int tmf_cam(const float* act, const float* grad, float* cam, float* weights, float* peak, void* workspace,
                       size_t workspace_bytes, int B, long V, int C, int method, int flags, void* stream) {
    TMF_REQUIRE_PTR(act); TMF_REQUIRE_PTR(grad); TMF_REQUIRE_PTR(workspace);
    TMF_REQUIRE(method == TMF_CAM_GRAD || method == TMF_CAM_HIRES, TMF_E_ARG, "tmf_cam: unknown method %d", method);
    TMF_REQUIRE((flags & ~(TMF_CAM_RELU | TMF_CAM_NORMALIZE)) == 0, TMF_E_ARG, "tmf_cam: unknown flag bits in %d", flags);
    TMF_REQUIRE(cam != nullptr || weights != nullptr, TMF_E_NULL, "tmf_cam: cam and weights are both NULL");
    TMF_REQUIRE(weights == nullptr || method == TMF_CAM_GRAD, TMF_E_ARG, "tmf_cam: weights exist for TMF_CAM_GRAD only");
    TMF_REQUIRE(cam != nullptr || peak == nullptr, TMF_E_ARG, "tmf_cam: peak without cam");
    TMF_REQUIRE(tmf_cam_ok(C), TMF_E_SHAPE, "tmf_cam: C=%d is not a multiple of 4 in 8..512", C);
    TMF_REQUIRE(cam_shape_ok(B, V, C, method), TMF_E_SHAPE, "tmf_cam: B=%d V=%ld C=%d", B, V, C);
    TMF_REQUIRE_ALIGNED(act); TMF_REQUIRE_ALIGNED(grad); TMF_REQUIRE_ALIGNED(workspace);
    TMF_REQUIRE(((uintptr_t)cam & 3u) == 0 && ((uintptr_t)weights & 3u) == 0 && ((uintptr_t)peak & 3u) == 0, TMF_E_ALIGN,
                "tmf_cam: an output is not 4-byte aligned");
    const CamPlan p = cam_plan(B, V, C, method);
    TMF_REQUIRE(workspace_bytes >= p.bytes, TMF_E_WORKSPACE, "tmf_cam: workspace %zu B < %zu B", workspace_bytes, p.bytes);
    char* ws = static_cast<char*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    switch (p.L) {
    case 2: return cam_launch<2>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    case 4: return cam_launch<4>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    case 8: return cam_launch<8>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    case 16: return cam_launch<16>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    case 32: return cam_launch<32>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    default: return cam_launch<64>(p, act, grad, cam, weights, peak, ws, B, V, C, method, flags, s);
    }
}
