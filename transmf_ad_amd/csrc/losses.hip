// losses.hip — FALoss and SupConLoss (models/losses.py) for gfx950, fp32.
//
// FALoss:  L = sum_b sum_ij |D_b[i][j]|,  D_b = F1_b^T F1_b - F2_b^T F2_b  (N x N, N = tokens of a (B, C, h, w, d) map),
// and, when a gradient is wanted, the UNSCALED gradients  G1_b = F1_b T_b,  G2_b = -F2_b T_b  with T = sign(D), sign(0) = 0
// (dL/dF1 = 2 g G1 / (B N^2), dL/dF2 = 2 g G2 / (B N^2); 'sum' drops the divisor: tmf_faloss_bwd only scales).
// The reference builds both B x N x N matrices, their difference and its sign; here no N^2 element is ever written.
//
// A workgroup of four waves owns 32 token rows I of one sample and streams the token rows J through LDS, `tj` tiles of 32
// at a time ([token][C + 1] floats per map: conflict-free for "one token per lane" and "one channel per lane" reads).
// Wave w works on map w & 1 and channel half w >> 1: per J tile it forms its half of S_map[J, I] on
// v_mfma_f32_32x32x2_f32 (the I operand lives in C / 4 registers), the four partial tiles meet in LDS, and every wave
// forms  S1 = S1a + S1b,  S2 = S2a + S2b,  D = S1 - S2  — S1 and S2 in separate accumulators summed in the same order, so
// identical maps give D == 0 exactly and the error is that of two dot products and one subtraction.  D arrives with its
// column i on the lane and its rows j in the 16 registers: the sign tile is at once the B operand of
// G_map[:, I] += F_map[:, J] T[J, I]  (A operand: the staged panel read channel-per-lane), which the wave accumulates for
// the channel tiles dt = (w >> 1), (w >> 1) + 2, ... of its map.  Wave 0 keeps sum |D| in a double per lane.
// Ragged N: token rows past N are zero-filled, a zero token gives D = 0: nothing in the sum, sign 0.
// The per-workgroup partials (double) are reduced in a fixed order by faloss_finalize_kernel.
//
// SupConLoss: one workgroup holds the (views*bs) x (views*bs) logits in LDS: products on the VALU in 8 x 8 register tiles,
// then one wave per anchor row for the row maximum, the masked log-sum-exp and the positive mean, and — when a gradient
// is wanted — E = dL/dlogits in place of the logits and  G = (E + E^T) X / temperature  (the features sit on both sides).
//
// Replaces the reference's op sequences at models/losses.py:122-128 (FALoss.forward) and :59-100 (SupConLoss.forward)
// and their autograd backward.
#include "tmf_device.h"

namespace {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

constexpr int FA_XCH = 2 * 4 * 16 * 64;          // floats: two buffers of four partial tiles

// Stage `rows` (a multiple of 32) token rows j0.. of one sample's map into lds[row][C + 1], zero-filled past N.
// cl != 0: the map is [N][C] (channels-last storage), 16-byte loads along the channels; else [C][N]: 4-byte loads,
// 32 consecutive tokens of one channel per half wave (128-byte segments).  Eight loads in flight per thread.
template <int C>
__device__ __forceinline__ void fa_stage(float* lds, const float* __restrict__ src, int N, int cl, int j0, int rows, int tid) {
    constexpr int BATCH = 8;
    if (cl) {
        constexpr int Q = C / 4;
        const int total = rows * Q;
        for (int base = 0; base < total; base += 256 * BATCH) {
            f32x4 v[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = base + u * 256 + tid;
                const int j = j0 + e / Q;
                f32x4 t = {0.f, 0.f, 0.f, 0.f};
                if (e < total && j < N) t = *reinterpret_cast<const f32x4*>(src + (size_t)j * C + (e % Q) * 4);
                v[u] = t;
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = base + u * 256 + tid;
                if (e < total) {
                    float* d = lds + (e / Q) * (C + 1) + (e % Q) * 4;
                    d[0] = v[u][0]; d[1] = v[u][1]; d[2] = v[u][2]; d[3] = v[u][3];
                }
            }
        }
    } else {
        const int total = rows * C;              // e = ((tile * C) + c) * 32 + token-in-tile
        for (int base = 0; base < total; base += 256 * BATCH) {
            float v[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = base + u * 256 + tid;
                const int q = e >> 5;
                const int j = j0 + (q / C) * 32 + (e & 31);
                v[u] = (e < total && j < N) ? src[(size_t)(q % C) * N + j] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = base + u * 256 + tid;
                const int q = e >> 5;
                if (e < total) lds[((q / C) * 32 + (e & 31)) * (C + 1) + (q % C)] = v[u];
            }
        }
    }
}

// One 32-token tile of both maps held in registers between its global loads and its LDS writes (C <= 128: C / 4 floats
// per thread), so that the loads of tile t + 1 fly during the matrix work on tile t.  Same element order as fa_stage.
template <int C>
struct FaTileRegs {
    static constexpr int PER = C / 8;            // floats per thread and map
    float v[2 * PER];
    __device__ __forceinline__ void load(const float* __restrict__ f1b, const float* __restrict__ f2b, int N, int cl, int j0,
                                         int tid) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const float* src = m ? f2b : f1b;
            if (cl) {
#pragma unroll
                for (int u = 0; u < PER / 4; ++u) {
                    const int e = u * 256 + tid;
                    const int j = j0 + e / (C / 4);
                    f32x4 t = {0.f, 0.f, 0.f, 0.f};
                    if (j < N) t = *reinterpret_cast<const f32x4*>(src + (size_t)j * C + (e % (C / 4)) * 4);
                    v[m * PER + 4 * u] = t[0]; v[m * PER + 4 * u + 1] = t[1];
                    v[m * PER + 4 * u + 2] = t[2]; v[m * PER + 4 * u + 3] = t[3];
                }
            } else {
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const int e = u * 256 + tid;
                    const int j = j0 + (e & 31);
                    v[m * PER + u] = j < N ? src[(size_t)(e >> 5) * N + j] : 0.f;
                }
            }
        }
    }
    // panel: [map][32][C + 1]
    __device__ __forceinline__ void store(float* panel, int cl, int tid) const {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            float* dst = panel + m * 32 * (C + 1);
            if (cl) {
#pragma unroll
                for (int u = 0; u < PER / 4; ++u) {
                    const int e = u * 256 + tid;
                    float* d = dst + (e / (C / 4)) * (C + 1) + (e % (C / 4)) * 4;
                    d[0] = v[m * PER + 4 * u]; d[1] = v[m * PER + 4 * u + 1];
                    d[2] = v[m * PER + 4 * u + 2]; d[3] = v[m * PER + 4 * u + 3];
                }
            } else {
#pragma unroll
                for (int u = 0; u < PER; ++u) {
                    const int e = u * 256 + tid;
                    dst[(e & 31) * (C + 1) + (e >> 5)] = v[m * PER + u];
                }
            }
        }
    }
};

// C <= 128 (every sNet level at dim 64 and 128): tile-by-tile streaming through two LDS panels with the next tile's
// loads in flight (FaTileRegs); the I operand comes through a panel as well (coalesced).  C > 128: `tj` tiles staged per
// barrier pair (fa_stage), the I operand loaded from global memory.
template <int C, bool GRAD>
__global__ __launch_bounds__(256, C <= 128 ? 2 : 1) void faloss_kernel(          // <= 256 registers either way
    const float* __restrict__ f1, const float* __restrict__ f2, double* __restrict__ partial, float* __restrict__ g1,
    float* __restrict__ g2, int N, int cl, int tj) {
    constexpr bool PF = C <= 128;
    constexpr int CT = C / 32;                   // channel tiles
    constexpr int NK = (CT + 1) / 2;             // ... of which a wave accumulates at most NK
    constexpr int KH = C / 2;                    // channels of a wave's half
    constexpr int PANEL = 32 * (C + 1);          // floats of one tile of one map
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int JR = 32 * tj;                      // PF: tj == 2, the two panels
    float* xch = smem + 2 * JR * (C + 1);
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hsel = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int map = wave & 1, kh = wave >> 1;
    const int b = blockIdx.y, i0 = blockIdx.x * 32;
    const size_t sample = (size_t)b * C * N;
    const float* f1b = f1 + sample;
    const float* f2b = f2 + sample;

    float ireg[KH / 2];                          // B operand: F_map[c = kh*KH + 2s + hsel][i = i0 + l31]
    f32x16 gacc[NK];
#pragma unroll
    for (int k = 0; k < NK; ++k)
#pragma unroll
        for (int r = 0; r < 16; ++r) gacc[k][r] = 0.f;
    double lsum = 0.0;
    int xb = 0;

    // one J tile: pm = this wave's map, 32 token rows of C + 1 floats
    auto tile = [&](const float* pm) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        {
            const float* p = pm + l31 * (C + 1) + kh * KH + hsel;
#pragma unroll
            for (int s = 0; s < KH / 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(p[2 * s], ireg[s], acc, 0, 0, 0);
        }
        float* xw = xch + xb * (4 * 16 * 64);
#pragma unroll
        for (int r = 0; r < 16; ++r) xw[(wave * 16 + r) * 64 + lane] = acc[r];
        // the exchange buffers alternate: a wave can run at most one barrier ahead of another
        __syncthreads();
        if (GRAD || wave == 0) {
            f32x16 T;
            float asum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s1 = xw[(0 * 16 + r) * 64 + lane] + xw[(2 * 16 + r) * 64 + lane];
                const float s2 = xw[(1 * 16 + r) * 64 + lane] + xw[(3 * 16 + r) * 64 + lane];
                const float dd = s1 - s2;
                asum += fabsf(dd);
                T[r] = dd > 0.f ? 1.f : (dd < 0.f ? -1.f : 0.f);
            }
            if (wave == 0) lsum += (double)asum;
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < NK; ++k) {
                    const int dt = kh + 2 * k;
                    if (dt < CT) {
                        // gacc[k][c = dt*32 + frag_row][i] += sum_j F_map[c][j] T[j][i]
                        const float* p = pm + 4 * hsel * (C + 1) + dt * 32 + l31;
#pragma unroll
                        for (int r = 0; r < 16; ++r)
                            gacc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(p[((r & 3) + 8 * (r >> 2)) * (C + 1)], T[r], gacc[k],
                                                                           0, 0, 0);
                    }
                }
            }
        }
        xb ^= 1;
    };

    if constexpr (PF) {
        FaTileRegs<C> regs;
        float* const panel0 = smem;
        float* const panel1 = smem + 2 * PANEL;
        regs.load(f1b, f2b, N, cl, i0, tid);
        regs.store(panel1, cl, tid);
        regs.load(f1b, f2b, N, cl, 0, tid);
        __syncthreads();
        {
            const float* p = panel1 + map * PANEL + l31 * (C + 1) + kh * KH + hsel;
#pragma unroll
            for (int s = 0; s < KH / 2; ++s) ireg[s] = p[2 * s];
        }
        regs.store(panel0, cl, tid);
        __syncthreads();
        const int nt = (N + 31) >> 5;
        for (int t = 0; t < nt; ++t) {
            if (t + 1 < nt) regs.load(f1b, f2b, N, cl, (t + 1) * 32, tid);
            tile(((t & 1) ? panel1 : panel0) + map * PANEL);
            // the other panel was last read for tile t - 1, ahead of the barrier that ended that iteration
            if (t + 1 < nt) regs.store((t & 1) ? panel0 : panel1, cl, tid);
            __syncthreads();
        }
    } else {
        float* J1 = smem;
        float* J2 = smem + JR * (C + 1);
        const float* fm = map ? f2b : f1b;
        const float* Jm = map ? J2 : J1;
        const int sc = cl ? 1 : N, sn = cl ? C : 1;
        {
            const int i = i0 + l31;
#pragma unroll
            for (int s = 0; s < KH / 2; ++s)
                ireg[s] = i < N ? fm[(size_t)(kh * KH + 2 * s + hsel) * sc + (size_t)i * sn] : 0.f;
        }
        for (int j0 = 0; j0 < N; j0 += JR) {
            const int nrows = (N - j0) < JR ? (N - j0) : JR;
            const int nt = (nrows + 31) >> 5;
            if (j0 > 0) __syncthreads();
            fa_stage<C>(J1, f1b, N, cl, j0, nt * 32, tid);
            fa_stage<C>(J2, f2b, N, cl, j0, nt * 32, tid);
            __syncthreads();
            for (int t = 0; t < nt; ++t) tile(Jm + t * PANEL);
        }
    }
    if (wave == 0) {
        const double tot = wave_sum_d(lsum);
        if (lane == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = tot;
    }
    if (GRAD) {
        float* gm = (map ? g2 : g1) + sample;
        const float sgn = map ? -1.f : 1.f;
        const int i = i0 + l31;
        if (i < N) {
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const int dt = kh + 2 * k;
                if (dt < CT) {
                    if (cl) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const f32x4 w4 = {sgn * gacc[k][4 * g], sgn * gacc[k][4 * g + 1], sgn * gacc[k][4 * g + 2],
                                              sgn * gacc[k][4 * g + 3]};
                            *reinterpret_cast<f32x4*>(gm + (size_t)i * C + dt * 32 + 8 * g + 4 * hsel) = w4;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) gm[(size_t)(dt * 32 + frag_row(r, hsel)) * N + i] = sgn * gacc[k][r];
                    }
                }
            }
        }
    }
}

// loss = scale * sum of the partials: each thread a strided, ordered share in double, then an ordered tree.
__global__ __launch_bounds__(256) void faloss_finalize_kernel(const double* __restrict__ partial, int n, double scale,
                                                             float* __restrict__ loss) {
    __shared__ double red[256];
    double a = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) a += partial[k];
    red[threadIdx.x] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * scale);
}

// d1 = u1 * (coef * g[0]),  d2 = u2 * (coef * g[0])   (u2 / d2 may be NULL); n % 4 == 0.
__global__ __launch_bounds__(256) void loss_scale_kernel(const float* __restrict__ u1, const float* __restrict__ u2,
                                                        const float* __restrict__ g, float* __restrict__ d1,
                                                        float* __restrict__ d2, long n4, double coef) {
    const float s = (float)(coef * (double)g[0]);
    const float* u = blockIdx.y ? u2 : u1;
    float* d = blockIdx.y ? d2 : d1;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < n4; e += (long)gridDim.x * 256) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(u + 4 * e);
        *reinterpret_cast<f32x4*>(d + 4 * e) = f32x4{v[0] * s, v[1] * s, v[2] * s, v[3] * s};
    }
}

int launch_scale(const char* what, const float* u1, const float* u2, const float* g, float* d1, float* d2, long n, double coef,
                 hipStream_t stream) {
    const long n4 = n / 4;
    long gx = (n4 + 255) / 256;
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(loss_scale_kernel, dim3((unsigned)gx, u2 ? 2 : 1), dim3(256), 0, stream, u1, u2, g, d1, d2, n4, coef);
    return tmf_launch_result(what);
}

int fa_tiles(int C, int N) {
    const int per_tile = 2 * 32 * (C + 1) * 4;
    if (C <= 128) return 2;                      // the two panels of the tile-by-tile form
    int tj = (160 * 1024 - FA_XCH * 4) / per_tile;
    if (tj > 8) tj = 8;
    const int need = (N + 31) / 32;
    return tj < need ? tj : need;
}

template <int C>
int fa_launch(const float* f1, const float* f2, double* partial, float* g1, float* g2, int B, int N, int cl, hipStream_t stream) {
    const int tj = fa_tiles(C, N);
    const size_t lds = (size_t)tj * 2 * 32 * (C + 1) * 4 + (size_t)FA_XCH * 4;
    const dim3 grid(tmf_cdiv(N, 32), B), block(256);
    int rc;
    if (g1) {
        if ((rc = tmf_allow_lds(faloss_kernel<C, true>, lds, "tmf_faloss_fwd")) != 0) return rc;
        hipLaunchKernelGGL((faloss_kernel<C, true>), grid, block, lds, stream, f1, f2, partial, g1, g2, N, cl, tj);
    } else {
        if ((rc = tmf_allow_lds(faloss_kernel<C, false>, lds, "tmf_faloss_fwd")) != 0) return rc;
        hipLaunchKernelGGL((faloss_kernel<C, false>), grid, block, lds, stream, f1, f2, partial, g1, g2, N, cl, tj);
    }
    return tmf_launch_result("tmf_faloss_fwd");
}

// ---------------------------------------------------------------------------------------------------------------------
// SupConLoss
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SC_R = 128;                        // most contrast rows (views * bs)
constexpr int SC_LS = SC_R + 1;                  // logits row stride
constexpr int SC_DC = 32;                        // feature columns per staged chunk
constexpr int SC_XS = SC_DC + 1;
constexpr size_t SC_LDS = SC_R * sizeof(double) + (size_t)(SC_R * SC_LS + SC_R * SC_XS) * sizeof(float);

// contrast row r = view * bs + sample  ->  features[sample][view][:]
__device__ __forceinline__ void sc_stage(float* X, const float* __restrict__ x, int bs, int views, int d, int d0, int tid) {
    const int R = bs * views;
#pragma unroll
    for (int u = 0; u < SC_R * SC_DC / 4 / 256; ++u) {
        const int e = u * 256 + tid;
        const int r = e / (SC_DC / 4), c = (e % (SC_DC / 4)) * 4;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        if (r < R && d0 + c < d) t = *reinterpret_cast<const f32x4*>(x + ((size_t)(r % bs) * views + r / bs) * d + d0 + c);
        float* p = X + r * SC_XS + c;
        p[0] = t[0]; p[1] = t[1]; p[2] = t[2]; p[3] = t[3];
    }
}

// labels != NULL: positives are equal labels; else mask != NULL: mask[bs][bs]; else the identity (SimCLR).
__device__ __forceinline__ float sc_base_mask(const long long* labels, const float* mask, int bs, int a, int c) {
    if (labels) return labels[a] == labels[c] ? 1.f : 0.f;
    if (mask) return mask[a * bs + c];
    return a == c ? 1.f : 0.f;
}

template <bool GRAD>
__global__ __launch_bounds__(256) void supcon_kernel(const float* __restrict__ x, const long long* __restrict__ labels,
                                                    const float* __restrict__ mask, float* __restrict__ loss,
                                                    float* __restrict__ gx, int bs, int views, int d, int A, float temperature,
                                                    float kappa) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_smem[];
    double* rowloss = reinterpret_cast<double*>(sc_smem);
    float* L = reinterpret_cast<float*>(sc_smem + SC_R * sizeof(double));
    float* X = L + SC_R * SC_LS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int R = bs * views;

    {   // logits: thread (ty, tx) owns rows ty + 16a, columns tx + 16b
        const int ty = tid >> 4, tx = tid & 15;
        float acc[8][8];
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[a][c] = 0.f;
        for (int d0 = 0; d0 < d; d0 += SC_DC) {
            if (d0 > 0) __syncthreads();
            sc_stage(X, x, bs, views, d, d0, tid);
            __syncthreads();
#pragma unroll 4
            for (int k = 0; k < SC_DC; ++k) {
                float xa[8], xc[8];
#pragma unroll
                for (int a = 0; a < 8; ++a) { xa[a] = X[(ty + 16 * a) * SC_XS + k]; xc[a] = X[(tx + 16 * a) * SC_XS + k]; }
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[a][c] = fmaf(xa[a], xc[c], acc[a][c]);
            }
        }
#pragma unroll
        for (int a = 0; a < 8; ++a)
#pragma unroll
            for (int c = 0; c < 8; ++c) L[(ty + 16 * a) * SC_LS + tx + 16 * c] = acc[a][c] / temperature;
    }
    __syncthreads();

    // one wave per anchor row; a lane holds columns lane and lane + 64
    for (int i = wave; i < (GRAD ? R : A); i += 4) {
        float* Li = L + i * SC_LS;
        if (i >= A) {                            // contrast_mode 'one': rows that are no anchors carry no dL/dlogits
            Li[lane] = 0.f; Li[lane + 64] = 0.f;
            continue;
        }
        float l[2], m[2], e[2];
        float mx = -INFINITY;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            l[h] = j < R ? Li[j] : -INFINITY;
            mx = fmaxf(mx, l[h]);
        }
        mx = wave_max(mx);                       // over all columns, the self column included (no gradient through it)
        double se = 0.0, sm = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = lane + 64 * h;
            const bool on = j < R && j != i;
            l[h] -= mx;
            e[h] = on ? expf(l[h]) : 0.f;
            m[h] = on ? sc_base_mask(labels, mask, bs, i % bs, j % bs) : 0.f;
            se += (double)e[h];
            sm += (double)m[h];
        }
        se = wave_sum_d(se);
        sm = wave_sum_d(sm);
        const float S = (float)se, M = (float)sm;
        const float logS = logf(S);
        double num = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if (lane + 64 * h < R) num += (double)(m[h] * (l[h] - logS));
        num = wave_sum_d(num);
        if (lane == 0) rowloss[i] = -(double)kappa * (double)((float)num / M);      // 0 / 0 = NaN: an anchor with no positive
        if (GRAD) {
            const float c = -kappa / (float)A;
            const float wsum = M / M;            // 1, or NaN with no positive
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = lane + 64 * h;
                Li[j] = j < R ? c * (m[h] / M - wsum * (e[h] / S)) : 0.f;
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int i = 0; i < A; ++i) a += rowloss[i];
        loss[0] = (float)(a / (double)A);
    }
    if (!GRAD) return;

    // Es = E + E^T in place: the pair (i, j), i < j, belongs to one thread
    for (int idx = tid; idx < SC_R * SC_R; idx += 256) {
        const int i = idx / SC_R, j = idx % SC_R;
        if (i < j) {
            const float s = L[i * SC_LS + j] + L[j * SC_LS + i];
            L[i * SC_LS + j] = s;
            L[j * SC_LS + i] = s;
        } else if (i == j) {
            L[i * SC_LS + i] *= 2.f;
        }
    }
    {   // G[r][:] = sum_k Es[r][k] X[k][:] / temperature; thread: column tid & 31 of the chunk, rows (tid >> 5) + 8a
        const int c = tid & 31, rg = tid >> 5;
        for (int d0 = 0; d0 < d; d0 += SC_DC) {
            __syncthreads();
            sc_stage(X, x, bs, views, d, d0, tid);
            __syncthreads();
            float g[16];
#pragma unroll
            for (int a = 0; a < 16; ++a) g[a] = 0.f;
            for (int k = 0; k < R; ++k) {
                const float xv = X[k * SC_XS + c];
#pragma unroll
                for (int a = 0; a < 16; ++a) g[a] = fmaf(L[(rg + 8 * a) * SC_LS + k], xv, g[a]);
            }
#pragma unroll
            for (int a = 0; a < 16; ++a) {
                const int r = rg + 8 * a;
                if (r < R && d0 + c < d) gx[((size_t)(r % bs) * views + r / bs) * d + d0 + c] = g[a] / temperature;
            }
        }
    }
}

}  // namespace

extern "C" int tmf_faloss_ok(int C, int N, int reduction) {
    return C >= 32 && C <= 256 && C % 32 == 0 && N >= 1 && (long)C * N < (1L << 31) && (reduction == 0 || reduction == 1);
}

extern "C" int tmf_faloss_partial_rows(int B, int N) { return B > 0 && N > 0 ? B * tmf_cdiv(N, 32) : 0; }

extern "C" size_t tmf_faloss_workspace_bytes(int B, int N) { return (size_t)tmf_faloss_partial_rows(B, N) * sizeof(double); }

extern "C" int tmf_faloss_fwd(const float* f1, const float* f2, float* loss, float* g1, float* g2, void* workspace,
                              size_t workspace_bytes, int B, int C, int N, int channels_last, int reduction, void* stream) {
    TMF_REQUIRE_PTR(f1); TMF_REQUIRE_PTR(f2); TMF_REQUIRE_PTR(loss); TMF_REQUIRE_PTR(workspace);
    TMF_REQUIRE(tmf_faloss_ok(C, N, reduction) && B >= 1 && B <= 65535, TMF_E_SHAPE,
                "tmf_faloss_fwd: B=%d C=%d N=%d reduction=%d (C a multiple of 32 up to 256, reduction 0 mean | 1 sum)", B, C, N,
                reduction);
    TMF_REQUIRE((g1 == nullptr) == (g2 == nullptr), TMF_E_NULL, "tmf_faloss_fwd: g1 and g2 go together");
    TMF_REQUIRE(workspace_bytes >= tmf_faloss_workspace_bytes(B, N), TMF_E_WORKSPACE, "tmf_faloss_fwd: workspace %zu < %zu",
                workspace_bytes, tmf_faloss_workspace_bytes(B, N));
    TMF_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, TMF_E_ALIGN, "tmf_faloss_fwd: workspace is not 8-byte aligned");
    if (channels_last) {
        TMF_REQUIRE_ALIGNED(f1); TMF_REQUIRE_ALIGNED(f2);
        if (g1) { TMF_REQUIRE_ALIGNED(g1); TMF_REQUIRE_ALIGNED(g2); }
    }
    hipStream_t s = (hipStream_t)stream;
    double* part = static_cast<double*>(workspace);
    int rc = 0;
    switch (C) {
        case 32:  rc = fa_launch<32>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 64:  rc = fa_launch<64>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 96:  rc = fa_launch<96>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 128: rc = fa_launch<128>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 160: rc = fa_launch<160>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 192: rc = fa_launch<192>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        case 224: rc = fa_launch<224>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
        default:  rc = fa_launch<256>(f1, f2, part, g1, g2, B, N, channels_last, s); break;
    }
    if (rc) return rc;
    const double scale = reduction == 0 ? 1.0 / ((double)B * (double)N * (double)N) : 1.0;
    hipLaunchKernelGGL(faloss_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)part, tmf_faloss_partial_rows(B, N), scale,
                       loss);
    return tmf_launch_result("tmf_faloss_fwd");
}

extern "C" int tmf_faloss_bwd(const float* g1, const float* g2, const float* grad_out, float* d1, float* d2, int B, int C, int N,
                              int reduction, void* stream) {
    TMF_REQUIRE_PTR(g1); TMF_REQUIRE_PTR(g2); TMF_REQUIRE_PTR(grad_out); TMF_REQUIRE_PTR(d1); TMF_REQUIRE_PTR(d2);
    TMF_REQUIRE(tmf_faloss_ok(C, N, reduction) && B >= 1, TMF_E_SHAPE, "tmf_faloss_bwd: B=%d C=%d N=%d reduction=%d", B, C, N,
                reduction);
    TMF_REQUIRE_ALIGNED(g1); TMF_REQUIRE_ALIGNED(g2); TMF_REQUIRE_ALIGNED(d1); TMF_REQUIRE_ALIGNED(d2);
    const double coef = reduction == 0 ? 2.0 / ((double)B * (double)N * (double)N) : 2.0;
    return launch_scale("tmf_faloss_bwd", g1, g2, grad_out, d1, d2, (long)B * C * N, coef, (hipStream_t)stream);
}

extern "C" int tmf_supcon_ok(int bs, int views, int d) {
    return bs >= 1 && views >= 1 && (long)bs * views <= SC_R && d >= 4 && d % 4 == 0;
}

extern "C" int tmf_supcon_fwd(const float* features, const long long* labels, const float* mask, float* loss, float* gfeat,
                              int bs, int views, int d, int anchors_all, float temperature, float base_temperature,
                              void* stream) {
    TMF_REQUIRE_PTR(features); TMF_REQUIRE_PTR(loss);
    TMF_REQUIRE(tmf_supcon_ok(bs, views, d), TMF_E_SHAPE, "tmf_supcon_fwd: bs=%d views=%d d=%d (bs*views <= 128, d %% 4 == 0)", bs,
                views, d);
    TMF_REQUIRE(!(labels && mask), TMF_E_ARG, "tmf_supcon_fwd: labels and mask are exclusive");
    TMF_REQUIRE_ALIGNED(features);
    const int A = anchors_all ? bs * views : bs;
    const float kappa = temperature / base_temperature;
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (gfeat) {
        if ((rc = tmf_allow_lds(supcon_kernel<true>, SC_LDS, "tmf_supcon_fwd")) != 0) return rc;
        hipLaunchKernelGGL(supcon_kernel<true>, dim3(1), dim3(256), SC_LDS, s, features, labels, mask, loss, gfeat, bs, views, d, A,
                           temperature, kappa);
    } else {
        if ((rc = tmf_allow_lds(supcon_kernel<false>, SC_LDS, "tmf_supcon_fwd")) != 0) return rc;
        hipLaunchKernelGGL(supcon_kernel<false>, dim3(1), dim3(256), SC_LDS, s, features, labels, mask, loss, gfeat, bs, views, d, A,
                           temperature, kappa);
    }
    return tmf_launch_result("tmf_supcon_fwd");
}

extern "C" int tmf_supcon_bwd(const float* gfeat, const float* grad_out, float* dfeat, int bs, int views, int d, void* stream) {
    TMF_REQUIRE_PTR(gfeat); TMF_REQUIRE_PTR(grad_out); TMF_REQUIRE_PTR(dfeat);
    TMF_REQUIRE(tmf_supcon_ok(bs, views, d), TMF_E_SHAPE, "tmf_supcon_bwd: bs=%d views=%d d=%d", bs, views, d);
    TMF_REQUIRE_ALIGNED(gfeat); TMF_REQUIRE_ALIGNED(dfeat);
    return launch_scale("tmf_supcon_bwd", gfeat, nullptr, grad_out, dfeat, nullptr, (long)bs * views * d, 1.0, (hipStream_t)stream);
}
