// shap.hip — atlas-region Shapley values by KernelSHAP in the paired-sampling form (include/tmf_hip.h states the semantics): the
// coalition sampler (tmf_shap_size_table on the host, tmf_shap_coalitions), the batch writer (tmf_shap_apply: K perturbed copies
// in ONE launch, a pure select), the normal equations (tmf_shap_gram: an exact int32 Gram matrix and ascending fp64 right-hand
// sides) and the constrained fit (tmf_shap_solve: blocked right-looking Cholesky in fp64 on a global-memory workspace, a fixed
// sequence of launches).  gfx950.  Compiled with -ffp-contract=off: the size table and the right-hand sides are chains of
// separately rounded fp64 operations; the solve asks for its fused multiply-adds by name.
//
// Coalitions: a workgroup owns pairs k, k + gridDim.x, ...; the P keys of a pair sit in LDS, a lane owns players tid, tid + 256,
// ... and counts its rank with broadcast LDS reads, wave ballots pack the words.
// Apply: a workgroup owns a tile of voxels and a run of one sample's jobs of the chunk; vol, labels and base are read into
// registers once per SHAP_ROWS jobs, whose rows are staged in LDS, and one tile is written per job.  Where the tiles alone
// would not fill the chip, up to SHAP_JOB_SPLIT workgroups (blockIdx.y) share the jobs of a tile.
// Gram: one workgroup per 32 x 32 tile of A; blocks of 32 coalitions are transposed in LDS (T_i: bit m of player i), then
// A[i][j] += popcount(T_i & T_j).  Integers only.  The right-hand sides: one lane per (b, i), ascending m, fed from LDS.
// Solve: panels of SHAP_NB = 32 columns.  Per panel two launches: (1) every workgroup factors the diagonal block in LDS from
// the working matrix M, workgroup 0 writes it to L, the others solve 256 rows of the panel each; (2) the trailing tiles of M
// take their rank-32 update from L.  M's diagonal block is not written while (1) reads it: L is a matrix of its own.
#include "tmf_device.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SHAP_THREADS = 256;
constexpr int SHAP_MAX_P = TMF_SHAP_MAX_PLAYERS;
constexpr int SHAP_MAX_WD = SHAP_MAX_P / 32;
constexpr int SHAP_COAL_GRID = 4096;        // workgroups of a coalition launch at most; they stride beyond that
constexpr int SHAP_ROWS = 8;                // coalition rows staged in LDS at a time by the apply kernel (1 KB at Wd = 32)
constexpr int SHAP_JOB_SPLIT = 8;           // workgroups that share one sample's jobs of a tile, at most
constexpr long SHAP_APPLY_FILL = 4096;      // workgroups an apply launch aims at: 16 per compute unit, so that none idles at the end
constexpr int SHAP_RHS_M = 256;             // coalitions whose scores and words a right-hand-side workgroup stages at a time
constexpr long SHAP_MAX_BLOCKS = 1 << 16;   // the limit of K and B
constexpr long SHAP_APPLY_GRID = 1 << 20;   // workgroups of an apply launch at most; they stride over the tiles beyond that
constexpr int SHAP_NB = 32;                 // panel width of the Cholesky factorisation
constexpr int SHAP_MBLK = 4;                // blocks of 32 coalitions a gram workgroup transposes at a time

// ---- coalitions ----

// rows m0 .. m0+N-1 of the header's sampler; unit k is a pair (paired) or one row
__global__ __launch_bounds__(SHAP_THREADS) void shap_coalitions_kernel(unsigned* __restrict__ coal, const unsigned* __restrict__ thr,
                                                                       int P, int Wd, int paired, unsigned k0, unsigned k1, int m0,
                                                                       int N, int kfirst, int nk) {
    __shared__ unsigned keys[SHAP_MAX_P];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    for (int ku = blockIdx.x; ku < nk; ku += gridDim.x) {
        const int k = kfirst + ku;
        unsigned r[4];
        philox4x32_10(0u, (unsigned)k, 1u, 0u, k0, k1, r);
        const unsigned u = r[0];
        int lo = 0, hi = P - 2;                         // the number of thr[t] <= u: thr ascends
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (thr[mid] <= u) lo = mid + 1; else hi = mid;
        }
        const int s = 1 + lo;
        __syncthreads();                                // the previous unit's keys have been read
        for (int q = tid; q < (P + 3) >> 2; q += SHAP_THREADS) {
            philox4x32_10((unsigned)q, (unsigned)k, 0u, 0u, k0, k1, r);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < P) keys[4 * q + j] = r[j];
        }
        __syncthreads();
        const int ma = paired ? 2 * k : k, mb = ma + 1;
        const bool wa = ma >= m0 && ma < m0 + N, wb = paired && mb >= m0 && mb < m0 + N;
        for (int i0 = 0; i0 < P; i0 += SHAP_THREADS) {
            const int i = i0 + tid;
            bool in = false;
            if (i < P) {
                const unsigned mine = keys[i];
                int rank = 0;
                for (int j = 0; j < P; ++j) {
                    const unsigned kj = keys[j];
                    rank += (kj < mine || (kj == mine && j < i)) ? 1 : 0;
                }
                in = rank < s;
            }
            const unsigned long long za = __ballot(in), zb = __ballot(i < P && !in);
            const int word = (i0 >> 5) + 2 * wave;
            if (lane < 2 && word + lane < Wd) {
                if (wa) coal[(size_t)(ma - m0) * Wd + word + lane] = (unsigned)(za >> (32 * lane));
                if (wb) coal[(size_t)(mb - m0) * Wd + word + lane] = (unsigned)(zb >> (32 * lane));
            }
        }
    }
}

// ---- apply ----

// whether a voxel of player sel (-1: none) keeps its value under the row
__device__ __forceinline__ bool shap_keeps(const unsigned* row, int sel) {
    return sel < 0 || ((row[(sel < 0 ? 0 : sel) >> 5] >> (sel & 31)) & 1u) != 0;
}

// out[k][v] = vol[b][v] where the voxel's player is in the row of job j0 + k = b*N + m (or the voxel has no player), else f.
// Workgroup blockIdx.x = s * tg + t: sample b0 + s of the chunk, tiles t, t + tg, ...
template <int VEC>
__global__ __launch_bounds__(SHAP_THREADS) void shap_apply_kernel(const float* __restrict__ vol, const int* __restrict__ labels,
                                                                  const unsigned* __restrict__ coal, const float* __restrict__ fill,
                                                                  const float* __restrict__ base, float* __restrict__ out, int V,
                                                                  int R, int p0, int Wd, int N, int j0, int K, int tg, int ntiles) {
    __shared__ unsigned rows[SHAP_ROWS * SHAP_MAX_WD];
    constexpr int TILE = SHAP_THREADS * VEC;
    const int s = blockIdx.x / tg, t0 = blockIdx.x - s * tg;
    const int b = j0 / N + s;
    const long jb = (long)b * N;                                        // the sample's first job
    const int ka = jb > j0 ? (int)(jb - j0) : 0, ke = jb + N - j0 < K ? (int)(jb + N - j0) : K;      // its jobs of the chunk: k in [ka, ke)
    const float f0 = base ? 0.f : fill[b];
    const float* src = vol + (size_t)b * V;
    const float* bs = base ? base + (size_t)b * V : nullptr;
    const int pa = ka + (int)((long)(ke - ka) * blockIdx.y / gridDim.y);               // this workgroup's share of them: [pa, pe)
    const int pe = ka + (int)((long)(ke - ka) * (blockIdx.y + 1) / gridDim.y);
    for (int kb = pa; kb < pe; kb += SHAP_ROWS) {
        const int cnt = min(SHAP_ROWS, pe - kb);
        __syncthreads();                                                // the previous rows have been read
        const unsigned* rsrc = coal + (size_t)(j0 + kb - jb) * Wd;
        for (int o = threadIdx.x; o < cnt * Wd; o += SHAP_THREADS) rows[o] = rsrc[o];
        __syncthreads();
        for (int tile = t0; tile < ntiles; tile += tg) {
            const long e = (long)tile * TILE + (long)threadIdx.x * VEC;
            if (e >= V) continue;                                       // VEC == 4: V % 4 == 0, the four voxels exist
            if constexpr (VEC == 4) {
                const f32x4 v = TmfIO<float, 4>::ld(src + e);
                const i32x4 l = *reinterpret_cast<const i32x4*>(labels + e);
                f32x4 f = {f0, f0, f0, f0};
                if (bs) f = TmfIO<float, 4>::ld(bs + e);
                i32x4 sel;                                              // the voxel's player, -1: never replaced
#pragma unroll
                for (int q = 0; q < 4; ++q) sel[q] = (l[q] <= 0 || l[q] > R) ? -1 : p0 + l[q] - 1;
                for (int r = 0; r < cnt; ++r) {
                    const unsigned* row = rows + r * Wd;
                    f32x4 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) o[q] = shap_keeps(row, sel[q]) ? v[q] : f[q];
                    TmfIO<float, 4>::st(out + (size_t)(kb + r) * V + e, o);
                }
            } else {
                const int l = labels[e];
                const float v = src[e], f = bs ? bs[e] : f0;
                const int sel = (l <= 0 || l > R) ? -1 : p0 + l - 1;
                for (int r = 0; r < cnt; ++r) out[(size_t)(kb + r) * V + e] = shap_keeps(rows + r * Wd, sel) ? v : f;
            }
        }
    }
}

// ---- gram ----

// tile (blockIdx.y, blockIdx.x) of A: players 32*by .. +31 against 32*bx .. +31
__global__ __launch_bounds__(SHAP_THREADS) void shap_gram_kernel(const unsigned* __restrict__ coal, int* __restrict__ A, int P, int Wd,
                                                                 int N) {
    __shared__ unsigned raw[SHAP_MBLK][2][32];      // [block of 32 coalitions][side][coalition]: the side's word of that row
    __shared__ unsigned T[SHAP_MBLK][2][32];        // [..][side][player of the word]: bit m' = the player is in coalition m'
    const int tid = threadIdx.x;
    const int wi = blockIdx.y, wj = blockIdx.x;
    const int blk = tid >> 6, side = (tid >> 5) & 1, x = tid & 31;
    const int i = tid >> 3, jq = (tid & 7) * 4;     // the lane's outputs: (i, jq .. jq+3)
    int acc[4] = {0, 0, 0, 0};
    for (int mb = 0; mb < N; mb += 32 * SHAP_MBLK) {
        const int m = mb + 32 * blk + x;
        __syncthreads();                            // the previous T has been read
        raw[blk][side][x] = m < N ? coal[(size_t)m * Wd + (side ? wj : wi)] : 0u;
        __syncthreads();
        unsigned t = 0;
#pragma unroll
        for (int mm = 0; mm < 32; ++mm) t |= ((raw[blk][side][mm] >> x) & 1u) << mm;
        T[blk][side][x] = t;
        __syncthreads();
#pragma unroll
        for (int g = 0; g < SHAP_MBLK; ++g) {
            const unsigned ti = T[g][0][i];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] += __popc(ti & T[g][1][jq + q]);
        }
    }
    const int gi = 32 * wi + i;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int gj = 32 * wj + jq + q;
        if (gi < P && gj < P) A[(size_t)gi * P + gj] = acc[q];
    }
}

// rhs[b][i] = sum over the m with z_mi = 1, ascending, of (double)scores[b][m] - (double)offset[b]; one lane per (b, i).
// Workgroup (b, blockIdx.y): players 256 * blockIdx.y .. + 255, that is 8 words of a row; SHAP_RHS_M coalitions at a time their
// y and those words go to LDS, the chain then reads LDS alone.
__global__ __launch_bounds__(SHAP_THREADS) void shap_rhs_kernel(const unsigned* __restrict__ coal, const float* __restrict__ scores,
                                                                const float* __restrict__ offset, double* __restrict__ rhs, int P,
                                                                int Wd, int N) {
    __shared__ double ys[SHAP_RHS_M];
    __shared__ unsigned zw[SHAP_RHS_M][8];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int i = blockIdx.y * SHAP_THREADS + tid;
    const int w0 = blockIdx.y * 8, nw = min(8, Wd - w0);
    const double off = (double)offset[b];
    const float* sc = scores + (size_t)b * N;
    const int wl = (tid >> 5), bit = tid & 31;
    double acc = 0.0;
    for (int m0 = 0; m0 < N; m0 += SHAP_RHS_M) {
        const int cnt = min(SHAP_RHS_M, N - m0);
        __syncthreads();                            // the previous block has been read
        if (tid < cnt) ys[tid] = (double)sc[m0 + tid] - off;
        for (int o = tid; o < cnt * nw; o += SHAP_THREADS) {
            const int mm = o / nw, w = o - mm * nw;
            zw[mm][w] = coal[(size_t)(m0 + mm) * Wd + w0 + w];
        }
        __syncthreads();
        if (i < P)
            for (int mm = 0; mm < cnt; ++mm) acc = ((zw[mm][wl] >> bit) & 1u) ? acc + ys[mm] : acc;
    }
    if (i < P) rhs[(size_t)b * P + i] = acc;
}

// ---- solve ----

// M = A + ridge I on Pp x Pp (the identity on the padding), X = [rhs_1 .. rhs_B, 1] with zeros on the padding, info = 0
__global__ __launch_bounds__(SHAP_THREADS) void shap_init_kernel(const int* __restrict__ A, const double* __restrict__ rhs,
                                                                 double ridge, double* __restrict__ M, double* __restrict__ X,
                                                                 int* __restrict__ info, int B, int P, int Pp) {
    const long nM = (long)Pp * Pp, nX = (long)(B + 1) * Pp;
    const long step = (long)gridDim.x * SHAP_THREADS;
    for (long it = (long)blockIdx.x * SHAP_THREADS + threadIdx.x; it < nM + nX; it += step) {
        if (it < nM) {
            const int i = (int)(it / Pp), j = (int)(it - (long)i * Pp);
            double v = i == j ? 1.0 : 0.0;
            if (i < P && j < P) v = (double)A[(size_t)i * P + j] + (i == j ? ridge : 0.0);
            M[it] = v;
        } else {
            const long o = it - nM;
            const int b = (int)(o / Pp), i = (int)(o - (long)b * Pp);
            X[o] = i >= P ? 0.0 : b < B ? rhs[(size_t)b * P + i] : 1.0;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = 0;
}

// Panel kb.  Every workgroup: the Cholesky factor of M's diagonal block in LDS (lower triangle).  Workgroup 0: writes it to L
// and the first failed pivot to info.  Workgroup g >= 1: rows (kb+1)*32 + (g-1)*256 + tid of the panel, X L11^T = A21.
__global__ __launch_bounds__(SHAP_THREADS) void shap_panel_kernel(const double* __restrict__ M, double* __restrict__ L,
                                                                  int* __restrict__ info, int P, int Pp, int kb) {
    __shared__ double a[SHAP_NB][SHAP_NB + 1];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const int c0 = kb * SHAP_NB;
    for (int o = tid; o < SHAP_NB * SHAP_NB; o += SHAP_THREADS) {
        const int i = o >> 5, j = o & 31;
        a[i][j] = M[(size_t)(c0 + i) * Pp + c0 + j];
    }
    if (tid == 0) bad = 0;
    __syncthreads();
    for (int k = 0; k < SHAP_NB; ++k) {
        const double piv = a[k][k];
        __syncthreads();
        if (tid == 0) {
            if (!(piv > 0.0) && bad == 0) bad = c0 + k + 1;
            a[k][k] = sqrt(piv);
        }
        __syncthreads();
        const double d = a[k][k];
        if (tid > k && tid < SHAP_NB) a[tid][k] = a[tid][k] / d;
        __syncthreads();
        const int i = tid & 31;
        if (i > k) {
            const double lik = a[i][k];
            for (int j = k + 1 + (tid >> 5); j <= i; j += 8) a[i][j] = __builtin_fma(-lik, a[j][k], a[i][j]);
        }
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        for (int o = tid; o < SHAP_NB * SHAP_NB; o += SHAP_THREADS) {
            const int i = o >> 5, j = o & 31;
            L[(size_t)(c0 + i) * Pp + c0 + j] = j <= i ? a[i][j] : 0.0;
        }
        if (tid == 0 && bad != 0 && bad <= P && info[0] == 0) info[0] = bad;
        return;
    }
    const int row = c0 + SHAP_NB + (blockIdx.x - 1) * SHAP_THREADS + tid;
    if (row >= Pp) return;
    double x[SHAP_NB];
    const double* src = M + (size_t)row * Pp + c0;
#pragma unroll
    for (int j = 0; j < SHAP_NB; ++j) x[j] = src[j];
#pragma unroll
    for (int j = 0; j < SHAP_NB; ++j) {
        double v = x[j];
#pragma unroll
        for (int t = 0; t < j; ++t) v = __builtin_fma(-x[t], a[j][t], v);
        x[j] = v / a[j][j];
    }
    double* dst = L + (size_t)row * Pp + c0;
#pragma unroll
    for (int j = 0; j < SHAP_NB; ++j) dst[j] = x[j];
}

// M[ti][tj] -= L[ti][kb] L[tj][kb]^T for the tiles kb < tj <= ti
__global__ __launch_bounds__(SHAP_THREADS) void shap_update_kernel(double* __restrict__ M, const double* __restrict__ L, int Pp,
                                                                   int kb) {
    const int ti = kb + 1 + blockIdx.y, tj = kb + 1 + blockIdx.x;
    if (tj > ti) return;
    __shared__ double li[SHAP_NB][SHAP_NB + 1], lj[SHAP_NB][SHAP_NB + 1];
    const int tid = threadIdx.x;
    for (int o = tid; o < SHAP_NB * SHAP_NB; o += SHAP_THREADS) {
        const int i = o >> 5, j = o & 31;
        li[i][j] = L[(size_t)(ti * SHAP_NB + i) * Pp + kb * SHAP_NB + j];
        lj[i][j] = L[(size_t)(tj * SHAP_NB + i) * Pp + kb * SHAP_NB + j];
    }
    __syncthreads();
    const int i = tid >> 3, jq = (tid & 7) * 4;
    double* dst = M + (size_t)(ti * SHAP_NB + i) * Pp + tj * SHAP_NB + jq;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        double acc = dst[q];
#pragma unroll
        for (int t = 0; t < SHAP_NB; ++t) acc = __builtin_fma(-li[i][t], lj[jq + q][t], acc);
        dst[q] = acc;
    }
}

// L y = r, then L^T x = y, in place on row blockIdx.x of X, 32 unknowns at a time: the first wave solves the diagonal block
// (a lane per unknown, the solved one broadcast by a shuffle), then every lane takes the block out of the rows still open.
__global__ __launch_bounds__(SHAP_THREADS) void shap_tri_kernel(const double* __restrict__ L, double* __restrict__ X, int Pp) {
    __shared__ double r[SHAP_MAX_P];
    const int tid = threadIdx.x, nb = Pp / SHAP_NB;
    double* xr = X + (size_t)blockIdx.x * Pp;
    for (int i = tid; i < Pp; i += SHAP_THREADS) r[i] = xr[i];
    __syncthreads();
    for (int kb = 0; kb < nb; ++kb) {
        const int c0 = kb * SHAP_NB;
        if (tid < 64) {
            const int t = tid & 31;
            double lr[SHAP_NB];                                         // the lane's row of the diagonal block
#pragma unroll
            for (int j = 0; j < SHAP_NB; ++j) lr[j] = L[(size_t)(c0 + t) * Pp + c0 + j];
            double v = r[c0 + t];
#pragma unroll
            for (int j = 0; j < SHAP_NB; ++j) {
                const double xj = __shfl(v / lr[j], j);                 // lane j holds the finished numerator of unknown j
                if (t == j) v = xj;
                else if (t > j) v = __builtin_fma(-lr[j], xj, v);
            }
            if (tid < SHAP_NB) r[c0 + t] = v;
        }
        __syncthreads();
        for (int i = c0 + SHAP_NB + tid; i < Pp; i += SHAP_THREADS) {
            const double* lrow = L + (size_t)i * Pp + c0;
            double v = r[i];
#pragma unroll
            for (int j = 0; j < SHAP_NB; ++j) v = __builtin_fma(-lrow[j], r[c0 + j], v);
            r[i] = v;
        }
        __syncthreads();
    }
    for (int kb = nb - 1; kb >= 0; --kb) {
        const int c0 = kb * SHAP_NB;
        if (tid < 64) {
            const int t = tid & 31;
            double lc[SHAP_NB];                                         // the lane's column of the diagonal block
#pragma unroll
            for (int j = 0; j < SHAP_NB; ++j) lc[j] = L[(size_t)(c0 + j) * Pp + c0 + t];
            double v = r[c0 + t];
#pragma unroll
            for (int j = SHAP_NB - 1; j >= 0; --j) {
                const double d = __shfl(lc[j], j);                      // L[j][j]
                const double xj = __shfl(v / d, j);
                if (t == j) v = xj;
                else if (t < j) v = __builtin_fma(-lc[j], xj, v);
            }
            if (tid < SHAP_NB) r[c0 + t] = v;
        }
        __syncthreads();
        for (int i = tid; i < c0; i += SHAP_THREADS) {
            double v = r[i];
#pragma unroll
            for (int j = 0; j < SHAP_NB; ++j) v = __builtin_fma(-L[(size_t)(c0 + j) * Pp + i], r[c0 + j], v);
            r[i] = v;
        }
        __syncthreads();
    }
    for (int i = tid; i < Pp; i += SHAP_THREADS) xr[i] = r[i];
}

// the sum of x[0 .. P-1] in a fixed order: strided partial sums, then a tree in LDS; every lane of the workgroup gets it
__device__ __forceinline__ double shap_sum(const double* __restrict__ x, int P, double* lds) {
    double s = 0.0;
    for (int i = threadIdx.x; i < P; i += SHAP_THREADS) s = s + x[i];
    __syncthreads();
    lds[threadIdx.x] = s;
    __syncthreads();
    for (int w = SHAP_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) lds[threadIdx.x] = lds[threadIdx.x] + lds[threadIdx.x + w];
        __syncthreads();
    }
    return lds[0];
}

// phi_b = x_b - x_1 (sum x_b - delta_b) / sum x_1, NaN where the factorisation failed
__global__ __launch_bounds__(SHAP_THREADS) void shap_finish_kernel(const double* __restrict__ X, const double* __restrict__ delta,
                                                                   const int* __restrict__ info, double* __restrict__ phi, int B,
                                                                   int P, int Pp) {
    __shared__ double lds[SHAP_THREADS];
    const int b = blockIdx.x;
    const double* xb = X + (size_t)b * Pp;
    const double* x1 = X + (size_t)B * Pp;
    const double sb = shap_sum(xb, P, lds), s1 = shap_sum(x1, P, lds);
    const double t = (sb - delta[b]) / s1;
    const bool ok = info[0] == 0;
    for (int i = threadIdx.x; i < P; i += SHAP_THREADS)
        phi[(size_t)b * P + i] = ok ? __builtin_fma(-x1[i], t, xb[i]) : __builtin_nan("");
}

// ---- host side ----

bool shap_a4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool shap_a8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
bool shap_a16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int shap_players(const char* fn, int P) {
    TMF_REQUIRE(P >= 2 && P <= SHAP_MAX_P, TMF_E_SHAPE, "%s: P = %d players (2 .. %d)", fn, P, SHAP_MAX_P);
    return TMF_OK;
}

int shap_batch(const char* fn, int B, int N) {
    TMF_REQUIRE(B >= 1 && B <= SHAP_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", fn, B, SHAP_MAX_BLOCKS);
    TMF_REQUIRE(N >= 1, TMF_E_ARG, "%s: N = %d coalitions", fn, N);
    TMF_REQUIRE((long long)B * N <= INT_MAX, TMF_E_SHAPE, "%s: B * N = %d * %d does not stay below 2^31", fn, B, N);
    return TMF_OK;
}

int shap_pp(int P) { return (P + SHAP_NB - 1) / SHAP_NB * SHAP_NB; }

}  // namespace

extern "C" int tmf_shap_size_table(int P, unsigned* thr) {
    TMF_TRY(shap_players(__func__, P));
    if (P == 2) return TMF_OK;
    TMF_REQUIRE_PTR(thr);
    double total = 0.0;
    for (int r = 1; r <= P - 1; ++r) total = total + 1.0 / ((double)r * (double)(P - r));
    double part = 0.0;
    for (int t = 0; t <= P - 3; ++t) {
        const int r = t + 1;
        part = part + 1.0 / ((double)r * (double)(P - r));
        const double v = floor(4294967296.0 * (part / total));
        thr[t] = v >= 4294967295.0 ? 4294967295u : (unsigned)v;
    }
    return TMF_OK;
}

extern "C" int tmf_shap_coalitions(unsigned* coal, const unsigned* thr, int P, int paired, unsigned long long seed, int m0, int N,
                                   void* stream) {
    TMF_REQUIRE_PTR(coal);
    TMF_TRY(shap_players(__func__, P));
    TMF_REQUIRE(thr != nullptr || P == 2, TMF_E_NULL, "%s: argument 'thr' is NULL", __func__);
    TMF_REQUIRE(paired == 0 || paired == 1, TMF_E_ARG, "%s: paired = %d", __func__, paired);
    TMF_REQUIRE(N >= 1 && m0 >= 0 && (long long)m0 + N <= INT_MAX, TMF_E_ARG, "%s: coalitions m0 = %d, N = %d", __func__, m0, N);
    TMF_REQUIRE(shap_a4(coal) && shap_a4(thr), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    const int kfirst = paired ? m0 >> 1 : m0;
    const int klast = paired ? (int)(((long long)m0 + N - 1) >> 1) : m0 + N - 1;
    const int nk = klast - kfirst + 1;
    hipLaunchKernelGGL(shap_coalitions_kernel, dim3((unsigned)(nk < SHAP_COAL_GRID ? nk : SHAP_COAL_GRID)), dim3(SHAP_THREADS), 0,
                       (hipStream_t)stream, coal, thr, P, (P + 31) / 32, paired, (unsigned)seed ^ 0x53484150u,
                       (unsigned)(seed >> 32) ^ 0x636F616Cu, m0, N, kfirst, nk);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_shap_apply(const float* vol, const int* labels, const unsigned* coal, const float* fill, const float* base,
                              float* out, int B, int D, int H, int W, int R, int p0, int P, int N, int j0, int K, void* stream) {
    TMF_REQUIRE_PTR(vol); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(coal); TMF_REQUIRE_PTR(out);
    TMF_REQUIRE(fill != nullptr || base != nullptr, TMF_E_NULL, "%s: fill and base are both NULL", __func__);
    TMF_REQUIRE(D >= 1 && H >= 1 && W >= 1, TMF_E_SHAPE, "%s: volume %d x %d x %d", __func__, D, H, W);
    const long long dh = (long long)D * H;
    TMF_REQUIRE(dh <= INT_MAX / W, TMF_E_SHAPE, "%s: D*H*W = %d*%d*%d does not stay below 2^31", __func__, D, H, W);
    const int V = (int)(dh * W);
    TMF_TRY(shap_players(__func__, P));
    TMF_TRY(shap_batch(__func__, B, N));
    TMF_REQUIRE(R >= 1 && p0 >= 0 && (long long)p0 + R <= P, TMF_E_ARG, "%s: players p0 = %d, R = %d of %d", __func__, p0, R, P);
    TMF_REQUIRE(K >= 1 && K <= SHAP_MAX_BLOCKS && j0 >= 0, TMF_E_ARG, "%s: jobs j0 = %d, K = %d (K at most %ld)", __func__, j0, K,
                SHAP_MAX_BLOCKS);
    TMF_REQUIRE((long long)j0 + K <= (long long)B * N, TMF_E_ARG, "%s: jobs %d .. %lld of %lld", __func__, j0,
                (long long)j0 + K - 1, (long long)B * N);
    TMF_REQUIRE(shap_a4(vol) && shap_a4(labels) && shap_a4(coal) && shap_a4(fill) && shap_a4(base) && shap_a4(out), TMF_E_ALIGN,
                "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE(out + (size_t)K * V <= vol || vol + (size_t)B * V <= out, TMF_E_ARG, "%s: out overlaps vol", __func__);
    const bool vec = V % 4 == 0 && shap_a16(vol) && shap_a16(out) && shap_a16(labels) && shap_a16(base);
    const int tile = SHAP_THREADS * (vec ? 4 : 1);
    const int ntiles = (int)(((long)V + tile - 1) / tile);
    const int ns = (j0 + K - 1) / N - j0 / N + 1;              // samples the chunk touches: <= K
    long tg = SHAP_APPLY_GRID / ns;
    tg = tg < 1 ? 1 : tg > ntiles ? ntiles : tg;
    long js = (SHAP_APPLY_FILL + tg * ns - 1) / (tg * ns);
    js = js > SHAP_JOB_SPLIT ? SHAP_JOB_SPLIT : js > K ? K : js;
    const dim3 grid((unsigned)(tg * ns), (unsigned)js);
    const int Wd = (P + 31) / 32;
    if (vec)
        hipLaunchKernelGGL(shap_apply_kernel<4>, grid, dim3(SHAP_THREADS), 0, (hipStream_t)stream, vol, labels, coal, fill, base, out,
                           V, R, p0, Wd, N, j0, K, (int)tg, ntiles);
    else
        hipLaunchKernelGGL(shap_apply_kernel<1>, grid, dim3(SHAP_THREADS), 0, (hipStream_t)stream, vol, labels, coal, fill, base, out,
                           V, R, p0, Wd, N, j0, K, (int)tg, ntiles);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_shap_gram(const unsigned* coal, const float* scores, const float* offset, int* A, double* rhs, int B, int P, int N,
                             void* stream) {
    TMF_REQUIRE_PTR(coal); TMF_REQUIRE_PTR(scores); TMF_REQUIRE_PTR(offset); TMF_REQUIRE_PTR(A); TMF_REQUIRE_PTR(rhs);
    TMF_TRY(shap_players(__func__, P));
    TMF_TRY(shap_batch(__func__, B, N));
    TMF_REQUIRE(shap_a4(coal) && shap_a4(scores) && shap_a4(offset) && shap_a4(A), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned",
                __func__);
    TMF_REQUIRE(shap_a8(rhs), TMF_E_ALIGN, "%s: rhs is not 8-byte aligned", __func__);
    const int Wd = (P + 31) / 32;
    hipLaunchKernelGGL(shap_gram_kernel, dim3((unsigned)Wd, (unsigned)Wd), dim3(SHAP_THREADS), 0, (hipStream_t)stream, coal, A, P, Wd,
                       N);
    TMF_TRY(tmf_launch_result(__func__));
    hipLaunchKernelGGL(shap_rhs_kernel, dim3((unsigned)B, (unsigned)tmf_cdiv(P, SHAP_THREADS)), dim3(SHAP_THREADS), 0,
                       (hipStream_t)stream, coal, scores, offset, rhs, P, Wd, N);
    return tmf_launch_result(__func__);
}

extern "C" size_t tmf_shap_solve_workspace(int B, int P) {
    if (B < 1 || B > SHAP_MAX_BLOCKS || P < 2 || P > SHAP_MAX_P) return 0;
    const size_t Pp = (size_t)shap_pp(P);
    return up256((2 * Pp * Pp + ((size_t)B + 1) * Pp) * sizeof(double));
}

extern "C" int tmf_shap_solve(const int* A, const double* rhs, const double* delta, double ridge, double* phi, int* info,
                              void* workspace, size_t workspace_bytes, int B, int P, void* stream) {
    TMF_REQUIRE_PTR(A); TMF_REQUIRE_PTR(rhs); TMF_REQUIRE_PTR(delta); TMF_REQUIRE_PTR(phi); TMF_REQUIRE_PTR(info);
    TMF_REQUIRE_PTR(workspace);
    TMF_TRY(shap_players(__func__, P));
    TMF_REQUIRE(B >= 1 && B <= SHAP_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", __func__, B, SHAP_MAX_BLOCKS);
    TMF_REQUIRE(isfinite(ridge) && ridge >= 0.0, TMF_E_ARG, "%s: ridge = %g", __func__, ridge);
    TMF_REQUIRE(shap_a4(A) && shap_a4(info), TMF_E_ALIGN, "%s: A or info is not 4-byte aligned", __func__);
    TMF_REQUIRE(shap_a8(rhs) && shap_a8(delta) && shap_a8(phi), TMF_E_ALIGN, "%s: rhs, delta or phi is not 8-byte aligned", __func__);
    TMF_REQUIRE(shap_a16(workspace), TMF_E_ALIGN, "%s: the workspace is not 16-byte aligned", __func__);
    TMF_REQUIRE(workspace_bytes >= tmf_shap_solve_workspace(B, P), TMF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", __func__,
                workspace_bytes, tmf_shap_solve_workspace(B, P));
    const int Pp = shap_pp(P), nb = Pp / SHAP_NB;
    hipStream_t s = (hipStream_t)stream;
    double* M = static_cast<double*>(workspace);
    double* L = M + (size_t)Pp * Pp;
    double* X = L + (size_t)Pp * Pp;
    const long items = (long)Pp * Pp + (long)(B + 1) * Pp;
    const long ib = (items + SHAP_THREADS - 1) / SHAP_THREADS;
    hipLaunchKernelGGL(shap_init_kernel, dim3((unsigned)(ib < 4096 ? ib : 4096)), dim3(SHAP_THREADS), 0, s, A, rhs, ridge, M, X, info,
                       B, P, Pp);
    for (int kb = 0; kb < nb; ++kb) {
        const int below = Pp - (kb + 1) * SHAP_NB;
        hipLaunchKernelGGL(shap_panel_kernel, dim3((unsigned)(1 + (below + SHAP_THREADS - 1) / SHAP_THREADS)), dim3(SHAP_THREADS), 0,
                           s, M, L, info, P, Pp, kb);
        if (kb + 1 < nb)
            hipLaunchKernelGGL(shap_update_kernel, dim3((unsigned)(nb - kb - 1), (unsigned)(nb - kb - 1)), dim3(SHAP_THREADS), 0, s,
                               M, L, Pp, kb);
    }
    hipLaunchKernelGGL(shap_tri_kernel, dim3((unsigned)(B + 1)), dim3(SHAP_THREADS), 0, s, L, X, Pp);
    hipLaunchKernelGGL(shap_finish_kernel, dim3((unsigned)B), dim3(SHAP_THREADS), 0, s, X, delta, info, phi, B, P, Pp);
    return tmf_launch_result(__func__);
}
