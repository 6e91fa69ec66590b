// criterion.hip — the tail of a train / eval step for gfx950, fp32: cross entropy, the adversarial criterion in one launch,
// the epoch metrics on a small device state, and the exact ROC AUC as an integer pair count.
//
// Cross entropy of one row x[0..C) with target y:  m = max x,  s = sum_c expf(x_c - m) (fp32, c ascending),
// l = logf(s) - (x_y - m),  p_c = expf(x_c - m) / s,  dl/dx_c = p_c - [c == y].  expf / logf are the accurate library
// functions.  A target of -100 (torch's default ignore_index) has weight 0; any other target outside [0, C) makes the loss
// NaN and its gradient row zero — no read leaves the row.  The rows are re-read from memory (a few hundred bytes, cached)
// rather than kept in a runtime-indexed register array, which would live in scratch.
//
// Every reduction here is one workgroup: a thread adds its samples i = tid, tid + 256, ... in that order in double (counts
// in integers), the 256 per-thread values meet in a fixed LDS tree.  No atomics, bitwise repeatable.  The metric states are
// read-add-written by one thread of one workgroup: launches on one stream serialize.
//
// Replaces kfold_train_adversarial.py:119-125 (criterion), :127-128 and :178-194 (the ignite metrics of every trainer and
// evaluator) and the scikit-learn call behind ignite's ROC_AUC.
#include "tmf_device.h"

namespace {

constexpr int CE_MAX_C = 16;
constexpr int CE_MAX_B = 4096;
constexpr long long CE_IGNORE = -100;
constexpr int AUC_MAX_N = 65536;
constexpr int AUC_IPT = 4;                       // i elements per thread
constexpr int AUC_IB = 256 * AUC_IPT;            // i elements per workgroup
constexpr int AUC_JB = 2048;                     // j elements per workgroup (LDS tile)

// fixed-order sum of one value per thread over the workgroup of 256; every thread gets the result.  red: 256 entries.
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* red) {
    const int tid = threadIdx.x;
    __syncthreads();                             // red may still be read from the previous use
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

struct RowStat { float m, s; };

__device__ __forceinline__ RowStat row_stat(const float* __restrict__ x, int C) {
    float m = x[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, x[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(x[c] - m);
    return RowStat{m, s};
}

// torch.argmax: the first maximal index, a NaN counting as larger than every number (the first NaN of a row that has one)
__device__ __forceinline__ int row_argmax(const float* __restrict__ x, int C) {
    int a = 0;
    float m = x[0];
    for (int c = 1; c < C; ++c)
        if (x[c] > m || (x[c] != x[c] && m == m)) { m = x[c]; a = c; }
    return a;
}

// target of sample i: the label array, or a constant (the domain heads)
__device__ __forceinline__ long long target_of(const long long* __restrict__ target, long long constant, int i) {
    return target ? target[i] : constant;
}

// sum_i w_i l_i and sum_i w_i over the B rows, w_i = weight[y_i] (1 without weights; 0 for the ignored target)
__device__ __forceinline__ void ce_sums(const float* __restrict__ x, const long long* __restrict__ target, long long constant,
                                        const float* __restrict__ weight, int B, int C, double* red, double& num, double& den) {
    double a = 0.0, w = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const long long y = target_of(target, constant, i);
        if (y == CE_IGNORE) continue;
        if (y < 0 || y >= C) { a = __builtin_nan(""); continue; }
        const float* xi = x + (size_t)i * C;
        const RowStat r = row_stat(xi, C);
        const float l = logf(r.s) - (xi[y] - r.m);
        const float wi = weight ? weight[y] : 1.f;
        a += (double)(wi * l);
        w += (double)wi;
    }
    num = block_sum(a, red);
    den = block_sum(w, red);
}

// g[i][c] = scale * w_i * (p_ic - [c == y_i])
__device__ __forceinline__ void ce_grads(const float* __restrict__ x, const long long* __restrict__ target, long long constant,
                                         const float* __restrict__ weight, int B, int C, float scale, float* __restrict__ g) {
    for (int i = threadIdx.x; i < B; i += 256) {
        const long long y = target_of(target, constant, i);
        const float* xi = x + (size_t)i * C;
        float* gi = g + (size_t)i * C;
        if (y < 0 || y >= C) {
            for (int c = 0; c < C; ++c) gi[c] = 0.f;
            continue;
        }
        const RowStat r = row_stat(xi, C);
        const float k = scale * (weight ? weight[y] : 1.f);
        for (int c = 0; c < C; ++c) {
            const float p = expf(xi[c] - r.m) / r.s;
            gi[c] = k * (p - (c == (int)y ? 1.f : 0.f));
        }
    }
}

__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ x, const long long* __restrict__ target,
                                                    const float* __restrict__ weight, float* __restrict__ loss,
                                                    float* __restrict__ g, int B, int C, int reduction) {
    __shared__ double red[256];
    double num, den;
    ce_sums(x, target, 0, weight, B, C, red, num, den);
    const double div = reduction == 0 ? den : 1.0;           // torch's mean: sum w l / sum w
    if (threadIdx.x == 0) loss[0] = (float)(num / div);
    if (g) ce_grads(x, target, 0, weight, B, C, (float)(1.0 / div), g);
}

// losses[0] = CE(logits, label);  losses[1] = (CE(d_mri, 1) + CE(d_pet, 0)) / 2;  the domain heads have two classes
__global__ __launch_bounds__(256) void adv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ dm,
                                                     const float* __restrict__ dp, const long long* __restrict__ label,
                                                     const float* __restrict__ weight, float* __restrict__ losses,
                                                     float* __restrict__ gx, float* __restrict__ gm, float* __restrict__ gp,
                                                     int B, int C) {
    __shared__ double red[256];
    double num, den, nm, dmn, np, dpn;
    ce_sums(x, label, 0, weight, B, C, red, num, den);
    ce_sums(dm, nullptr, 1, nullptr, B, 2, red, nm, dmn);
    ce_sums(dp, nullptr, 0, nullptr, B, 2, red, np, dpn);
    if (threadIdx.x == 0) {
        losses[0] = (float)(num / den);
        losses[1] = (float)(0.5 * (nm / dmn + np / dpn));
    }
    if (gx) {
        ce_grads(x, label, 0, weight, B, C, (float)(1.0 / den), gx);
        ce_grads(dm, nullptr, 1, nullptr, B, 2, (float)(0.5 / dmn), gm);
        ce_grads(dp, nullptr, 0, nullptr, B, 2, (float)(0.5 / dpn), gp);
    }
}

// d = s * g over up to three tensors laid end to end in the index space: [0, n0) tensor 0 scaled by s0[0], then n1 elements
// of tensor 1 and n1 of tensor 2 scaled by s1[0].  A NULL scalar is zero.
__global__ __launch_bounds__(256) void scale3_kernel(const float* __restrict__ g0, const float* __restrict__ g1,
                                                    const float* __restrict__ g2, const float* __restrict__ s0,
                                                    const float* __restrict__ s1, float* __restrict__ d0, float* __restrict__ d1,
                                                    float* __restrict__ d2, int n0, int n1) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n0) {
        d0[e] = s0 ? s0[0] * g0[e] : 0.f;
    } else if (e < n0 + n1) {
        d1[e - n0] = s1 ? s1[0] * g1[e - n0] : 0.f;
    } else if (e < n0 + 2 * n1) {
        d2[e - n0 - n1] = s1 ? s1[0] * g2[e - n0 - n1] : 0.f;
    }
}

// state (8 x 8 bytes): [0] updates, [1] samples (int64); [2] sum ce_loss, [3] sum ad_loss (double); [4..6] correct
// predictions of the label head, the MRI domain head (target 1) and the PET domain head (target 0) (int64); [7] unused
__global__ __launch_bounds__(256) void train_metrics_kernel(long long* __restrict__ state, const float* __restrict__ losses,
                                                           const float* __restrict__ x, const float* __restrict__ dm,
                                                           const float* __restrict__ dp, const long long* __restrict__ label,
                                                           int B, int C) {
    __shared__ int red[256];
    int ok = 0, okm = 0, okp = 0;
    for (int i = threadIdx.x; i < B; i += 256) {
        ok += (long long)row_argmax(x + (size_t)i * C, C) == label[i];
        okm += row_argmax(dm + (size_t)i * 2, 2) == 1;
        okp += row_argmax(dp + (size_t)i * 2, 2) == 0;
    }
    ok = block_sum(ok, red);
    okm = block_sum(okm, red);
    okp = block_sum(okp, red);
    if (threadIdx.x == 0) {
        double* sums = reinterpret_cast<double*>(state);
        state[0] += 1;
        state[1] += B;
        sums[2] += (double)losses[0];
        sums[3] += (double)losses[1];
        state[4] += ok;
        state[5] += okm;
        state[6] += okp;
    }
}

// state (2 + C * C words of 8 bytes, then three the AUC leaves its result in): [0] sum of the per-sample CE (double),
// [1] samples (int64), [2 + t * C + p] samples of true class t predicted as p (int64).
__global__ __launch_bounds__(256) void eval_metrics_kernel(long long* __restrict__ state, float* __restrict__ scores,
                                                          long long* __restrict__ labels_out, long offset,
                                                          const float* __restrict__ x, const long long* __restrict__ label,
                                                          int B, int C) {
    __shared__ double red[256];
    __shared__ unsigned short code[CE_MAX_B];    // true * C + predicted of each sample; 0xFFFF: a label outside [0, C)
    double a = 0.0;
    for (int i = threadIdx.x; i < B; i += 256) {
        const float* xi = x + (size_t)i * C;
        const long long y = label[i];
        const RowStat r = row_stat(xi, C);
        scores[offset + i] = expf(xi[C - 1] - r.m) / r.s;
        labels_out[offset + i] = y;
        if (y < 0 || y >= C) {
            a = __builtin_nan("");
            code[i] = 0xFFFFu;
            continue;
        }
        a += (double)(logf(r.s) - (xi[y] - r.m));
        code[i] = (unsigned short)((int)y * C + row_argmax(xi, C));
    }
    const double tot = block_sum(a, red);        // its barriers publish `code`
    if ((int)threadIdx.x < C * C) {              // C <= 16: one thread per cell, every lane reads the same LDS word
        int n = 0;
        for (int i = 0; i < B; ++i) n += code[i] == threadIdx.x;
        state[2 + threadIdx.x] += n;
    }
    if (threadIdx.x == 0) {
        reinterpret_cast<double*>(state)[0] += tot;
        state[1] += B;
    }
}

// Workgroup (bx, by): positives among i in [bx * AUC_IB, ...) against negatives among j in [by * AUC_JB, ...):
// partial[by * gridDim.x + bx] = sum 2 [s_i > s_j] + [s_i == s_j].  A j that is no negative is staged as NaN, an i that is
// no positive is held as NaN: every comparison with it is false.
__global__ __launch_bounds__(256) void auc_pairs_kernel(const float* __restrict__ scores, const long long* __restrict__ labels,
                                                       int n, unsigned long long* __restrict__ partial) {
    __shared__ float sj[AUC_JB];
    __shared__ unsigned long long red[256];
    const float nan = __builtin_nanf("");
    const int j0 = blockIdx.y * AUC_JB;
    for (int k = threadIdx.x; k < AUC_JB; k += 256) {
        const int j = j0 + k;
        sj[k] = (j < n && labels[j] == 0) ? scores[j] : nan;
    }
    float si[AUC_IPT];
#pragma unroll
    for (int u = 0; u < AUC_IPT; ++u) {
        const int i = blockIdx.x * AUC_IB + u * 256 + threadIdx.x;
        si[u] = (i < n && labels[i] != 0) ? scores[i] : nan;
    }
    __syncthreads();
    const int nj = min(AUC_JB, n - j0);
    unsigned gt = 0, eq = 0;                     // <= AUC_IPT * AUC_JB each
    for (int k = 0; k < nj; ++k) {
        const float s = sj[k];
#pragma unroll
        for (int u = 0; u < AUC_IPT; ++u) {
            gt += si[u] > s;
            eq += si[u] == s;
        }
    }
    const unsigned long long t = block_sum(2ull * gt + eq, red);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// out[0] = T (sum of the partials), out[1] = P, out[2] = N
__global__ __launch_bounds__(256) void auc_finalize_kernel(const unsigned long long* __restrict__ partial, int np,
                                                          const long long* __restrict__ labels, int n,
                                                          unsigned long long* __restrict__ out) {
    __shared__ unsigned long long red[256];
    unsigned long long t = 0, p = 0;
    for (int k = threadIdx.x; k < np; k += 256) t += partial[k];
    for (int k = threadIdx.x; k < n; k += 256) p += labels[k] != 0;
    t = block_sum(t, red);
    p = block_sum(p, red);
    if (threadIdx.x == 0) {
        out[0] = t;
        out[1] = p;
        out[2] = (unsigned long long)n - p;
    }
}

int auc_grid_x(int n) { return tmf_cdiv(n, AUC_IB); }
int auc_grid_y(int n) { return tmf_cdiv(n, AUC_JB); }

}  // namespace

extern "C" int tmf_ce_ok(int B, int C) { return B >= 1 && B <= CE_MAX_B && C >= 2 && C <= CE_MAX_C; }

extern "C" int tmf_ce_fwd(const float* logits, const long long* target, const float* weight, float* loss, float* g, int B, int C,
                          int reduction, void* stream) {
    TMF_REQUIRE_PTR(logits); TMF_REQUIRE_PTR(target); TMF_REQUIRE_PTR(loss);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_ce_fwd: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    TMF_REQUIRE(reduction == 0 || reduction == 1, TMF_E_ARG, "tmf_ce_fwd: reduction=%d (0 mean | 1 sum)", reduction);
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, target, weight, loss, g, B, C, reduction);
    return tmf_launch_result("tmf_ce_fwd");
}

extern "C" int tmf_ce_bwd(const float* g, const float* grad_out, float* dlogits, int B, int C, void* stream) {
    TMF_REQUIRE_PTR(g); TMF_REQUIRE_PTR(grad_out); TMF_REQUIRE_PTR(dlogits);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_ce_bwd: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    hipLaunchKernelGGL(scale3_kernel, dim3(tmf_cdiv(B * C, 256)), dim3(256), 0, (hipStream_t)stream, g, (const float*)nullptr,
                       (const float*)nullptr, grad_out, (const float*)nullptr, dlogits, (float*)nullptr, (float*)nullptr, B * C, 0);
    return tmf_launch_result("tmf_ce_bwd");
}

extern "C" int tmf_adv_criterion_fwd(const float* logits, const float* d_mri, const float* d_pet, const long long* label,
                                     const float* weight, float* losses, float* g_logits, float* g_mri, float* g_pet, int B,
                                     int C, void* stream) {
    TMF_REQUIRE_PTR(logits); TMF_REQUIRE_PTR(d_mri); TMF_REQUIRE_PTR(d_pet); TMF_REQUIRE_PTR(label); TMF_REQUIRE_PTR(losses);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_adv_criterion_fwd: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    TMF_REQUIRE((g_logits == nullptr) == (g_mri == nullptr) && (g_logits == nullptr) == (g_pet == nullptr), TMF_E_NULL,
                "tmf_adv_criterion_fwd: g_logits, g_mri and g_pet go together");
    hipLaunchKernelGGL(adv_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, d_mri, d_pet, label, weight, losses,
                       g_logits, g_mri, g_pet, B, C);
    return tmf_launch_result("tmf_adv_criterion_fwd");
}

extern "C" int tmf_adv_criterion_bwd(const float* g_logits, const float* g_mri, const float* g_pet, const float* grad_ce,
                                     const float* grad_ad, float* dlogits, float* dmri, float* dpet, int B, int C, void* stream) {
    TMF_REQUIRE_PTR(g_logits); TMF_REQUIRE_PTR(g_mri); TMF_REQUIRE_PTR(g_pet);
    TMF_REQUIRE_PTR(dlogits); TMF_REQUIRE_PTR(dmri); TMF_REQUIRE_PTR(dpet);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_adv_criterion_bwd: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    hipLaunchKernelGGL(scale3_kernel, dim3(tmf_cdiv(B * C + 4 * B, 256)), dim3(256), 0, (hipStream_t)stream, g_logits, g_mri, g_pet,
                       grad_ce, grad_ad, dlogits, dmri, dpet, B * C, 2 * B);
    return tmf_launch_result("tmf_adv_criterion_bwd");
}

extern "C" int tmf_train_metrics_update(void* state, const float* losses, const float* logits, const float* d_mri,
                                        const float* d_pet, const long long* label, int B, int C, void* stream) {
    TMF_REQUIRE_PTR(state); TMF_REQUIRE_PTR(losses); TMF_REQUIRE_PTR(logits); TMF_REQUIRE_PTR(d_mri); TMF_REQUIRE_PTR(d_pet);
    TMF_REQUIRE_PTR(label);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_train_metrics_update: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    TMF_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, TMF_E_ALIGN, "tmf_train_metrics_update: state is not 8-byte aligned");
    hipLaunchKernelGGL(train_metrics_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<long long*>(state), losses,
                       logits, d_mri, d_pet, label, B, C);
    return tmf_launch_result("tmf_train_metrics_update");
}

extern "C" int tmf_eval_metrics_update(void* state, float* scores, long long* labels_out, long offset, const float* logits,
                                       const long long* label, int B, int C, void* stream) {
    TMF_REQUIRE_PTR(state); TMF_REQUIRE_PTR(scores); TMF_REQUIRE_PTR(labels_out); TMF_REQUIRE_PTR(logits); TMF_REQUIRE_PTR(label);
    TMF_REQUIRE(tmf_ce_ok(B, C), TMF_E_SHAPE, "tmf_eval_metrics_update: B=%d C=%d (1 <= B <= 4096, 2 <= C <= 16)", B, C);
    TMF_REQUIRE(offset >= 0, TMF_E_ARG, "tmf_eval_metrics_update: offset=%ld is negative", offset);
    TMF_REQUIRE((reinterpret_cast<uintptr_t>(state) & 7u) == 0, TMF_E_ALIGN, "tmf_eval_metrics_update: state is not 8-byte aligned");
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<long long*>(state), scores,
                       labels_out, offset, logits, label, B, C);
    return tmf_launch_result("tmf_eval_metrics_update");
}

extern "C" int tmf_auc_ok(long n) { return n >= 1 && n <= AUC_MAX_N; }

extern "C" size_t tmf_auc_workspace_bytes(long n) {
    return tmf_auc_ok(n) ? (size_t)auc_grid_x((int)n) * auc_grid_y((int)n) * sizeof(unsigned long long) : 0;
}

extern "C" int tmf_auc(const float* scores, const long long* labels, long n, void* workspace, void* out, void* stream) {
    TMF_REQUIRE_PTR(scores); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(workspace); TMF_REQUIRE_PTR(out);
    TMF_REQUIRE(tmf_auc_ok(n), TMF_E_SHAPE, "tmf_auc: n=%ld (1 <= n <= 65536)", n);
    TMF_REQUIRE(((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(out)) & 7u) == 0, TMF_E_ALIGN,
                "tmf_auc: workspace / out is not 8-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int gx = auc_grid_x((int)n), gy = auc_grid_y((int)n);
    unsigned long long* part = static_cast<unsigned long long*>(workspace);
    hipLaunchKernelGGL(auc_pairs_kernel, dim3(gx, gy), dim3(256), 0, s, scores, labels, (int)n, part);
    TMF_TRY(tmf_launch_result("tmf_auc"));
    hipLaunchKernelGGL(auc_finalize_kernel, dim3(1), dim3(256), 0, s, (const unsigned long long*)part, gx * gy, labels, (int)n,
                       static_cast<unsigned long long*>(out));
    return tmf_launch_result("tmf_auc");
}
