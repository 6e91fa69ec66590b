// adam.hip — the optimizer step of the reference's train_step as ONE launch.
//
// reference: kfold_train_adversarial.py:135 (`optimizer.step()`), utils/utils.py:38-39 (getOptimizer: torch.optim.Adam,
// lr 1e-4, betas (0.9, 0.999), eps 1e-8, weight decay 0) over the 156 parameter tensors of model_ad (4.17 M floats).
// torch's multi-tensor Adam needs ~10 launches for them (its per-launch tensor table is a kernel argument of limited
// size); here every tensor's pointers ride in ONE kernel-argument table (the two moment estimates live in two flat
// buffers owned by the optimizer, so a tensor costs 8 + 8 + 4 + 4 + 4 = 28 bytes of table) and a workgroup finds its tensor by a binary
// search over the chunk prefix sums.  SURVEY.md §8f rank 2.
//
// Update (torch.optim.Adam, amsgrad = False, maximize = False; weight_decay is L2 as in torch):
//   g' = g + wd * p;  m = m + (1 - b1) (g' - m);  v = b2 v + (1 - b2) g' g';
//   p = p - (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
#include "tmf_optim.h"

namespace {

constexpr int CHUNK = TMF_OPT_CHUNK;
using AdamTable = TmfTensorTable;              // the table, its search and its host loop are shared with sgd.hip (tmf_optim.h)

__global__ __launch_bounds__(256) void adam_step_kernel(const AdamTable t, float* __restrict__ m_, float* __restrict__ v_,
                                                        float step_size, float inv_sqrt_bc2, float omb1, float b2, float omb2,
                                                        float eps, float wd) {
    const int chunk = blockIdx.x;
    const int ti = tmf_table_find(t, chunk);
    const int base = (chunk - t.first[ti]) * CHUNK;
    const int n = t.numel[ti];
    float* __restrict__ p = t.p[ti];
    const float* __restrict__ g = t.g[ti];
    float* __restrict__ m = m_ + t.off[ti];
    float* __restrict__ v = v_ + t.off[ti];
    auto upd = [&](float& pe, float ge, float& me, float& ve) {
        ge += wd * pe;
        me += omb1 * (ge - me);
        ve = b2 * ve + omb2 * ge * ge;
        pe -= step_size * me / (sqrtf(ve) * inv_sqrt_bc2 + eps);
    };
    // 16-byte accesses where the tensor allows (storage offsets of views are only 4-byte aligned in general)
    const bool vec = (((size_t)p | (size_t)g | (size_t)m | (size_t)v) & 15) == 0;
#pragma unroll
    for (int it = 0; it < CHUNK / 1024; ++it) {
        const int e = base + it * 1024 + threadIdx.x * 4;
        if (e >= n) break;
        if (vec && e + 4 <= n) {
            f32x4 pv = *reinterpret_cast<f32x4*>(p + e), mv = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pe = pv[j], me = mv[j], ve = vv[j];
                upd(pe, gv[j], me, ve);
                pv[j] = pe; mv[j] = me; vv[j] = ve;
            }
            *reinterpret_cast<f32x4*>(p + e) = pv; *reinterpret_cast<f32x4*>(m + e) = mv; *reinterpret_cast<f32x4*>(v + e) = vv;
        } else {
            for (int j = 0; j < 4 && e + j < n; ++j) upd(p[e + j], g[e + j], m[e + j], v[e + j]);
        }
    }
}

}  // namespace

extern "C" int tmf_adam_step(int n, float* const* params, const float* const* grads, const long* numel,
                             float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                             double weight_decay, int step, void* stream) {
    TMF_REQUIRE_PTR(params); TMF_REQUIRE_PTR(grads); TMF_REQUIRE_PTR(numel); TMF_REQUIRE_PTR(exp_avg); TMF_REQUIRE_PTR(exp_avg_sq);
    TMF_REQUIRE(n > 0 && n <= TMF_ADAM_MAX_TENSORS, TMF_E_SHAPE, "tmf_adam_step: %d tensors (1 .. %d per call)", n,
                TMF_ADAM_MAX_TENSORS);
    TMF_REQUIRE(step >= 1, TMF_E_ARG, "tmf_adam_step: step=%d (the count INCLUDING this update, from 1)", step);
    TMF_REQUIRE(lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0. && weight_decay >= 0.,
                TMF_E_ARG, "tmf_adam_step: lr=%g betas=(%g, %g) eps=%g weight_decay=%g", lr, beta1, beta2, eps, weight_decay);
    TMF_REQUIRE_ALIGNED(exp_avg); TMF_REQUIRE_ALIGNED(exp_avg_sq);
    AdamTable t;
    int chunks = 0;
    TMF_TRY(tmf_table_fill("tmf_adam_step", n, params, grads, numel, t, &chunks, nullptr));
    if (t.n == 0) return TMF_OK;
    const double bc1 = 1.0 - pow(beta1, step), bc2 = 1.0 - pow(beta2, step);
    hipLaunchKernelGGL(adam_step_kernel, dim3(chunks), dim3(256), 0, (hipStream_t)stream, t, exp_avg, exp_avg_sq,
                       (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
                       (float)eps, (float)weight_decay);      // hyper-parameters arrive as doubles: 1 - beta is formed as torch forms it
    return tmf_launch_result("tmf_adam_step");
}

// elements of the flat state buffers tmf_adam_step and tmf_sgd_step address for these tensors (each tensor padded to a
// multiple of 4)
extern "C" long tmf_adam_state_elems(int n, const long* numel) {
    if (n <= 0 || numel == nullptr) return 0;
    long off = 0;
    for (int i = 0; i < n; ++i) off += tmf_state_padded(numel[i]);
    return off;
}
