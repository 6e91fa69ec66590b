// sgd.hip — torch.optim.SGD (weight decay, momentum) over all parameter tensors as ONE launch.
//
// reference: utils/utils.py:34-37 (getOptimizer with --optimizer SGD: torch.optim.SGD(lr, weight_decay), MultiStepLR [10, 26]),
// kfold_train_Mnet.py:85 (SGD(lr=0.001, momentum=0.9)).  torch's multi-tensor form splits the 156 parameter tensors of model_ad
// over several launches per arithmetic step; here they ride in the kernel-argument table of tmf_optim.h, as for Adam
// (adam.hip), and a workgroup finds its tensor by the same binary search.
//
// Update (torch.optim.SGD, dampening = 0, nesterov = False, maximize = False; weight_decay is L2 as in torch):
//   g' = g + wd * p
//   momentum == 0:  p -= lr * g'
//   momentum != 0:  buf = g'  for a tensor that has no momentum buffer yet (torch clones g': NOT scaled), else
//                   buf = momentum * buf + g';   p -= lr * buf
// The "no buffer yet" flag is one byte per tensor beside the table, so fresh and seasoned tensors share the launch; a fresh
// tensor's buffer is written without being read, so the caller's buffer needs no initial fill.
#include "tmf_optim.h"

namespace {

constexpr int CHUNK = TMF_OPT_CHUNK;

struct SgdTable {
    TmfTensorTable t;
    unsigned char fresh[TMF_ADAM_MAX_TENSORS];     // 1: the tensor has no momentum buffer yet (rows as in t)
};
static_assert(sizeof(SgdTable) <= 6144, "the table is a kernel argument");

template <bool MOMENTUM>
__global__ __launch_bounds__(256) void sgd_step_kernel(const SgdTable s, float* __restrict__ buf_, float lr, float momentum, float wd) {
    const int chunk = blockIdx.x;
    const int ti = tmf_table_find(s.t, chunk);
    const int base = (chunk - s.t.first[ti]) * CHUNK;
    const int n = s.t.numel[ti];
    float* __restrict__ p = s.t.p[ti];
    const float* __restrict__ g = s.t.g[ti];
    float* __restrict__ b = MOMENTUM ? buf_ + s.t.off[ti] : nullptr;
    const bool fresh = MOMENTUM && s.fresh[ti] != 0;           // uniform over the workgroup
    const bool decay = wd != 0.f;                              // torch leaves g alone at weight_decay == 0
    auto upd = [&](float& pe, float ge, float& be) {
        if (decay) ge += wd * pe;
        if (MOMENTUM) {
            be = fresh ? ge : momentum * be + ge;
            ge = be;
        }
        pe -= lr * ge;
    };
    // 16-byte accesses where the tensor allows (storage offsets of views are only 4-byte aligned in general)
    const bool vec = (((size_t)p | (size_t)g | (size_t)b) & 15) == 0;
#pragma unroll
    for (int it = 0; it < CHUNK / 1024; ++it) {
        const int e = base + it * 1024 + threadIdx.x * 4;
        if (e >= n) break;
        if (vec && e + 4 <= n) {
            f32x4 pv = *reinterpret_cast<f32x4*>(p + e), bv = {0.f, 0.f, 0.f, 0.f};
            const f32x4 gv = *reinterpret_cast<const f32x4*>(g + e);
            if (MOMENTUM && !fresh) bv = *reinterpret_cast<f32x4*>(b + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pe = pv[j], be = bv[j];
                upd(pe, gv[j], be);
                pv[j] = pe; bv[j] = be;
            }
            *reinterpret_cast<f32x4*>(p + e) = pv;
            if (MOMENTUM) *reinterpret_cast<f32x4*>(b + e) = bv;
        } else {
            for (int j = 0; j < 4 && e + j < n; ++j) {
                float be = (MOMENTUM && !fresh) ? b[e + j] : 0.f;
                upd(p[e + j], g[e + j], be);
                if (MOMENTUM) b[e + j] = be;
            }
        }
    }
}

}  // namespace

extern "C" int tmf_sgd_step(int n, float* const* params, const float* const* grads, const long* numel, float* momentum_buf,
                            const int* no_buffer_yet, double lr, double momentum, double weight_decay, void* stream) {
    TMF_REQUIRE_PTR(params); TMF_REQUIRE_PTR(grads); TMF_REQUIRE_PTR(numel);
    TMF_REQUIRE(n > 0 && n <= TMF_ADAM_MAX_TENSORS, TMF_E_SHAPE, "tmf_sgd_step: %d tensors (1 .. %d per call)", n,
                TMF_ADAM_MAX_TENSORS);
    TMF_REQUIRE(lr >= 0. && momentum >= 0. && weight_decay >= 0., TMF_E_ARG, "tmf_sgd_step: lr=%g momentum=%g weight_decay=%g",
                lr, momentum, weight_decay);
    const bool mom = momentum != 0.;
    if (mom) {
        TMF_REQUIRE(momentum_buf != nullptr && no_buffer_yet != nullptr, TMF_E_NULL,
                    "tmf_sgd_step: momentum=%g needs momentum_buf and no_buffer_yet (NULL only with momentum == 0)", momentum);
        TMF_REQUIRE_ALIGNED(momentum_buf);
    }
    SgdTable s;
    int chunks = 0;
    int src[TMF_ADAM_MAX_TENSORS];
    TMF_TRY(tmf_table_fill("tmf_sgd_step", n, params, grads, numel, s.t, &chunks, src));
    if (s.t.n == 0) return TMF_OK;
    for (int k = 0; k < s.t.n; ++k) s.fresh[k] = (mom && no_buffer_yet[src[k]] != 0) ? 1 : 0;
    if (mom)
        hipLaunchKernelGGL(sgd_step_kernel<true>, dim3(chunks), dim3(256), 0, (hipStream_t)stream, s, momentum_buf, (float)lr,
                           (float)momentum, (float)weight_decay);
    else
        hipLaunchKernelGGL(sgd_step_kernel<false>, dim3(chunks), dim3(256), 0, (hipStream_t)stream, s, (float*)nullptr, (float)lr,
                           (float)momentum, (float)weight_decay);
    return tmf_launch_result("tmf_sgd_step");
}
