// Shared host/device helpers for libtmf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/tmf_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
#ifdef __HIPCC__
typedef __bf16 tmf_bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 tmf_bf16x8 __attribute__((ext_vector_type(8)));
// two floats -> two bf16 (round-to-nearest-even, a in the low half): one v_cvt_pk_bf16_f32 on gfx950 (the integer emulation
// cost 8 VALU instructions per pair and made the staging of the bf16 kernels VALU-bound, PMC)
__device__ __forceinline__ unsigned int tmf_pack_bf16(float a, float b) {
    const tmf_bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(unsigned int, v);
}
// Typed activation I/O: float tensors, or bf16 tensors (unsigned short storage) widened to / rounded from fp32 registers.
typedef unsigned short tmf_bf16_t;
typedef unsigned int tmf_u32x2 __attribute__((ext_vector_type(2)));
typedef float tmf_f32x1 __attribute__((ext_vector_type(1)));
template <typename T, int VEC> struct TmfIO;
template <> struct TmfIO<float, 4> {
    static __device__ __forceinline__ f32x4 ld(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
    static __device__ __forceinline__ void st(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
    // streaming (read-once / write-once) forms: keep the lines out of L2 so that re-used data (halos, weights) stay
    static __device__ __forceinline__ f32x4 ld_nt(const float* p) { return __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p)); }
    static __device__ __forceinline__ void st_nt(float* p, f32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p)); }
};
template <> struct TmfIO<float, 1> {
    static __device__ __forceinline__ tmf_f32x1 ld(const float* p) { return *reinterpret_cast<const tmf_f32x1*>(p); }
    static __device__ __forceinline__ void st(float* p, tmf_f32x1 v) { *p = v[0]; }
};
template <> struct TmfIO<tmf_bf16_t, 4> {
    static __device__ __forceinline__ f32x4 ld(const tmf_bf16_t* p) {
        const tmf_u32x2 r = *reinterpret_cast<const tmf_u32x2*>(p);
        return f32x4{__builtin_bit_cast(float, r[0] << 16), __builtin_bit_cast(float, r[0] & 0xFFFF0000u),
                     __builtin_bit_cast(float, r[1] << 16), __builtin_bit_cast(float, r[1] & 0xFFFF0000u)};
    }
    static __device__ __forceinline__ void st(tmf_bf16_t* p, f32x4 v) {
        *reinterpret_cast<tmf_u32x2*>(p) = tmf_u32x2{tmf_pack_bf16(v[0], v[1]), tmf_pack_bf16(v[2], v[3])};
    }
};
typedef float tmf_f32x8 __attribute__((ext_vector_type(8)));
typedef unsigned int tmf_u32x4 __attribute__((ext_vector_type(4)));
template <> struct TmfIO<float, 8> {
    static __device__ __forceinline__ tmf_f32x8 ld(const float* p) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
        return tmf_f32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    }
    static __device__ __forceinline__ void st(float* p, tmf_f32x8 v) {
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
    }
};
template <> struct TmfIO<tmf_bf16_t, 8> {          // one 16-byte access per lane
    static __device__ __forceinline__ tmf_f32x8 ld(const tmf_bf16_t* p) {
        const tmf_u32x4 r = *reinterpret_cast<const tmf_u32x4*>(p);
        tmf_f32x8 v;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[2 * i] = __builtin_bit_cast(float, r[i] << 16);
            v[2 * i + 1] = __builtin_bit_cast(float, r[i] & 0xFFFF0000u);
        }
        return v;
    }
    static __device__ __forceinline__ void st(tmf_bf16_t* p, tmf_f32x8 v) {
        *reinterpret_cast<tmf_u32x4*>(p) = tmf_u32x4{tmf_pack_bf16(v[0], v[1]), tmf_pack_bf16(v[2], v[3]),
                                                      tmf_pack_bf16(v[4], v[5]), tmf_pack_bf16(v[6], v[7])};
    }
};
template <> struct TmfIO<tmf_bf16_t, 1> {
    static __device__ __forceinline__ tmf_f32x1 ld(const tmf_bf16_t* p) {
        return tmf_f32x1{__builtin_bit_cast(float, (unsigned int)(*p) << 16)};
    }
    static __device__ __forceinline__ void st(tmf_bf16_t* p, tmf_f32x1 v) {
        *p = (tmf_bf16_t)(tmf_pack_bf16(v[0], 0.f) & 0xFFFFu);
    }
};
#endif

void tmf_set_error(const char* fmt, ...);
// conv3d_mfma.hip: tmf_conv3d_fwd / tmf_conv3d_stat_blocks with a per-call minimum for the "conv_rt" mode (snet_path.hip: TMF_SNET_ALONE)
int tmf_conv3d_fwd_mode(const float* x, const float* w, float* z, float* stat_partial, int B, int D, int H, int W, int cin,
                        int cout, int ksize, int rt_min, void* stream);
int tmf_conv3d_stat_blocks_mode(int B, int D, int H, int W, int cin, int cout, int ksize, int rt_min);
// Process options (options.hip: one table row each; include/tmf_hip.h documents them).  tmf_opt: the value in effect — the
// calling entry's choice for the options of the per-call word (below), else tmf_set_option's, else the environment's, else the default.
enum TmfOpt {
    TMF_OPT_CONV_WINO, TMF_OPT_WINO_P, TMF_OPT_WINO_X, TMF_OPT_C1_GRAM, TMF_OPT_C1_SPLIT, TMF_OPT_POOL_RECOMPUTE,   // (also per call)
    TMF_OPT_WINO_CUS, TMF_OPT_CONV_RT, TMF_OPT_CONV_WAVES, TMF_OPT_BF16_V2, TMF_OPT_BF16_DMA, TMF_OPT_WGRAD_TR, TMF_OPT_DEBUG,
    TMF_OPT_WINO_EVEN, TMF_OPT_WINOX_SWAP, TMF_OPT_BF_NT2, TMF_OPT_CONV_AUTO, TMF_OPT_C1_BLOCKS, TMF_OPT_C1_FWD_MULT,   // (environment only)
    TMF_OPT_COUNT
};
int tmf_opt(TmfOpt o);
// per-call algorithm choice (tmf_snet_desc.flags & TMF_SNET_ALGO): the whole-encoder entries hold it for the calling thread while they
// plan and enqueue (a word without TMF_SNET_ALGO keeps the one held before); tmf_opt decodes it for the options it carries
struct TmfAlgoScope {       // options.hip
    int prev;
    explicit TmfAlgoScope(int flags);
    ~TmfAlgoScope();
    TmfAlgoScope(const TmfAlgoScope&) = delete;
    TmfAlgoScope& operator=(const TmfAlgoScope&) = delete;
};
int tmf_winox_takes(int B, int D, int H, int W, int cin, int cout, int geom);
long tmf_winox_items(int D, int H, int W, int* swap);     // items per sample (the better of the two item orientations)
int tmf_winox_first_grid(long nitems, int ncu);           // workgroups of a launch's first window
int tmf_winox_launch(const char* what, const float* x, const unsigned short* u3, float* z, float* stat_partial, int B, int D, int H,
                     int W, int cin, int cout, int ncu, hipStream_t stream, const float* scale = nullptr, const float* shift = nullptr,
                     float slope = 0.f, int pool = 0);     // scale != NULL: the eval-mode block (y = LeakyReLU(scale z + shift), pool none | max)
// token_gemm.hip / token_ops.hip: the one implementation behind each plain / _masked pair of exported entries, for fusion_path.hip
// to call with whatever mask it has.  mask NULL: the plain entry's launch and name (dx_masked is not looked at), else the _masked one's
#define TMF_INTERNAL __attribute__((visibility("hidden")))      // not among the library's dynamic symbols
TMF_INTERNAL
int tmf_tok_linear_fwd_impl(const float* x, const float* w, const float* bias, const float* residual, float* y, int R, int K,
                            int Nout, const float* ln_gamma, const float* ln_beta, float eps, float* ln_mean, float* ln_rstd,
                            float* ln_out, float* gelu_pre, const float* mask, void* stream);
TMF_INTERNAL
int tmf_tok_linear_bwd_input_impl(const float* dy, const float* w, float* dx, int R, int Nout, int K, const float* gelu_pre,
                                 const float* ln_x, const float* ln_mean, const float* ln_rstd, const float* ln_gamma,
                                 const float* add1, const float* add2, float* ln_partial, float* bias_partial,
                                 int partial_stride, const float* mask, float* dx_masked, void* stream);
TMF_INTERNAL
int tmf_layernorm_bwd_impl(const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy, float* dx,
                          float* partial, int rows, int dim, const float* mask, float* dx_masked, void* stream);

#define TMF_REQUIRE_PTR(p)                                                     \
    do {                                                                       \
        if ((p) == nullptr) {                                                  \
            tmf_set_error("%s: argument '%s' is NULL", __func__, #p);          \
            return TMF_E_NULL;                                                 \
        }                                                                      \
    } while (0)

#define TMF_REQUIRE_ALIGNED(p)                                                 \
    do {                                                                       \
        if ((reinterpret_cast<uintptr_t>(p) & 15u) != 0) {                     \
            tmf_set_error("%s: argument '%s' is not 16-byte aligned", __func__, #p); \
            return TMF_E_ALIGN;                                                \
        }                                                                      \
    } while (0)

#define TMF_REQUIRE(cond, code, ...)                                           \
    do {                                                                       \
        if (!(cond)) {                                                         \
            tmf_set_error(__VA_ARGS__);                                        \
            return (code);                                                     \
        }                                                                      \
    } while (0)

// TMF_REQUIRE_PTR / TMF_REQUIRE_ALIGNED inside an implementation that several entries share: fn is the calling entry's name
#define TMF_REQUIRE_PTR_FN(fn, p) TMF_REQUIRE((p) != nullptr, TMF_E_NULL, "%s: argument '%s' is NULL", (fn), #p)
#define TMF_REQUIRE_ALIGNED_FN(fn, p) \
    TMF_REQUIRE((reinterpret_cast<uintptr_t>(p) & 15u) == 0, TMF_E_ALIGN, "%s: argument '%s' is not 16-byte aligned", (fn), #p)

// propagate a non-zero status of a library call to the caller
#define TMF_TRY(call) do { int rc__ = (call); if (rc__ != TMF_OK) return rc__; } while (0)

// Returns 0 or the (positive) hipError_t of the launch that just happened.  tag: what a shared implementation adds to the
// calling entry's name `what`, e.g. "(ln,gelu)".
static inline int tmf_launch_result(const char* what, const char* tag = "") {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        tmf_set_error("%s%s: launch failed: %s", what, tag, hipGetErrorString(e));
        return (int)e;
    }
    return TMF_OK;
}

// Opt a kernel into > 64 KiB of dynamic LDS (gfx950 has 160 KiB per CU).
template <typename K>
static inline int tmf_allow_lds(K kernel, size_t bytes, const char* what) {
    // once per kernel instantiation and size (K is a distinct function-pointer VALUE per call site, so key on it)
    // ... and on the device: the attribute belongs to the function ON ONE DEVICE, so a second GPU driven from the
    // same thread needs its own call
    static thread_local const void* last_fn[8] = {};
    static thread_local size_t last_sz[8] = {};
    static thread_local int last_dev[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    const void* fn = reinterpret_cast<const void*>(kernel);
    const unsigned slot = (unsigned)((reinterpret_cast<uintptr_t>(fn) >> 4) & 7u);
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (last_fn[slot] == fn && last_dev[slot] == dev && last_sz[slot] >= bytes) return TMF_OK;
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        tmf_set_error("%s: cannot reserve %zu B of LDS: %s", what, bytes, hipGetErrorString(e));
        return (int)e;
    }
    last_fn[slot] = fn;
    last_sz[slot] = bytes;
    last_dev[slot] = dev;
    return TMF_OK;
}

static inline int tmf_cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }     // arena offsets: 256-byte granules

// Workgroups of one window of n items of a persistent Winograd launch on ncu compute units: min(n, ncu), and with `even` as few
// as the window's number of ROUNDS needs (864 items on 256 CUs are 4 rounds: 216 workgroups of exactly 4 items take as long as
// 256 of 3 or 4 and leave 40 CUs to the other encoder's stream).  The statistic rows at and past this count are zeros.
static inline int tmf_wino_window_grid(long n, int ncu, int even) {
    if (n <= ncu) return (int)n;
    if (!even) return ncu;
    const long rounds = (n + ncu - 1) / ncu;
    return (int)((n + rounds - 1) / rounds);
}

// Two-stage slab reduction plan: `groups` first-stage groups (1 = single stage straight into `out`).
static inline int tmf_reduce_groups(int nsplit) {
    if (nsplit <= 64) return 1;
    int g = nsplit / 16;
    return g > 32 ? 32 : g;
}
// Reduce `nsplit` slabs of `n` floats into out[n].  `scratch` (>= tmf_reduce_groups(nsplit)*n floats) is only
// touched when the plan has two stages.
// tcin / tcout > 0 (weight gradients, dw_layout == TMF_DW_REFERENCE): the final stage stores in the nn.Conv3d layout.
int tmf_reduce_slabs(const float* partial, int nsplit, long n, float* scratch, float* out, hipStream_t s, const char* what,
                     int tcin = 0, int tcout = 0);        // reduce.hip

#ifdef __HIPCC__
// MI355X dispatches workgroup b to XCD b % 8 (speed hint only, MI355X_MICROARCH.md).
// Map the launch index so that each XCD (= one private L2) walks a contiguous range
// of tiles: neighbouring tiles share their halo in that L2.  Bijective for any n: XCD x takes n / 8 indices, the first
// n % 8 XCDs one more.  The ONE placement rule of the library — the persistent Winograd kernels apply it to their workgroup
// index (window slot) too; tmf_xcd_slot (conv3d_wino.hip) shows it to host tests.
__host__ __device__ __forceinline__ int xcd_contiguous(int bid, int n) {
    const int q = n >> 3, r = n & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + idx;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
#endif
