// Device-only helpers shared by the kernel files of libtmf_hip.so (gfx950 only): ONE copy of each small primitive — buffer
// resources, LDS-DMA, counted waits, the store hazard pad, fragment maps, GELU, the exact bf16 splits.  Everything here is
// __forceinline__ and leaves no symbol in an object; the host-only files (snet_path.hip, fusion_path.hip, options.hip) do not
// need it.  A kernel file must not re-define one of these names in its anonymous namespace: the local one would silently win.
#pragma once
#include "tmf_common.h"

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// ---- buffer resources, LDS-DMA, counted waits ---------------------------------------------------------------------------------
// Raw buffer resource over `bytes` bytes at p (stride 0, range-checked: an access at or beyond `bytes` reads zeros / is dropped).
__device__ __forceinline__ i32x4 make_rsrc(const void* p, unsigned bytes) {
    const unsigned long long a = (unsigned long long)p;
    return i32x4{(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xFFFFu), (int)bytes, 0x00020000};
}
// LDS-DMA of 16 bytes per lane through a buffer resource: LDS byte = lds_wave_base (wave-uniform LDS address, via m0) + 16 * lane
// <- resource base + voff (per lane) + soff (scalar).  A lane whose voff + soff is not below the resource's num_records delivers
// ZEROS to its LDS bytes (gfx950: the scalar offset is part of the range check, tools/microbench/blds_probe.hip) — zero fill costs
// no pointer select, no compare.
// Written as inline assembly on purpose: with __builtin_amdgcn_global_load_lds the compiler cannot tell that the copy fills the
// OTHER buffer and waits vmcnt(0) before the first fragment read of every brick, which serialises copy and multiply (the first
// build of conv3d_bf16.hip did: 61 us of 240 exposed).  The price is that the compiler does not see the copies at all: the kernel
// waits for them itself (vm_wait) before the barrier that publishes the buffer.
//
// blds16: the plain form — soff and the descriptor as the caller has them.  Used by conv3d_bf16.hip and by every kernel of
// conv3d_wino.hip.
__device__ __forceinline__ void blds16(int voff, i32x4 rsrc, int soff, unsigned lds_wave_base) {
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(rsrc), "s"(soff), "s"(lds_wave_base) : "memory");
}
// blds16_uniform: the same instruction with soff pinned to a register (not a literal the instruction cannot encode) and the
// descriptor made wave-uniform word by word (readfirstlane folds away where it already sits in scalar registers).  Used by
// conv3d_winox.hip.  The two forms compile to different schedules around every copy, so neither file was moved to the other's:
// whether the kernels on the plain form are exposed to what this one guards against is unmeasured — a question for a change that
// measures it, not for a textual clean-up.
__device__ __forceinline__ void blds16_uniform(int voff, i32x4 rsrc, int soff, unsigned lds_wave_base) {
    asm volatile("" : "+s"(soff));
    rsrc = i32x4{__builtin_amdgcn_readfirstlane(rsrc[0]), __builtin_amdgcn_readfirstlane(rsrc[1]), __builtin_amdgcn_readfirstlane(rsrc[2]),
                 __builtin_amdgcn_readfirstlane(rsrc[3])};
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds" ::"v"(voff), "s"(rsrc), "s"(soff), "s"(lds_wave_base) : "memory");
}
// 16 bytes per lane to registers (V: f32x4 or i32x4), invisible to the compiler's wait-count pass: the kernel counts its waits
// itself (vm_wait) and re-defines the registers behind the wait, so that every use is ordered behind it.  Two forms for the
// same reason as above — bload16: plain, conv3d_wino.hip; bload16_pinned: soff pinned to a register, conv3d_winox.hip (on that
// form every persistent kernel of conv3d_wino.hip compiles to different code).
template <typename V> __device__ __forceinline__ void bload16(V& dst, int voff, i32x4 rsrc, int soff) {
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
template <typename V> __device__ __forceinline__ void bload16_pinned(V& dst, int voff, i32x4 rsrc, int soff) {
    asm volatile("" : "+s"(soff));
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(dst) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
// Wait until at most N vector-memory operations of this wave are outstanding (loads, LDS-DMA copies and stores retire in order).
// vm_wait<0>() is the wait behind the LDS-DMA copies above.
template <int N> __device__ __forceinline__ void vm_wait() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// A buffer_store_dwordx4 reads its data registers AFTER it has issued: a v_pk_* that overwrites them in the very next slot
// corrupted the second register of the pair in lanes 12-15 of every row of 16 (measured on gfx950 with an SGPR soffset, the
// case LLVM's hazard recognizer exempts; tools/asm_checks.py finds the pattern in a listing).  One wait state after a wide store
// whose data dies right behind it:
__device__ __forceinline__ void store_guard() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 0");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- MFMA fragment map, activation, half-wave sum -----------------------------------------------------------------------------
// row of element r (0..15) of a 32x32 fp32 accumulator in the lane half hsel
__device__ __forceinline__ int frag_row(int r, int hsel) { return (r & 3) + 8 * (r >> 2) + 4 * hsel; }

// exact (erf) GELU and its derivative: token_gemm.hip and xformer_fused.hip must agree bit for bit (dim 128 fused against the
// per-op path), hence one definition
__device__ __forceinline__ float gelu_f(float h) { return 0.5f * h * (1.f + erff(h * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_grad_f(float h) {
    return 0.5f * (1.f + erff(h * 0.70710678118654752f)) + h * 0.3989422804014327f * expf(-0.5f * h * h);
}
__device__ __forceinline__ float half_sum(float v) {         // sum over the 32 lanes of a half-wave
    v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
    return v;
}

// ---- exact 3-way bf16 splits: x = h + m + l, three bf16 numbers (8 + 8 + 8 significand bits), no rounding error ---------------
// The two roundings give DIFFERENT parts for the same x; which one a kernel's operand images were built with must not change.
// split3_trunc: h and m by truncation (the top 16 bits), l = the remaining <= 8 bits; the parts as fp32 numbers whose low 16 bits
// are zero.  conv1_fused.hip (SPLIT), the fp32x halo of conv3d_bf16.hip, the weight images of conv3d_wino.hip (wino_pack_one);
// conv3d_winox.hip restates it inline (split8).
__device__ __forceinline__ void split3_trunc(float x, float& h, float& m, float& l) {
    h = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, x) & 0xFFFF0000u);
    const float r = x - h;
    m = __builtin_bit_cast(float, __builtin_bit_cast(unsigned, r) & 0xFFFF0000u);
    l = r - m;
}
// split3_rne: every part rounded to nearest even; the parts as bf16 bit patterns.  The fp32x weight pack of token_ops.hip.
__device__ __forceinline__ unsigned short bf16_bits_rne(float a) { return __builtin_bit_cast(unsigned short, (__bf16)a); }
__device__ __forceinline__ void split3_rne(float a, unsigned short& h, unsigned short& m, unsigned short& l) {
    h = bf16_bits_rne(a);
    const float r1 = a - __builtin_bit_cast(float, (unsigned)h << 16);           // exact
    m = bf16_bits_rne(r1);
    const float r2 = r1 - __builtin_bit_cast(float, (unsigned)m << 16);          // exact, fits bf16
    l = bf16_bits_rne(r2);
}

// ---- Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1) -> four 32-bit words ----------------------------------
// Counter-based, so a draw is a pure function of (seed, counter): no generator state on the device, reproducible under a seed.
// The Dropout keep-masks of heads.hip and the RISE node grids and shifts of rise.hip; each keys it with its own domain constant.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                              unsigned (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// ---- the order-preserving uint32 image of a float ------------------------------------------------------------------------------
// ascending key <=> ascending a = x + 0.0f as floats (-0.0 ranks with +0.0; infinities are ordinary values).  The radix select of
// faithfulness.hip and the packed max / argmax of region_stats.hip.
__device__ __forceinline__ unsigned fc_key(float x) {
    unsigned u = __float_as_uint(x);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fc_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}
