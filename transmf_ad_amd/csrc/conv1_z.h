// conv1_z.h — the ONE definition of z = conv(x) of the first sNet block as the fused passes evaluate it (gfx950).
//
// conv1_fused.hip (statistics, forward, reduce, weight gradient, one-pass backward) and conv1_dgrad.hip (the data
// gradient) recompute z from an LDS halo brick, and the max-pool routing every backward pass derives must be the
// forward's bit for bit.  That only holds while all of them issue the same products in the same order and pick the first
// maximum the same way, so the brick geometry, the LDS images, the operand fragments, the MFMA sequences (conv_tiles_*) and the
// window routing (window_*) live here and nowhere else: both files call them, neither restates them.  Everything is
// __forceinline__; the passes differ in what they do with z, not in how they obtain it.
#pragma once
#include "tmf_device.h"

namespace c1z {

#ifndef TMF_C1_TD
#define TMF_C1_TD 4
#endif
#ifndef TMF_C1X_ABL
#define TMF_C1X_ABL 0              // timing ablations of the SPLIT forward (wrong results): 1 = no stores, 2 = no MFMAs
#endif
constexpr int TD = TMF_C1_TD, TH = 8, TW = 8;
constexpr int NTI = TD / 2;                           // M-tiles per wave and brick (4 waves, TD * 2 tiles of 32 voxels)
constexpr int HD = TD + 2, HH = TH + 2, HW = TW + 2;
constexpr int NHALO = HD * HH * HW;

// bf16 passes: the halo brick lives in LDS as bf16, TWICE — copy c stores element e at index e + c — so that the pair
// (x[w], x[w + 1]) is one aligned dword for every w (even w: copy 0, odd w: copy 1).  A lane then fetches two taps per
// ds_read_b32 with no conversion: 9 reads per M-tile instead of 16 fp32 reads + 8 packs.  With the fp32 halo these passes
// were bound by the LDS port (PMC: half of all LDS cycles bank conflicts; no gather at all: 99 -> 37 us, stats, 128^3).
// Pitches (dwords) are chosen so that the five lane bits of a fragment row land on five different address bits:
//   w0 -> copy offset + 1 = 2 (mod 32), w1 -> 1, h0 -> 8, h1 -> 16, d0 -> 100 = 4 (mod 32): conflict-free ds_read_b32.
constexpr int BROW = 16, BPLANE = 200;                          // elements: row, plane
constexpr int BCP_DW = (HD * BPLANE / 2 + 1 + 31) / 32 * 32 + 1;    // copy pitch in dwords: = 1 (mod 32); TD = 4: 609 = 19 * 32 + 1
constexpr int BCOPY = 2 * BCP_DW;                               // ... in elements
constexpr int NHB_DW = 2 * BCP_DW;                              // dwords of LDS for both copies (copy 1 ends at 609 + 600 + 1)
static_assert(HD * BPLANE / 2 + 1 <= BCP_DW && HH * BROW <= BPLANE && HW + 2 <= BROW, "bf16 halo layout");
__device__ __forceinline__ constexpr int brow_off(int r) { return (r / 3) * BPLANE + (r % 3) * BROW; }   // tap row r = 3 dz + dy

__device__ __forceinline__ constexpr int tapoff(int tap) {
    return tap >= 27 ? 0 : ((tap / 9) * HH + (tap / 3) % 3) * HW + tap % 3;
}
// halo index (tap (0,0,0) corner) of M-tile t's origin, and of fragment row r (lane half 0) relative to it
__device__ __forceinline__ constexpr int row_off(int r) {   // r bits: b0 -> w0, b1 -> h0, b2 -> d0, b3 -> w1
    return (((r >> 2) & 1) * HH + ((r >> 1) & 1)) * HW + 2 * ((r >> 3) & 1) + (r & 1);
}

__device__ __forceinline__ tmf_bf16x8 pack8(const float (&v)[8]) {
    const tmf_u32x4 p = {tmf_pack_bf16(v[0], v[1]), tmf_pack_bf16(v[2], v[3]), tmf_pack_bf16(v[4], v[5]), tmf_pack_bf16(v[6], v[7])};
    return __builtin_bit_cast(tmf_bf16x8, p);
}

// ---- the taps as MFMA B operands for the lane's channel co (cv: the channel exists) -------------------------------------------
// bf16 / SPLIT: K = 48 = 3 MFMAs x (2 lane halves x 4 tap rows x 2 taps): k = 16 m + 8 hsel + 2 s + t is tap row r = 4 m + s
// (= 3 dz + dy), dx = 2 hsel + t — the lane half picks the pair (dx 0, 1) or (dx 2, pad); rows >= 9 and dx = 3 are zero.
// SPLIT: [part h / m / l][MFMA], the parts of split3_trunc.
template <bool SPLIT>
__device__ __forceinline__ void weights_b16(const float* w, int C, int co, bool cv, int hsel, tmf_bf16x8 (&bwb)[SPLIT ? 3 : 1][3]) {
    constexpr int NIMG = SPLIT ? 3 : 1;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = 4 * m + (j >> 1), dx = 2 * hsel + (j & 1);
            v[j] = (r < 9 && dx < 3 && cv) ? w[(3 * r + dx) * C + co] : 0.f;
        }
        if (SPLIT) {
            float vh[8], vm[8], vl[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) split3_trunc(v[j], vh[j], vm[j], vl[j]);
            bwb[0][m] = pack8(vh); bwb[NIMG > 1 ? 1 : 0][m] = pack8(vm); bwb[NIMG > 2 ? 2 : 0][m] = pack8(vl);
        } else {
            bwb[0][m] = pack8(v);
        }
    }
}
// fp32: 14 MFMAs of K = 2, k = lane half: tap 2 s + hsel (tap 27 is zero)
__device__ __forceinline__ void weights_f32(const float* w, int C, int co, bool cv, int hsel, float (&bw)[14]) {
#pragma unroll
    for (int s = 0; s < 14; ++s) {
        const int tap = 2 * s + hsel;
        bw[s] = (tap < 27 && cv) ? w[tap * C + co] : 0.f;
    }
}

// ---- one halo value into the LDS images ---------------------------------------------------------------------------------------
// hdst: element index in copy 0 (hd * BPLANE + hh * BROW + hw).  SPLIT: three images, one per part.
__device__ __forceinline__ void store_halo_split(float* halo, int hdst, float v) {
    float ph, pm, pl;
    split3_trunc(v, ph, pm, pl);
    const unsigned short p16[3] = {(unsigned short)(__builtin_bit_cast(unsigned, ph) >> 16),
                                   (unsigned short)(__builtin_bit_cast(unsigned, pm) >> 16),
                                   (unsigned short)(__builtin_bit_cast(unsigned, pl) >> 16)};
#pragma unroll
    for (int im = 0; im < 3; ++im) {
        unsigned short* dst = reinterpret_cast<unsigned short*>(halo) + im * (2 * NHB_DW) + hdst;
        dst[0] = p16[im];
        dst[BCOPY + 1] = p16[im];
    }
}
__device__ __forceinline__ void store_halo_bf16(float* halo, int hdst, float v) {
    const unsigned short h16 = (unsigned short)(tmf_pack_bf16(v, 0.f) & 0xFFFFu);
    unsigned short* dst = reinterpret_cast<unsigned short*>(halo) + hdst;
    dst[0] = h16;
    dst[BCOPY + 1] = h16;
}

// ---- A fragments: voxel i = lane & 31 of an M-tile in fragment-row order ------------------------------------------------------
// fp32 halo index of voxel i relative to its M-tile's origin, and of M-tile mt's origin in the brick
__device__ __forceinline__ int vox_off(int i) {
    return (((i >> 3) & 1) * HH + 2 * ((i >> 2) & 1) + ((i >> 1) & 1)) * HW + 2 * ((i >> 4) & 1) + (i & 1);
}
__device__ __forceinline__ constexpr int tile_org(int mt) { return ((2 * (mt >> 2)) * HH + 4 * ((mt >> 1) & 1)) * HW + 4 * (mt & 1); }
// bf16 images: per MFMA four dwords = the lane half's tap pair of four tap rows (rows >= 9 repeat row 8 against zero weights);
// the lane's LDS byte address is loop-invariant up to the M-tile origin
__device__ __forceinline__ unsigned lane_base(unsigned hb_base, int i, int hsel) {
    return hb_base + 2u * (unsigned)(((i >> 3) & 1) * BPLANE + (2 * ((i >> 2) & 1) + ((i >> 1) & 1)) * BROW +
                                     2 * ((i >> 4) & 1) + 2 * (i & 1) + (i & 1) * BCOPY + 2 * hsel);
}
__device__ __forceinline__ void load_rows(unsigned lane_b, int mt, int img, unsigned (&pr)[9]) {
    const unsigned tb = lane_b + 2u * (unsigned)((2 * (mt >> 2)) * BPLANE + 4 * ((mt >> 1) & 1) * BROW + 4 * (mt & 1)) +
                        (unsigned)(img * NHB_DW * 4);
#pragma unroll
    for (int r = 0; r < 9; ++r)
        pr[r] = *reinterpret_cast<const __attribute__((address_space(3))) unsigned*>((size_t)(tb + 2u * (unsigned)brow_off(r)));
}
__device__ __forceinline__ void mma_b16(f32x16& z, int m, const unsigned (&pr)[9], tmf_bf16x8 bw) {
    const tmf_u32x4 av = {pr[4 * m < 9 ? 4 * m : 8], pr[4 * m + 1 < 9 ? 4 * m + 1 : 8],
                      pr[4 * m + 2 < 9 ? 4 * m + 2 : 8], pr[4 * m + 3 < 9 ? 4 * m + 3 : 8]};
#if TMF_C1X_ABL & 2
    asm volatile("" :: "v"(av));
    z[m] += __builtin_bit_cast(float, av[0]);
#else
    z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(tmf_bf16x8, av), bw, z, 0, 0, 0);
#endif
}

// ---- z of N M-tiles mt0 .. mt0 + N - 1 of a wave, their MFMA chains interleaved (N = 1: one tile at a time, the form a pass with a
// tight register budget uses; the order of the products of a tile is the same for every N, so z is bit-identical) --------------
// SPLIT: image l, then m, then h — the products in ascending size: wh xl | wm xm, wh xm | wl xh, wm xh, wh xh.  (bf16: one image.)
template <bool SPLIT, int N>
__device__ __forceinline__ void conv_tiles_b16(f32x16* z, unsigned lane_b, int mt0, const tmf_bf16x8 (&bwb)[SPLIT ? 3 : 1][3]) {
#pragma unroll
    for (int ti = 0; ti < N; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) z[ti][r] = 0.f;
#pragma unroll
    for (int img = SPLIT ? 2 : 0; img >= 0; --img) {
        unsigned pr[N][9];
#pragma unroll
        for (int ti = 0; ti < N; ++ti) load_rows(lane_b, mt0 + ti, img, pr[ti]);
#pragma unroll
        for (int wp = SPLIT ? 2 - img : 0; wp >= 0; --wp)
#pragma unroll
            for (int m = 0; m < 3; ++m)
#pragma unroll
                for (int ti = 0; ti < N; ++ti) mma_b16(z[ti], m, pr[ti], bwb[SPLIT ? wp : 0][m]);
    }
}
// fp32 halo: tap 2 s + hsel per MFMA; vox = vox_off(lane & 31)
template <int N>
__device__ __forceinline__ void conv_tiles_f32(f32x16* z, const float* halo, int mt0, int vox, int hsel, const float (&bw)[14]) {
    int a_vox[N];
#pragma unroll
    for (int ti = 0; ti < N; ++ti) {
        a_vox[ti] = tile_org(mt0 + ti) + vox;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[ti][r] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < 14; ++s) {
        const int off = hsel ? tapoff(2 * s + 1) : tapoff(2 * s);
#pragma unroll
        for (int ti = 0; ti < N; ++ti)
            z[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(halo[a_vox[ti] + off], bw[s], z[ti], 0, 0, 0);
    }
}

// ---- first-maximum routing of one pooling window: y[k] = z[k] * sc + sh, k = 4 d + 2 h + w (torch scan order) -----------------
// LeakyReLU (slope > 0) is increasing, so the window maximum of the activation is the activation of the maximum of y; the routed
// element is the FIRST k with y[k] == max.  q: the lane's window (fragment rows 8 q .. 8 q + 7).
__device__ __forceinline__ void window_y(const f32x16& z, int q, float sc, float sh, float (&y)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) y[k] = z[8 * q + k] * sc + sh;
}
__device__ __forceinline__ float window_max(const float (&y)[8]) {
    return fmaxf(fmaxf(fmaxf(y[0], y[1]), fmaxf(y[2], y[3])), fmaxf(fmaxf(y[4], y[5]), fmaxf(y[6], y[7])));
}
__device__ __forceinline__ int window_arg(const float (&y)[8], float ymax) {
    int arg = 7;
#pragma unroll
    for (int k = 6; k >= 0; --k) arg = (y[k] == ymax) ? k : arg;
    return arg;
}
__device__ __forceinline__ float window_zsel(const float (&y)[8], float ymax, const f32x16& z, int q) {   // z of the first maximum
    float zs = z[8 * q + 7];
#pragma unroll
    for (int k = 6; k >= 0; --k) zs = (y[k] == ymax) ? z[8 * q + k] : zs;
    return zs;
}

// ---- the shapes every pass of the block accepts (host) ------------------------------------------------------------------------
inline int check_shape(const char* fn, int B, int D, int H, int W, int C) {
    TMF_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0 && C > 0, TMF_E_SHAPE, "%s: non-positive dimension", fn);
    TMF_REQUIRE((long)D * H * W * C < (1L << 31), TMF_E_SHAPE, "%s: one sample exceeds 2^31 elements", fn);
    TMF_REQUIRE((long)(D > 6 ? D : 6) * H * W < (1L << 29), TMF_E_SHAPE, "%s: the input volume exceeds 2^29 voxels", fn);
    return TMF_OK;
}

}  // namespace c1z
