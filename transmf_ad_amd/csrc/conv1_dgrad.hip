// conv1_dgrad.hip — data gradient of the first sNet block (Conv3d(1->C, 3x3x3) -> BatchNorm3d -> LeakyReLU -> MaxPool3d(2))
// WITHOUT the conv output, or anything else of size voxels x C, in HBM.  gfx950.
//
//   z_c(v)  = sum_t w[t][c] x~(v + t - 1)                      y = scale_c z + shift_c
//   dy_c(v) = dpool_c(window of v) [v is the window's FIRST maximum of y] (y > 0 ? 1 : slope)
//   dz_c(v) = scale_c (dy_c(v) - coef0_c - coef1_c invstd_c (z_c(v) - mean_c))          for EVERY voxel of the volume
//   dx(u)   = sum_t sum_c w[t][c] dz_c(u - t + 1)
//
// dx splits into the ROUTED part (dy: one non-zero per pooling window and channel) and the BATCHNORM part, which loses its
// channel dimension analytically:
//   dx(u) = sum_t P[u - t + 1][t]  -  sum_{t: v = u - t + 1 inside the volume} (a_t + sum_t' M[t][t'] x~(v + t' - 1))
//   P[v][t]  = sum_c w[t][c] scale_c dy_c(v)
//   a_t      = sum_c w[t][c] scale_c (coef0_c - coef1_c invstd_c mean_c)
//   M[t][t'] = sum_c w[t][c] w[t'][c] scale_c coef1_c invstd_c
// a, M and the collapsed interior stencil N[delta] = sum_{t' - t = delta} M[t][t'] (125 taps, for voxels all of whose 27
// neighbours lie inside the volume) are formed once in fp64 by c1_dgrad_prep_kernel; all-zero coef (eval mode) sets a flag
// that skips the part.
//
// c1_dgrad_kernel: one workgroup owns a z brick of TD x 8 x 8 voxels at even coordinates (so that it holds whole pooling
// windows) and writes the dx of its inner (TD - 2) x 6 x 6 voxels: every dz a dx needs is the workgroup's own, no sum crosses
// workgroups, no atomics, and every addition has a fixed place in a fixed order — results are bit-reproducible.  z comes from
// conv1_z.h (conv_tiles_*, window_*: the functions tmf_c1_bn_pool_fwd itself calls, same c1_split setting), in the fragment layout of conv1_fused.hip:
// a lane holds two complete windows of one channel, so the routing and dy are per-lane register work.  The workgroup loops
// over ALL channel groups; per group and M-tile the dy registers go through a wave-private LDS transpose ([voxel][channel])
// and come back as the A operand of 16 fp32 MFMAs (K = the group's 32 channels, B = the taps) that accumulate P[voxel][tap].
// P then goes to LDS tap-major and dx gathers its 27 entries in tap order; the BatchNorm stencil reads the fp32 halo brick.
//
// Budget (TD = 4): 256 threads, <= 256 registers at two waves per SIMD, zero scratch; LDS 62.2 KB with c1_split (three bf16
// images 14.6 KB + fp32 halo 2.4 KB + transpose 16.9 KB + P 27.8 KB + stencil 0.5 KB), 47.6 KB without: two workgroups per CU.
#include "conv1_z.h"

namespace {
using namespace c1z;

constexpr int OD_ = TD - 2, OH_ = TH - 2, OW_ = TW - 2;     // dx voxels per brick: the z brick without its one-voxel shell
constexpr int NOUT = OD_ * OH_ * OW_;
constexpr int NVOX = TD * TH * TW;
constexpr int TP = 33;                                      // transpose pitch (floats): conflict-free row reads
constexpr int PP = NVOX + 1;                                // P pitch per tap: the 27 taps of a lane's store land on 27 banks
// prepared numbers (floats): a[27] | sum a | M[27][27] | N[125] | flag (any coef != 0)
constexpr int PREP_A = 0, PREP_ASUM = 27, PREP_M = 28, PREP_N = PREP_M + 729, PREP_FLAG = PREP_N + 125, PREP_COUNT = PREP_FLAG + 1;
static_assert(NOUT <= 256, "one thread per dx voxel of a brick");

struct DArgs {
    const float* x;        // [B][D][H][W]
    const float* w;        // [27][C]
    const float* scale;    // [C]
    const float* shift;
    const float* dpool;    // [B][D/2][H/2][W/2][C]
    const float* prep;     // PREP_COUNT floats
    float* dx;             // [B][D][H][W]
    int D, H, W, C;
    int nD, nH, nW, ntiles;
    float slope;
};

__global__ __launch_bounds__(256) void c1_dgrad_prep_kernel(const float* __restrict__ w, const float* __restrict__ scale,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ coef, float* __restrict__ prep, int C) {
    for (int e = blockIdx.x * 256 + threadIdx.x; e < PREP_COUNT; e += gridDim.x * 256) {
        double acc = 0.0;
        auto a_of = [&](int t) {
            double s = 0.0;
            for (int c = 0; c < C; ++c)
                s += (double)w[t * C + c] * (double)scale[c] * ((double)coef[c] - (double)coef[C + c] * (double)invstd[c] * (double)mean[c]);
            return s;
        };
        auto m_of = [&](int t, int u) {
            double s = 0.0;
            for (int c = 0; c < C; ++c)
                s += (double)w[t * C + c] * (double)w[u * C + c] * ((double)scale[c] * (double)coef[C + c] * (double)invstd[c]);
            return s;
        };
        if (e < PREP_ASUM) {
            acc = a_of(e);
        } else if (e == PREP_ASUM) {
            for (int t = 0; t < 27; ++t) acc += a_of(t);
        } else if (e < PREP_N) {
            acc = m_of((e - PREP_M) / 27, (e - PREP_M) % 27);
        } else if (e < PREP_FLAG) {
            const int q = e - PREP_N, dd = q / 25 - 2, dh = (q / 5) % 5 - 2, dw = q % 5 - 2;
            for (int t = 0; t < 27; ++t) {
                const int ud = t / 9 + dd, uh = (t / 3) % 3 + dh, uw = t % 3 + dw;      // t' = t + delta, per axis
                if (ud >= 0 && ud < 3 && uh >= 0 && uh < 3 && uw >= 0 && uw < 3) acc += m_of(t, (ud * 3 + uh) * 3 + uw);
            }
        } else {
            for (int c = 0; c < 2 * C; ++c) acc += (coef[c] != 0.f) ? 1.0 : 0.0;
            acc = acc > 0.0 ? 1.0 : 0.0;
        }
        prep[e] = (float)acc;
    }
}

template <bool SPLIT>
__global__ __launch_bounds__(256, 2) void c1_dgrad_kernel(DArgs a) {
    constexpr int NIMG = SPLIT ? 3 : 1;
    __shared__ float halo[SPLIT ? NIMG * NHB_DW : 1];       // SPLIT: the three bf16 images of z's operand
    __shared__ float halo32[NHALO];                         // the fp32 brick: z without c1_split, the BatchNorm stencil
    __shared__ float tr[4 * 32 * TP];                       // per wave: dy of one M-tile as [voxel][channel]
    __shared__ float pl[27 * PP];                           // P[tap][voxel of the z brick]
    __shared__ float nst[128];                              // the interior BatchNorm stencil N[125], then sum a (broadcast reads)
    const unsigned hb_base = (unsigned)(size_t)(__attribute__((address_space(3))) const void*)halo;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, hsel = lane >> 5;
    const int OD = a.D / 2, OH = a.H / 2, OW = a.W / 2;
    const int ngroups = (a.C + 31) / 32;
    const bool bn_part = a.prep[PREP_FLAG] != 0.f;

    constexpr int HVN = (NHALO + 255) / 256;
    int hd_[HVN], hh_[HVN], hw_[HVN];
#pragma unroll
    for (int q = 0; q < HVN; ++q) {
        const int e = tid + q * 256;
        hw_[q] = e % HW; hh_[q] = (e / HW) % HH; hd_[q] = e / (HW * HH);
    }
    if (tid < 126) nst[tid] = tid < 125 ? a.prep[PREP_N + tid] : a.prep[PREP_ASUM];      // (published by the brick loop's first barrier)
    if (SPLIT) {                                            // pad elements (row tails, plane gaps) are read against zero weights
        for (int e = tid; e < NIMG * NHB_DW; e += 256) halo[e] = 0.f;
    }
    const unsigned lane_b = lane_base(hb_base, l31, hsel);
    const int vox = vox_off(l31);
    float* trw = tr + wave * 32 * TP;
    // this thread's dx voxel (z-brick coordinates 1 .. T - 2)
    const int ud = 1 + tid / (OH_ * OW_), uh = 1 + (tid / OW_) % OH_, uw = 1 + tid % OW_;

    // Every global load of a brick is issued well ahead of its use — a brick is short (a few thousand cycles), so a load waited for in
    // place would cost as much as the arithmetic: the NEXT brick's halo is fetched to registers while this one computes, the pooled
    // gradients of a channel group are requested ahead of its MFMAs, and a single channel group's taps are loaded once per workgroup.
    struct Brick { int b, zd0, zh0, zw0; };
    auto brick_of = [&](int tile) {
        int t = tile;
        const int jw = t % a.nW; t /= a.nW;
        const int jh = t % a.nH; t /= a.nH;
        const int jd = t % a.nD;
        return Brick{t / a.nD, OD_ * jd - 2, OH_ * jh - 2, OW_ * jw - 2};      // z-brick origin: even, may be -2
    };
    float hv[HVN];
    auto fetch = [&](int tile) {
        const Brick k = brick_of(tile);
        const float* xb = a.x + (size_t)k.b * a.D * a.H * a.W;
#pragma unroll
        for (int q = 0; q < HVN; ++q) {
            const int gd = k.zd0 - 1 + hd_[q], gh = k.zh0 - 1 + hh_[q], gw = k.zw0 - 1 + hw_[q];
            const bool ok = tid + q * 256 < NHALO && (unsigned)gd < (unsigned)a.D && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W;
            hv[q] = ok ? xb[((size_t)gd * a.H + gh) * a.W + gw] : 0.f;
        }
    };
    float bw[SPLIT ? 1 : 14];
    tmf_bf16x8 bwb[NIMG][3];
    float sc = 0.f, sh = 0.f;
    float bp[16];                                           // B of the P product: [k = channel 2 s + hsel of the group][j = tap l31]
    auto load_group = [&](int g) {
        const int n0 = g * 32, co = n0 + l31;
        const bool cv = co < a.C;
        if constexpr (SPLIT) weights_b16<true>(a.w, a.C, co, cv, hsel, bwb);
        else weights_f32(a.w, a.C, co, cv, hsel, bw);
        sc = cv ? a.scale[co] : 0.f;
        sh = cv ? a.shift[co] : 0.f;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int ch = n0 + 2 * s + hsel;
            bp[s] = (l31 < 27 && ch < a.C) ? a.w[l31 * a.C + ch] : 0.f;
        }
    };
    if (ngroups == 1) load_group(0);
    if ((int)blockIdx.x < a.ntiles) fetch(blockIdx.x);

    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const Brick bk = brick_of(tile);
        const int b = bk.b, zd0 = bk.zd0, zh0 = bk.zh0, zw0 = bk.zw0;
        __syncthreads();                                    // the previous brick's readers are done
#pragma unroll
        for (int q = 0; q < HVN; ++q) {
            const int e = tid + q * 256;
            if (e < NHALO) {
                halo32[e] = hv[q];
                if (SPLIT) store_halo_split(halo, hd_[q] * BPLANE + hh_[q] * BROW + hw_[q], hv[q]);
            }
        }
        __syncthreads();
        if (tile + (int)gridDim.x < a.ntiles) fetch(tile + gridDim.x);

        f32x16 pacc[NTI];
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) pacc[ti][r] = 0.f;

        for (int g = 0; g < ngroups; ++g) {
            const int co = g * 32 + l31;
            const bool cv = co < a.C;
            if (ngroups > 1) load_group(g);
            // the pooled gradients of this lane's windows, M-tile ti: pooled (od, oh, owb + q); a window below 0 or beyond the pooled
            // tensor does not exist
            float gq[NTI][2];
#pragma unroll
            for (int ti = 0; ti < NTI; ++ti) {
                const int mt = wave * NTI + ti;
                const int od = (zd0 >> 1) + (mt >> 2), oh = (zh0 >> 1) + 2 * ((mt >> 1) & 1) + hsel, owb = (zw0 >> 1) + 2 * (mt & 1);
                const bool win_dh = cv && (unsigned)od < (unsigned)OD && (unsigned)oh < (unsigned)OH;
#pragma unroll
                for (int q = 0; q < 2; ++q)
                    gq[ti][q] = (win_dh && (unsigned)(owb + q) < (unsigned)OW)
                                    ? a.dpool[((((size_t)b * OD + od) * OH + oh) * OW + (owb + q)) * a.C + co] : 0.f;
            }
#pragma unroll
            for (int ti = 0; ti < NTI; ++ti) {
                const int mt = wave * NTI + ti;             // M-tile of the brick (wave-uniform)
                f32x16 z;
                if constexpr (SPLIT) conv_tiles_b16<true, 1>(&z, lane_b, mt, bwb);
                else conv_tiles_f32<1>(&z, halo32, mt, vox, hsel, bw);
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    float y[8];
                    window_y(z, q, sc, sh, y);
                    const float ymax = window_max(y);
                    const float lrm = ymax > 0.f ? 1.f : a.slope;
                    const float add = sc * (gq[ti][q] * lrm);   // scale dy at the routed element
                    const int arg = window_arg(y, ymax);
#pragma unroll
                    for (int k = 0; k < 8; ++k) z[8 * q + k] = (k == arg) ? add : 0.f;
                }
                // [voxel][channel] through the wave's LDS tile; a wave's LDS operations execute in order
#pragma unroll
                for (int r = 0; r < 16; ++r) trw[frag_row(r, hsel) * TP + l31] = z[r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int s = 0; s < 16; ++s)
                    pacc[ti] = __builtin_amdgcn_mfma_f32_32x32x2f32(trw[l31 * TP + 2 * s + hsel], bp[s], pacc[ti], 0, 0, 0);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        }

        // P to LDS: accumulator row = voxel i of the M-tile (fragment-row order), column l31 = tap
#pragma unroll
        for (int ti = 0; ti < NTI; ++ti) {
            const int mt = wave * NTI + ti;
            const int td0 = 2 * (mt >> 2), th0 = 4 * ((mt >> 1) & 1), tw0 = 4 * (mt & 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int i = frag_row(r, hsel);
                const int vd = td0 + ((i >> 3) & 1), vh = th0 + 2 * ((i >> 2) & 1) + ((i >> 1) & 1), vw = tw0 + 2 * ((i >> 4) & 1) + (i & 1);
                if (l31 < 27) pl[l31 * PP + (vd * TH + vh) * TW + vw] = pacc[ti][r];
            }
        }
        __syncthreads();

        if (tid < NOUT) {
            const int gd = zd0 + ud, gh = zh0 + uh, gw = zw0 + uw;
            if ((unsigned)gd < (unsigned)a.D && (unsigned)gh < (unsigned)a.H && (unsigned)gw < (unsigned)a.W) {
                float routed = 0.f;                         // sum_t P[u - t + 1][t], t ascending
#pragma unroll
                for (int tp = 0; tp < 27; ++tp) {
                    const int vd = ud - tp / 9 + 1, vh = uh - (tp / 3) % 3 + 1, vw = uw - tp % 3 + 1;
                    routed += pl[tp * PP + (vd * TH + vh) * TW + vw];
                }
                float bn = 0.f;
                if (bn_part) {
                    const int hc = ((ud + 1) * HH + (uh + 1)) * HW + (uw + 1);      // u in the halo brick
                    const bool inner = gd >= 1 && gd + 1 < a.D && gh >= 1 && gh + 1 < a.H && gw >= 1 && gw + 1 < a.W;
                    if (inner) {
                        bn = nst[125];
#pragma unroll
                        for (int q = 0; q < 125; ++q) {
                            const int dd = q / 25 - 2, dh = (q / 5) % 5 - 2, dw = q % 5 - 2;
                            bn = fmaf(nst[q], halo32[hc + (dd * HH + dh) * HW + dw], bn);
                        }
                    } else {
                        for (int tp = 0; tp < 27; ++tp) {
                            const int kd = tp / 9, kh = (tp / 3) % 3, kw = tp % 3;
                            const int vd = gd - kd + 1, vh = gh - kh + 1, vw = gw - kw + 1;
                            if ((unsigned)vd < (unsigned)a.D && (unsigned)vh < (unsigned)a.H && (unsigned)vw < (unsigned)a.W) {
                                const int hvox = hc + ((1 - kd) * HH + (1 - kh)) * HW + (1 - kw);  // v in the halo brick
                                float sv = a.prep[PREP_A + tp];
#pragma unroll
                                for (int tq = 0; tq < 27; ++tq)
                                    sv = fmaf(a.prep[PREP_M + tp * 27 + tq],
                                              halo32[hvox + ((tq / 9 - 1) * HH + ((tq / 3) % 3 - 1)) * HW + (tq % 3 - 1)], sv);
                                bn += sv;
                            }
                        }
                    }
                }
                a.dx[(size_t)b * a.D * a.H * a.W + ((size_t)gd * a.H + gh) * a.W + gw] = routed - bn;
            }
        }
    }
}

}  // namespace

extern "C" size_t tmf_c1_bwd_dgrad_workspace_bytes(int B, int D, int H, int W, int C) {
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)((PREP_COUNT + 3) / 4 * 4) * 4;
}

extern "C" int tmf_c1_bwd_dgrad(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                                const float* invstd, const float* coef, const float* dpool, float* dx,
                                void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int C, float slope, void* stream) {
    TMF_REQUIRE_PTR(x); TMF_REQUIRE_PTR(w); TMF_REQUIRE_PTR(scale); TMF_REQUIRE_PTR(shift); TMF_REQUIRE_PTR(mean);
    TMF_REQUIRE_PTR(invstd); TMF_REQUIRE_PTR(coef); TMF_REQUIRE_PTR(dx); TMF_REQUIRE_PTR(workspace);
    int rc = check_shape("tmf_c1_bwd_dgrad", B, D, H, W, C);
    if (rc) return rc;
    const bool no_windows = D / 2 == 0 || H / 2 == 0 || W / 2 == 0;      // an empty pooled tensor is valid (and may have no storage)
    TMF_REQUIRE(dpool != nullptr || no_windows, TMF_E_NULL, "tmf_c1_bwd_dgrad: argument 'dpool' is NULL");
    const size_t need = tmf_c1_bwd_dgrad_workspace_bytes(B, D, H, W, C);
    TMF_REQUIRE(workspace_bytes >= need, TMF_E_WORKSPACE, "tmf_c1_bwd_dgrad: workspace %zu B < required %zu B", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    float* prep = (float*)workspace;
    hipLaunchKernelGGL(c1_dgrad_prep_kernel, dim3(tmf_cdiv(PREP_COUNT, 256)), dim3(256), 0, s, w, scale, mean, invstd, coef, prep, C);
    if ((rc = tmf_launch_result("tmf_c1_bwd_dgrad(prepare)"))) return rc;
    DArgs a = {};
    a.x = x; a.w = w; a.scale = scale; a.shift = shift; a.dpool = dpool; a.prep = prep; a.dx = dx;
    a.D = D; a.H = H; a.W = W; a.C = C; a.slope = slope;
    a.nD = D / OD_ + 1; a.nH = H / OH_ + 1; a.nW = W / OW_ + 1;          // brick j writes dx of OD_ j - 1 .. OD_ j + OD_ - 2
    const long ntiles = (long)B * a.nD * a.nH * a.nW;
    TMF_REQUIRE(ntiles < (1L << 31), TMF_E_SHAPE, "tmf_c1_bwd_dgrad: too many bricks");
    a.ntiles = (int)ntiles;
    const int grid = ntiles < 8192 ? (int)ntiles : 8192;
    if (tmf_opt(TMF_OPT_C1_SPLIT)) hipLaunchKernelGGL((c1_dgrad_kernel<true>), dim3(grid), dim3(256), 0, s, a);
    else                           hipLaunchKernelGGL((c1_dgrad_kernel<false>), dim3(grid), dim3(256), 0, s, a);
    return tmf_launch_result("tmf_c1_bwd_dgrad");
}
