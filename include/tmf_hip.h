/*
 * tmf_hip.h — C ABI of libtmf_hip.so: the MI355X (gfx950) kernels behind the
 * TransMF_AD forward/backward hot path.
 *
 * The reference (Kateridge/TransMF_AD) has no FFI of its own: the whole path is a
 * sequence of ATen calls issued by Python nn.Modules.  Each entry point below
 * therefore replaces a group of ATen calls at a cited reference call site; the
 * Python package `transmf_ad_amd` binds them with ctypes (transmf_ad_amd/_lib.py)
 * from torch.autograd.Functions, and INTEGRATION.md shows the binding a reference
 * maintainer would add.
 *
 * Conventions
 *  - All pointers are DEVICE pointers (hipMalloc'd / torch.Tensor.data_ptr()),
 *    fp32 unless stated; all buffers, including workspaces, are caller-allocated.
 *  - Activations are channels-last:  x[b][d][h][w][c]  ("NDHWC").
 *  - 3x3x3 weights are tap-major:    w[kd*9+kh*3+kw][cin][cout]; 1x1x1: w[cin][cout].
 *  - `stream` is a hipStream_t passed as void*; every call is asynchronous on it,
 *    never synchronises, never allocates, never throws.  Re-entrant: no state is
 *    kept between calls, but the kernel choice follows the process options
 *    (tmf_set_option below), which a call carrying TMF_SNET_ALGO overrides with its own.
 *  - Return: 0 = launched; <0 = TMF_E_* argument error (nothing launched);
 *    >0 = hipError_t from the launch.  tmf_last_error_string() describes the last
 *    non-zero return on the calling thread.
 *
 * How this file is written (transmf_ad_amd/_lib.py parses it at import into the ctypes prototypes, Structure classes and
 * constants, and refuses what it cannot map):
 *  - one declaration per `;`, every parameter named, no function pointers;
 *  - scalar types int, long, long long, unsigned long long, size_t, float, double (struct fields also int32_t);
 *  - structs as `typedef struct tmf_x { ... } tmf_x;`, array sizes literal or a TMF_* define;
 *  - a `tmf_x*` parameter is a HOST struct, except tmf_augment_decision (records in device memory);
 *  - constants as `#define TMF_NAME <integer>`; function-like macros are not exported.
 */
#ifndef TMF_HIP_H
#define TMF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMF_OK              0
#define TMF_E_NULL         -1   /* a required pointer is NULL */
#define TMF_E_SHAPE        -2   /* unsupported / inconsistent shape */
#define TMF_E_ALIGN        -3   /* pointer not 16-byte aligned */
#define TMF_E_WORKSPACE    -4   /* workspace smaller than *_workspace_bytes() */
#define TMF_E_ARG          -5   /* bad enum / scalar argument */

/* layout of a convolution weight gradient: tap-major dw[t][cin][cout] (the kernels' own weight layout) or the
 * reference's nn.Conv3d layout (Cout, Cin, k, k, k) = dw[cout][cin][t], written directly by the final reduction */
#define TMF_DW_TAPMAJOR  0
#define TMF_DW_REFERENCE 1

#define TMF_POOL_NONE 0
#define TMF_POOL_MAX2 1        /* MaxPool3d(2, stride=2), floor mode */
#define TMF_POOL_AVG2 2        /* AvgPool3d(2, stride=2), floor mode */

int         tmf_version(void);                 /* ABI version, currently 1 */
const char* tmf_last_error_string(void);
/* Process options: tmf_set_option(name, value) or, where listed, an environment variable read once on first use; a value set
 * wins over the environment.  0 on success; TMF_E_ARG for an unknown name or a value the option refuses (the table's "set").
 * Process-wide, safe to call from any thread; a launch plans with the values of the moment.  Each option chooses kernels only:
 * results stay equal up to fp32 summation order ("debug" aside).  Options marked "per call" are also carried by
 * tmf_snet_desc.flags (TMF_SNET_ALGO, below): such a call follows its own word, not the process option.
 *
 *  option       set                      environment (atoi)            default  per call  chooses
 *  conv_wino    0..3                     TMF_CONV_WINO: 0..2, else 3   3        yes       Winograd form for: 0 none, 1 data gradients,
 *                                                                                         2 + forward, 3 + weight gradients (tmf_conv_wino_mode)
 *  wino_p       any, non-zero -> 1       TMF_WINO_P: 0, else 1         1        yes       persistent Winograd kernels (tmf_wino_p_mode)
 *  wino_x       any, non-zero -> 1       TMF_WINO_X: 0, else 1         1        yes       Winograd as exact bf16 splits (tmf_wino_x_mode)
 *  c1_gram      <=0 -> 0, >=2 -> 2, 1    TMF_C1_GRAM: the same         1        yes       first block through its tap Gram matrix;
 *                                                                                         2 in the bf16 mode as well (tmf_c1_gram_bytes)
 *  c1_split     any, non-zero -> 1       TMF_C1_SPLIT: 0, else 1       1        yes       first block's z as exact bf16 splits (tmf_c1_split_mode)
 *  pool_recompute 0..3                   TMF_POOL_RECOMPUTE: 0..3,     0        yes       max-pool routing of the whole-encoder fp32 train path:
 *                                        else 0                                           0 kept by the forward, 1 recomputed in backward,
 *                                                                                         2 / 3 recomputed in block 0 / in blocks 2, 4 only
 *  wino_cus     >= 0; 0: the environment TMF_WINO_CUS                  0        no        n > 0 caps the persistent Winograd workgroups at
 *                                                                                         min(n, compute units); 0 the device's count
 *  conv_rt      0..2                     TMF_CONV_RT: 1, 2, else 0     0        no*       register-tiled fp32 forward / data-gradient
 *                                                                                         kernel: never / volumes <= 24^3 / wherever it fits
 *  conv_waves   2, 4, 8, 16              TMF_CONV_WAVES: 2, 4, 8,      16       no        workgroup shape of the direct convolutions
 *                                        else 16
 *  bf16_v2      0..2                     TMF_BF_V2: 0, 2, else 1       1        no        bf16 forward with 8x8x8 bricks: never / by brick
 *                                                                                         count / always (tmf_conv3d_bf16_stat_blocks follows)
 *  bf16_dma     0, 1                     -                             1        no        LDS-DMA form of that kernel (bf16 tensors)
 *  wgrad_tr     0..2                     -                             1        no        bf16 weight gradient with transposing LDS reads:
 *                                                                                         never / where faster / wherever cin, cout % 8 == 0
 *  debug        any                      -                             0        no        timing-ablation bits of the direct kernels, in bf16
 *                                                                                         only in -DTMF_ABLATE builds (results are garbage)
 *  (none)       -                        TMF_WINO_EVEN, TMF_WINOX_SWAP, TMF_BF_NT2, TMF_CONV_AUTO: 0 turns off (default on) an
 *                                        even persistent Winograd grid, the transposed split-kernel items, 64-channel bf16
 *                                        workgroups, the per-launch brick choice of the direct forward
 *  (none)       -                        TMF_C1_BLOCKS (default 1024; below 64 the default), TMF_C1_FWD_MULT (default 4):
 *                                        workgroups of the first block's slab passes / multiple of them for its forward
 *  * conv_rt: a call with TMF_SNET_ALONE asks for at least 1 for itself.
 * The kernel-name and size queries (tmf_conv3d_fwd_kernel_name, tmf_conv3d_stat_blocks, tmf_conv3d_wino_stat_blocks, ...)
 * follow the options of the moment: a buffer sized under one setting must not be launched under another.
 * Size limits of the convolution entries: one sample of a layer (D*H*W*max(cin, cout)) and one weight tensor stay below
 * 2^29 elements — offsets inside a sample are 32-bit byte offsets of buffer resources; violating shapes return TMF_E_SHAPE. */
int         tmf_set_option(const char* name, int value);

/* ------------------------------------------------------------------------------
 * 3-D convolution, stride 1, "same" zero padding, cross-correlation, NO bias
 * (a bias ahead of BatchNorm is folded into the BN shift / running mean by
 * tmf_bn_finalize).  Replaces F.conv3d at networks.py:22,28,31,37,40,46,49.
 *
 * ksize = 3 or 1.  fp32 in / fp32 accumulate on v_mfma_f32_32x32x2_f32 (exact fp32).
 * If `stat_partial` != NULL the kernel also writes per-workgroup partial sums
 * [nblk][2][cout] (sum z, sum z^2) for the BatchNorm statistics, nblk =
 * tmf_conv3d_stat_blocks(); reduce them with tmf_bn_finalize.
 * The data-gradient of the layer is the SAME entry called on dz with the weight
 * tensor flipped and transposed (w'[26-t][co][ci] = w[t][ci][co]).
 * ---------------------------------------------------------------------------- */
int  tmf_conv3d_fwd(const float* x, const float* w, float* z, float* stat_partial,
                    int B, int D, int H, int W, int cin, int cout, int ksize, void* stream);
int  tmf_conv3d_stat_blocks(int B, int D, int H, int W, int cin, int cout, int ksize);
/* Template-argument text ("FwdCfg<3, 16, 1, 1, 8, 1, 4, 8, 8, 3>" / "WgCfg<1, 4, 8, 8, 8, 32>") of the kernel instance
 * tmf_conv3d_fwd / tmf_conv3d_wgrad launch for a shape, as a kernel trace prints it (measurement aid: bench.py groups
 * its live launch timings by it).  Thread-local static storage; "?" for shapes without a kernel. */
const char* tmf_conv3d_fwd_kernel_name(int B, int D, int H, int W, int cin, int cout, int ksize);
const char* tmf_conv3d_wgrad_kernel_name(int B, int D, int H, int W, int cin, int cout, int ksize);
/* Eval-mode block in ONE pass (BatchNorm is affine in eval mode; val_step, kfold_train_adversarial.py:144-161):
 *   y = pool( LeakyReLU( scale[c] * conv(x)[c] + shift[c] ) ),   pool = TMF_POOL_NONE | MAX2 | AVG2 (floor mode),
 * scale / shift from tmf_bn_eval_coeffs (they absorb the conv bias).  The raw conv output is never written.
 * y: [B][D][H][W][cout] or [B][D/2][H/2][W/2][cout].  cin and cout must be multiples of 4.  Forward only. */
int  tmf_conv3d_fwd_affine(const float* x, const float* w, const float* scale, const float* shift, float* y,
                           int B, int D, int H, int W, int cin, int cout, int ksize, int pool, float slope, void* stream);

/* Weight gradient: dw[t][ci][co] = sum_{b,pos} x[b,pos+t-1][ci] * dz[b,pos][co].
 * Two stages: split-K partial slabs into `workspace`, then a deterministic reduce.
 * Replaces the weight half of aten::convolution_backward for the call sites above. */
size_t tmf_conv3d_wgrad_workspace_bytes(int B, int D, int H, int W, int cin, int cout, int ksize);
int    tmf_conv3d_wgrad(const float* x, const float* dz, float* dw, void* workspace, size_t workspace_bytes,
                        int B, int D, int H, int W, int cin, int cout, int ksize, int dw_layout, void* stream);

/* bf16 matrix-core variant (BASELINE configs[2]: "bf16 with MFMA 3D conv"), 3x3x3 only: fp32 tensors in HBM,
 * operands rounded to bf16 (RNE) on the way into LDS, v_mfma_f32_32x32x16_bf16 with fp32 accumulation, fp32
 * output and statistics.  w_bf16: bf16 [27][cout][cin] (cin contiguous); cin % 8 == 0.  The data gradient is the
 * same entry on dz with w'[26-t][ci][co] = w[t][co][ci].  stat_partial: [tmf_conv3d_bf16_stat_blocks()][2][cout]. */
int  tmf_conv3d_fwd_bf16(const float* x, const void* w_bf16, float* z, float* stat_partial,
                         int B, int D, int H, int W, int cin, int cout, void* stream);
int  tmf_conv3d_bf16_stat_blocks(int B, int D, int H, int W);
/* Weight gradient on the bf16 matrix cores (x and dz rounded to bf16 while staged, fp32 accumulation, fp32 dw
 * [27][cin][cout]); workspace as tmf_conv3d_wgrad. */
size_t tmf_conv3d_wgrad_bf16_workspace_bytes(int B, int D, int H, int W, int cin, int cout);
int    tmf_conv3d_wgrad_bf16(const float* x, const float* dz, float* dw, void* workspace, size_t workspace_bytes,
                             int B, int D, int H, int W, int cin, int cout, void* stream);
/* bf16 ACTIVATION STORAGE (configs[2]: "bf16 storage + bf16 MFMA with fp32 accumulate"): the same kernels reading /
 * writing bf16 tensors directly (no conversion in the staging path, half the bytes).  io bits for the forward: 1 = x is
 * bf16, 2 = z is bf16 (statistics still from the fp32 accumulators); for the weight gradient io = 1: x and dz are bf16. */
int    tmf_conv3d_fwd_bf16_t(const void* x, const void* w_bf16, void* z, float* stat_partial,
                             int B, int D, int H, int W, int cin, int cout, int io, void* stream);
const char* tmf_conv3d_fwd_bf16_kernel_name(int B, int D, int H, int W, int cin, int cout, int io);   /* as tmf_conv3d_fwd_kernel_name */
const char* tmf_conv3d_wgrad_bf16_kernel_name(int B, int D, int H, int W, int cin, int cout, int io); /* io: 1 = bf16 tensors */
/* The plan of that launch under the current "wgrad_tr" option (no device call): workgroups per channel block into *nsplit, the
 * bricks each of them walks into *tiles_per_split; returns the number of 4x8x8 bricks, 0 on bad arguments. */
int    tmf_conv3d_wgrad_bf16_plan(int B, int D, int H, int W, int cin, int cout, int io, int* nsplit, int* tiles_per_split);
int    tmf_conv3d_wgrad_bf16_t(const void* x, const void* dz, float* dw, void* workspace, size_t workspace_bytes,
                               int B, int D, int H, int W, int cin, int cout, int io, int dw_layout, void* stream);
/* fp32-ACCURATE variant on the bf16 matrix cores: operands split exactly into three bf16 numbers (hi+mid+lo), the
 * six partial products of order >= 2^-16 accumulated in fp32 (the dropped terms are below one fp32 ulp of the
 * product).  w3_bf16: bf16 [3 parts][27][cout][cin]; same shapes as tmf_conv3d_fwd_bf16; stat_partial:
 * [tmf_conv3d_split_stat_blocks()][2][cout]. */
int  tmf_conv3d_fwd_split(const float* x, const void* w3_bf16, float* z, float* stat_partial,
                          int B, int D, int H, int W, int cin, int cout, void* stream);
int  tmf_conv3d_split_stat_blocks(int B, int D, int H, int W);        /* rows of its stat_partial */
/* WINOGRAD form F(2x2x2, 3x3x3) of the same convolution (csrc/conv3d_wino.hip), exact-fp32 arithmetic on the fp32 matrix
 * pipe: 64 products per 2x2x2 output tile, input and output channel instead of 216.  Replaces aten::conv3d and the input
 * gradient of convolution_backward at networks.py:28,31,37,40,46 for layers with cin % 8 == 0 and cout % 32 == 0
 * (tmf_conv3d_wino_ok).  x [B][D][H][W][cin], z [B][D][H][W][cout] fp32 channels-last; u = the transformed weights from
 * tmf_pack_conv_weights_wino (forward: u_fwd; data gradient: the same entry called with dz, u_dgrad and the channel
 * counts swapped); stat_partial (may be NULL): [tmf_conv3d_wino_stat_blocks()][2][cout].  Results differ from the direct
 * kernels' by fp32 rounding only (about twice their distance to the fp64 value).
 * tmf_conv_wino_mode(): the option "conv_wino" (tmf_set_option) — which train-mode encoder blocks that qualify take this form. */
int    tmf_conv3d_fwd_wino(const float* x, const float* u, float* z, float* stat_partial,
                           int B, int D, int H, int W, int cin, int cout, void* stream);
int    tmf_conv3d_wino_ok(int cin, int cout);
/* ... and the eval-mode block in one pass (tmf_conv3d_fwd_affine's Winograd form, val_step: kfold_train_adversarial.py:144-161):
 * y = LeakyReLU(scale * conv(x, w) + shift), pool TMF_POOL_NONE | TMF_POOL_MAX2 (floor mode) applied before the store. */
int    tmf_conv3d_fwd_wino_affine(const float* x, const float* u, const float* scale, const float* shift, float* y,
                                  int B, int D, int H, int W, int cin, int cout, int pool, float slope, void* stream);
int    tmf_conv3d_wino_stat_blocks(int B, int D, int H, int W);       /* rows of stat_partial: one per workgroup of the persistent
                                                                       * kernel (= compute units; all rows are written), one per
                                                                       * 4x8x8 brick with "wino_p" 0 */
int    tmf_conv3d_wino_bricks(int B, int D, int H, int W);            /* bricks the forward kernel walks per 32 output channels */
int    tmf_conv3d_wino_bricks2(int B, int D, int H, int W, int cin, int cout);   /* ... of a launch with these channel counts: where the split
                                                                         kernel can take it, the one-sample bricks are kept unless the folded
                                                                         geometry saves more than 15 % of them (round 6) */
int    tmf_conv3d_wino_grid(int B, int D, int H, int W, int cin, int cout);      /* workgroups of that launch's first window (persistent
                                                                         kernels: min(items, CUs), evened to the rounds it needs);
                                                                         statistic rows at and past it are zeros; 0 with "wino_p" 0 */
int    tmf_xcd_slot(int block, int grid);                             /* the placement rule of the persistent Winograd kernels: the
                                                                       * window slot (forward / data gradient: items slot + i * grid)
                                                                       * or split (weight gradient) of workgroup `block`, which runs
                                                                       * on XCD block % 8 — a permutation of 0 .. grid - 1 that gives
                                                                       * every XCD one contiguous range, for every grid; -1 outside */
const char* tmf_conv3d_wino_kernel_name(int B, int D, int H, int W, int stats);        /* the instance a kernel trace shows (as */
const char* tmf_conv3d_wgrad_wino_kernel_name(int B, int D, int H, int W, int cin, int cout);   /* tmf_conv3d_fwd_kernel_name) */
long   tmf_conv3d_wgrad_wino_tiles(int B, int D, int H, int W, int cin, int cout);     /* 2x2x2 tiles (padded: 16 per stage) the weight-
                                                                       * gradient launch multiplies per channel pair */
const char* tmf_conv3d_wino_kernel_name2(int B, int D, int H, int W, int cin, int cout, int stats);   /* ... with the channel counts: the
                                                                       * split kernel conv3d_winox_kernel where it takes the launch */
size_t tmf_conv3d_wino_weight_bytes(int cin, int cout);             /* 64 * cin * cout floats + the same numbers as three bf16 parts
                                                                       * (6 bytes each) behind them */
/* tmf_wino_x_mode(): the option "wino_x" (tmf_set_option).  1: tmf_conv3d_fwd_wino (train forward and data gradient)
 * runs csrc/conv3d_winox.hip where cin % 32 == 0, cout % 32 == 0 and the volume takes 4x8x8 bricks: the SAME fp32 products, each
 * operand split exactly into three bf16 numbers (no rounding: 8 + 8 + 8 significand bits), six of the nine partial products on
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation — the dropped three are below 2^-24 of the product, under the rounding of the
 * fp32 product itself.  0: the fp32 matrix pipe (conv3d_wino_p_kernel) everywhere. */
int    tmf_wino_x_mode(void);
int    tmf_conv_wino_mode(void);
/* tmf_wino_p_mode(): the option "wino_p" (tmf_set_option).  1: the three Winograd entries run their persistent
 * one-wave-per-SIMD kernels (conv3d_wino_p_kernel, conv3d_wino_wgrad_p_kernel; the forward picks per volume between 4x8x8
 * bricks of one sample and 4x4x4 bricks of four samples — tmf_conv3d_wino_bricks() follows it); 0: the two-waves-per-
 * SIMD kernels of round 4.  Same results up to fp32 rounding of the output transform's order of additions. */
int    tmf_wino_p_mode(void);
/* The option "wino_cus" (tmf_set_option) — a test and experiment aid: with n > 0 every workgroup of the persistent Winograd forward /
 * data-gradient kernels walks many items and launches split into windows of n x (item table) items.  tmf_conv3d_wino_stat_blocks
 * follows it: a statistics buffer sized under one setting must not be launched under a larger one. */
/* Weight gradient in the same form: dU_p = V_p^T Z_p per position of the transformed tile (V = the forward's input transform of
 * x, Z = A dz A^T), summed over all tiles on the fp32 matrix pipe, then dw = G^T dU G (fp64) — replaces the weight gradient of
 * convolution_backward at networks.py:28,31,37,40,46 for cin % 32 == 0 and cout % 32 == 0.  Arguments as tmf_conv3d_wgrad. */
int    tmf_conv3d_wgrad_wino_ok(int cin, int cout);
size_t tmf_conv3d_wgrad_wino_workspace_bytes(int B, int D, int H, int W, int cin, int cout);
int    tmf_conv3d_wgrad_wino(const float* x, const float* dz, float* dw, void* workspace, size_t workspace_bytes,
                             int B, int D, int H, int W, int cin, int cout, int dw_layout, void* stream);

/* First layer, cin == 1 (networks.py:22): x[b][d][h][w], w[27][cout]. */
int    tmf_conv3d_c1_fwd(const float* x, const float* w, float* z, float* stat_partial,
                         int B, int D, int H, int W, int cout, void* stream);
int    tmf_conv3d_c1_stat_blocks(int B, int D, int H, int W, int cout);
size_t tmf_conv3d_c1_wgrad_workspace_bytes(int B, int D, int H, int W, int cout);
int    tmf_conv3d_c1_wgrad(const float* x, const float* dz, float* dw, void* workspace, size_t workspace_bytes,
                           int B, int D, int H, int W, int cout, int dw_layout, void* stream);

/* ------------------------------------------------------------------------------
 * Fused first block: Conv3d(1->C,3x3x3) -> BatchNorm3d -> LeakyReLU -> MaxPool3d(2) (networks.py:21-26)
 * without materialising the conv output: every pass recomputes it from x (28 MB) instead of
 * reading/writing the 906 MB tensor.  x[b][d][h][w], w[27][C], pooled/dpool [b][D/2][H/2][W/2][C].
 *   tmf_c1_stats        -> stat_partial [tmf_c1_blocks()][2][C]  (reduce with tmf_bn_finalize)
 *   tmf_c1_bn_pool_fwd  -> pooled
 *   tmf_c1_bwd_reduce   -> partial [tmf_c1_blocks()][2][C]       (reduce with tmf_bn_bwd_finalize)
 *   tmf_c1_bwd_wgrad    -> dw[27][C]   (coef from tmf_bn_bwd_finalize)
 *   tmf_c1_bwd_dgrad    -> dx[b][d][h][w] (coef from tmf_bn_bwd_finalize; all-zero coef = eval-mode BatchNorm; fp32 tensors)
 * ---------------------------------------------------------------------------- */
int    tmf_c1_blocks(int B, int D, int H, int W, int C);
int    tmf_c1_stats(const float* x, const float* w, float* stat_partial, int B, int D, int H, int W, int C, void* stream);
/* Round 5: the first block through the tap Gram matrix of its INPUT (csrc/conv1_gram.hip; the option "c1_gram" of tmf_set_option;
 * fp32).  tmf_c1_stats_g: the statistics WITHOUT a convolution pass and the exact 27 x 27 matrix
 * G[t][t'] = sum_v x~(v + t) x~(v + t') of the zero-padded volume (+ the 27 shifted sums S_t), from 63 offset pair sums of the
 * volume minus per-face-class sums over the one-voxel shell around it, all in fp64 —
 * gram: tmf_c1_gram_bytes() bytes (0: not available — option "c1_gram" off or C > 64), doubles [0,729) G, [729,756) S_t, 756 S, then
 * scratch; stat_partial rows 0 / 1 = the high / low float halves of sum z, sum z^2 (tmf_bn_finalize over 2 rows).  With G the
 * backward of the block is ONE pass over the
 * volume: tmf_c1_bwd_fused = tmf_c1_bwd_reduce + tmf_bn_bwd_finalize + tmf_c1_bwd_wgrad (train mode, fp32):
 *   dw[t][c] = scale_c [ D[t][c] - c0_c S_t - c1_c invstd_c (sum_t' w[t'][c] G[t][t'] - mean_c S_t) ],  D = sum_v x(v + t) dy_c(v)
 * (dy is one element per pooling window: 27 multiply-adds per window beside the BatchNorm sums).  workspace:
 * tmf_c1_bwd_fused_workspace_bytes(). */
size_t tmf_c1_gram_bytes(int B, int D, int H, int W, int C);
size_t tmf_c1_gram_bytes_bf16(int B, int D, int H, int W, int C);   /* what a bf16-mode caller asks: 0 unless "c1_gram" is 2 */
int    tmf_c1_stats_g(const float* x, const float* w, float* stat_partial, void* gram, size_t gram_bytes,
                      int B, int D, int H, int W, int C, void* stream);
size_t tmf_c1_bwd_fused_workspace_bytes(int B, int D, int H, int W, int C);
int    tmf_c1_bwd_fused(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const float* dpool, const void* gram, float* dw, float* dgamma, float* dbeta,
                        void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int C, float slope,
                        int dw_layout, void* stream);
/* Round 6: the same two entries for the bf16 mode (TMF_PREC_BF16; conv1_fused_kernel<.., true> multiplies the volume and the taps
 * ROUNDED to bf16): G, S_t of the rounded volume, forms in the rounded taps — the exact statistics of that kernel's z; the backward
 * pass accumulates D from the rounded volume and the unrounded dy (pooled_bf16: dpool is a bf16 tensor). */
int    tmf_c1_stats_g_bf16(const float* x, const float* w, float* stat_partial, void* gram, size_t gram_bytes,
                           int B, int D, int H, int W, int C, void* stream);
int    tmf_c1_bwd_fused_bf16(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const void* dpool, const void* gram, float* dw, float* dgamma, float* dbeta,
                             void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int C, float slope,
                             int pooled_bf16, int dw_layout, void* stream);
int    tmf_c1_bn_pool_fwd(const float* x, const float* w, const float* scale, const float* shift, float* pooled,
                          int B, int D, int H, int W, int C, float slope, void* stream);
/* The pool routing kept by the forward (fp32): tmf_c1_bn_pool_fwd_route also writes, per pooled window and channel, z_sel = the
 * conv output of the window's FIRST maximum of scale*z + shift (torch scan order) and arg = its index 4 d + 2 h + w — both
 * [b][D/2][H/2][W/2][C], float and byte; `pooled` is bit-identical to tmf_c1_bn_pool_fwd's.  tmf_c1_bwd_fused_route is
 * tmf_c1_bwd_fused reading them instead of evaluating z (x still feeds D): same workspace, bit-identical dw, dgamma, dbeta. */
int    tmf_c1_bn_pool_fwd_route(const float* x, const float* w, const float* scale, const float* shift, float* pooled,
                                float* z_sel, unsigned char* arg, int B, int D, int H, int W, int C, float slope, void* stream);
int    tmf_c1_bwd_fused_route(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                              const float* invstd, const float* dpool, const float* z_sel, const unsigned char* arg,
                              const void* gram, float* dw, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
                              int B, int D, int H, int W, int C, float slope, int dw_layout, void* stream);
/* tmf_c1_bwd_fused[_route] that also writes coef [2][C] for tmf_c1_bwd_dgrad (z_sel = arg = NULL: the recomputing form) */
int    tmf_c1_bwd_fused_coef(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                             const float* invstd, const float* dpool, const float* z_sel, const unsigned char* arg,
                             const void* gram, float* dw, float* dgamma, float* dbeta, float* coef, void* workspace,
                             size_t workspace_bytes, int B, int D, int H, int W, int C, float slope, int dw_layout, void* stream);
int    tmf_c1_bwd_reduce(const float* x, const float* w, const float* scale, const float* shift,
                         const float* mean, const float* invstd, const float* dpool, float* partial,
                         int B, int D, int H, int W, int C, float slope, void* stream);
size_t tmf_c1_bwd_wgrad_workspace_bytes(int B, int D, int H, int W, int C);
int    tmf_c1_bwd_wgrad(const float* x, const float* w, const float* scale, const float* shift,
                        const float* mean, const float* invstd, const float* coef, const float* dpool,
                        float* dw, void* workspace, size_t workspace_bytes,
                        int B, int D, int H, int W, int C, float slope, int dw_layout, void* stream);
/* Data gradient of the block (csrc/conv1_dgrad.hip): with dy the routed, LeakyReLU-masked dpool (first maximum of y, the
 * forward's routing bit for bit under the same "c1_split" setting) and dz_c = scale_c (dy_c - coef[0][c] - coef[1][c] invstd_c
 * (z_c - mean_c)) on EVERY voxel, dx(u) = sum_t sum_c w[t][c] dz_c(u - t + 1).  Nothing of size voxels x C touches memory; the
 * result is bit-reproducible.  Any D, H, W, C >= 1; an empty pooled tensor (dpool may then be NULL) leaves the BatchNorm part.
 * workspace: tmf_c1_bwd_dgrad_workspace_bytes() (a few KB of prepared stencil coefficients). */
size_t tmf_c1_bwd_dgrad_workspace_bytes(int B, int D, int H, int W, int C);
int    tmf_c1_bwd_dgrad(const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                        const float* invstd, const float* coef, const float* dpool, float* dx,
                        void* workspace, size_t workspace_bytes, int B, int D, int H, int W, int C, float slope, void* stream);
/* The same four passes with both products on the bf16 matrix cores (operands rounded to bf16, fp32 accumulation):
 * 2 MFMAs per tile instead of 14 / 16.  Same arguments, same workspace / block counts; pooled_bf16 != 0: the pooled
 * output / its gradient dpool are bf16 tensors (bf16 activation storage, BASELINE configs[2]). */
int    tmf_c1_stats_bf16(const float* x, const float* w, float* stat_partial, int B, int D, int H, int W, int C, void* stream);
int    tmf_c1_bn_pool_fwd_bf16(const float* x, const float* w, const float* scale, const float* shift, void* pooled,
                               int B, int D, int H, int W, int C, float slope, int pooled_bf16, void* stream);
int    tmf_c1_bwd_reduce_bf16(const float* x, const float* w, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const void* dpool, float* partial,
                              int B, int D, int H, int W, int C, float slope, int pooled_bf16, void* stream);
int    tmf_c1_bwd_wgrad_bf16(const float* x, const float* w, const float* scale, const float* shift,
                             const float* mean, const float* invstd, const float* coef, const void* dpool,
                             float* dw, void* workspace, size_t workspace_bytes,
                             int B, int D, int H, int W, int C, float slope, int pooled_bf16, int dw_layout, void* stream);

/* ------------------------------------------------------------------------------
 * BatchNorm3d (training statistics) + LeakyReLU + 2x2x2 pool, two passes.
 * Replaces F.batch_norm / leaky_relu / max_pool3d / avg_pool3d at
 * networks.py:23-25,29-30,32-34,38-39,41-43,47-48,50-52.
 * ---------------------------------------------------------------------------- */

/* Reduce the conv's partial sums -> per-channel mean / invstd / scale / shift and
 * update the running buffers (momentum, unbiased running_var, torch semantics).
 * conv_bias (may be NULL) is added to the mean that goes into running_mean.
 * count = B*D*H*W.  running_* may be NULL (no update). */
int tmf_bn_finalize(const float* stat_partial, int nblk, int C, double count,
                    const float* gamma, const float* beta, const float* conv_bias,
                    float* running_mean, float* running_var, float momentum, float eps,
                    float* mean, float* invstd, float* scale, float* shift, void* stream);

/* Eval mode: scale/shift from the running statistics (and the folded conv bias). */
int tmf_bn_eval_coeffs(const float* gamma, const float* beta, const float* conv_bias,
                       const float* running_mean, const float* running_var, float eps, int C,
                       float* scale, float* shift, void* stream);

/* out = pool(leaky_relu(z*scale + shift, slope)); out dims are floor(D/2).. for pools. */
int tmf_bn_act_pool_fwd(const float* z, const float* scale, const float* shift, float* out,
                        int B, int D, int H, int W, int C, int pool, float slope, void* stream);

/* Backward pass 1: per-workgroup partials [nblk][2][C] of sum(dy) and sum(dy*xhat),
 * dy = d(loss)/d(BN output) obtained from `dout` through pool and LeakyReLU. */
int tmf_bn_act_pool_bwd_blocks(int B, int D, int H, int W, int C, int pool);
int tmf_bn_act_pool_bwd_reduce(const float* z, const float* dout, const float* scale, const float* shift,
                               const float* mean, const float* invstd, float* partial,
                               int B, int D, int H, int W, int C, int pool, float slope, void* stream);
/* Reduce partials -> dgamma, dbeta and the two per-channel constants the apply pass needs
 * (coef[0][c] = sum(dy)/count, coef[1][c] = sum(dy*xhat)/count). */
int tmf_bn_bwd_finalize(const float* partial, int nblk, int C, double count,
                        float* dgamma, float* dbeta, float* coef, void* stream);
/* Backward pass 2: dz = scale * (dy - coef0 - xhat*coef1). */
int tmf_bn_act_pool_bwd_apply(const float* z, const float* dout, const float* scale, const float* shift,
                              const float* mean, const float* invstd, const float* coef, float* dz,
                              int B, int D, int H, int W, int C, int pool, float slope, void* stream);

/* The three passes on typed tensors.  io bit 0: z and dz are bf16 tensors; bit 1: out and dout are bf16 tensors
 * (io = 0 all float, 1 = bf16 z with a float output (the block feeding the fp32 1x1x1 layer), 3 = all bf16).  Arithmetic,
 * per-channel vectors and partials are fp32 in every mode. */
int tmf_bn_act_pool_fwd_t(const void* z, const float* scale, const float* shift, void* out,
                          int B, int D, int H, int W, int C, int pool, float slope, int io, void* stream);
int tmf_bn_act_pool_bwd_reduce_t(const void* z, const void* dout, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, float* partial,
                                 int B, int D, int H, int W, int C, int pool, float slope, int io, void* stream);
int tmf_bn_act_pool_bwd_apply_t(const void* z, const void* dout, const float* scale, const float* shift,
                                const float* mean, const float* invstd, const float* coef, void* dz,
                                int B, int D, int H, int W, int C, int pool, float slope, int io, void* stream);

/* Max pool, all float, with the routing kept: tmf_bn_act_pool_fwd_route is tmf_bn_act_pool_fwd(.., TMF_POOL_MAX2, ..) that also
 * writes z_sel [b][D/2][H/2][W/2][C], the z of each window's first maximum of z*scale + shift (`out` bit-identical);
 * tmf_bn_act_pool_bwd_reduce_route reads (z_sel, dout) instead of (z, dout) — a ninth of the bytes — and writes the partials of
 * tmf_bn_act_pool_bwd_reduce bit for bit (same tmf_bn_act_pool_bwd_blocks).  The apply pass still needs z. */
int tmf_bn_act_pool_fwd_route(const float* z, const float* scale, const float* shift, float* out, float* z_sel,
                              int B, int D, int H, int W, int C, float slope, void* stream);
int tmf_bn_act_pool_bwd_reduce_route(const float* z_sel, const float* dout, const float* scale, const float* shift,
                                     const float* mean, const float* invstd, float* partial,
                                     int B, int D, int H, int W, int C, float slope, void* stream);

/* Sum `nblk` partial rows of `ncol` floats (fp64 accumulation) into out[ncol]. */
int tmf_colsum_finalize(const float* partial, int nblk, int ncol, float* out, void* stream);

/* ------------------------------------------------------------------------------
 * Fused multi-head cross attention:  out = softmax(q k^T * scale) v
 * (networks.py:169-173: einsum -> softmax -> einsum, plus the two rearranges).
 * q: [B][N][*] rows of stride q_stride floats, head h at columns [h*dh, (h+1)*dh);
 * k, v: [B][M][*] rows of stride kv_stride (so they can alias the to_kv output);
 * out: [B][N][heads*dh] ('b n (h d)'); lse: [B][heads][N] log-sum-exp (saved for bwd).
 * dh must be 8, 16, 32 or 64.
 * ---------------------------------------------------------------------------- */
int tmf_xattn_fwd(const float* q, const float* k, const float* v, float* out, float* lse,
                  int B, int heads, int N, int M, int dh, int q_stride, int kv_stride, float scale,
                  void* stream);
/* dq: [B][N][heads*dh] (stride heads*dh); dk, dv: rows of stride dkv_stride. */
int tmf_xattn_bwd(const float* q, const float* k, const float* v, const float* out, const float* lse,
                  const float* dout, float* dq, float* dk, float* dv,
                  int B, int heads, int N, int M, int dh, int q_stride, int kv_stride, int dkv_stride,
                  float scale, void* stream);
/* Two-part context (CrossTransformer, networks.py:250-251: keys / values over torch.cat([mri, pet], 1)): context row j
 * of batch b is row j of k1 / v1 ([B][M1][*]) when j < M1, else row j - M1 of k2 / v2 ([B][M2][*]); no concatenated copy
 * is built.  dk1 / dv1 and dk2 / dv2 receive the two parts' gradients in the same layouts (rows of stride dkv_stride).
 * Otherwise as tmf_xattn_fwd / _bwd with M = M1 + M2; M1, M2 > 0. */
int tmf_xattn_fwd_cat(const float* q, const float* k1, const float* v1, const float* k2, const float* v2, float* out,
                      float* lse, int B, int heads, int N, int M1, int M2, int dh, int q_stride, int kv_stride, float scale,
                      void* stream);
int tmf_xattn_bwd_cat(const float* q, const float* k1, const float* v1, const float* k2, const float* v2, const float* out,
                      const float* lse, const float* dout, float* dq, float* dk1, float* dv1, float* dk2, float* dv2,
                      int B, int heads, int N, int M1, int M2, int dh, int q_stride, int kv_stride, int dkv_stride,
                      float scale, void* stream);
/* P = softmax(q k^T scale) rebuilt from the lse that tmf_xattn_fwd / _fwd_cat wrote (base 2).
 * probs: [B][heads][N][M1+M2] or NULL; recv: [B][heads][M1+M2] = mean over queries of P, or NULL;
 * at least one non-NULL.  k2 may be NULL when M2 == 0.  dh 8, 16, 32 or 64.  No atomics: two calls give the same bits. */
int tmf_xattn_probs(const float* q, const float* k1, const float* k2, const float* lse,
                    float* probs, float* recv, int B, int heads, int N, int M1, int M2, int dh,
                    int q_stride, int kv_stride, float scale, void* stream);

/* ------------------------------------------------------------------------------
 * LayerNorm over the last dim (networks.py:117,219) and the token pooling of
 * CrossTransformer_MOD_AVG.forward (networks.py:276-281).
 * ---------------------------------------------------------------------------- */
/* y = LayerNorm(x) * gamma + beta (+ residual, [rows][dim], may be NULL: the "+ tokens" of networks.py:262-263). */
int tmf_layernorm_fwd(const float* x, const float* gamma, const float* beta, const float* residual, float* y,
                      float* mean, float* rstd, int rows, int dim, float eps, void* stream);
int tmf_layernorm_bwd_blocks(int rows, int dim);
/* partial: [nblk][2][dim] (dgamma, dbeta partials; reduce with tmf_colsum_finalize, ncol = 2*dim).
 * Shares its implementation with tmf_layernorm_bwd_masked below: this entry is that one without a mask. */
int tmf_layernorm_bwd(const float* x, const float* gamma, const float* mean, const float* rstd,
                      const float* dy, float* dx, float* partial, int rows, int dim, void* stream);
/* The same, and also dx_masked = dx * mask (mask [rows][dim]: a Dropout keep-mask already scaled by 1 / (1 - p)) in the
 * same pass: the block-final LayerNorm's input gradient and its m_f-masked copy (networks.py:133).  One implementation
 * serves both entries (same checks, same launch geometry); the _masked form adds: mask and dx_masked, both required,
 * and the <VEC, true> kernel instances. */
int tmf_layernorm_bwd_masked(const float* x, const float* gamma, const float* mean, const float* rstd,
                             const float* dy, float* dx, float* partial, int rows, int dim,
                             const float* mask, float* dx_masked, void* stream);
/* y = x * mask over n floats (16-byte aligned): a keep-mask applied to a gradient no other entry produces. */
int tmf_mask_mul(const float* x, const float* mask, float* y, long n, void* stream);

/* ------------------------------------------------------------------------------
 * Linear layers of the fusion transformer fused with their neighbours (token_gemm.hip): one launch per
 * nn.Linear, 16-row token tiles, exact-fp32 MFMA.  Replaces, per Transformer block, F.layer_norm + F.linear
 * (networks.py:117-121 with 158-159, 219), to_out + bias + residual (:160-163, 226), Linear + GELU + Linear +
 * residual (:131-141, 227), and the matching backward passes.
 *
 * forward:  y = [GELU]( LayerNorm?(x) . w^T + bias ) + residual
 *   x [R][K], w [Nout][K] (nn.Linear layout), y [R][Nout]; K % 16 == 0, Nout % 64 == 0.
 *   ln_gamma != NULL: LayerNorm over K first (K must be 64, 128 or 256); writes ln_mean / ln_rstd [R] and, when
 *   ln_out != NULL, the normalised rows [R][K].  bias [Nout] and residual [R][Nout] may be NULL.
 *   gelu_pre != NULL: gelu_pre = (..) . w^T + bias and y = GELU(gelu_pre) (erf form); no residual then.
 * backward (input gradient):  dx = E( dy . w ),  dy [R][Nout], w [Nout][K], dx [R][K]; Nout % 16 == 0, K % 64 == 0.
 *   gelu_pre != NULL: E(v) = v * GELU'(gelu_pre), gelu_pre [R][K].
 *   ln_x != NULL (K of 64, 128 or 256): E(v) = LayerNormBackward(v; ln_x, ln_mean, ln_rstd, ln_gamma) + add1 + add2,
 *   and the row-block partials of dgamma / dbeta go to ln_partial[blk * partial_stride + {0..K-1 | K..2K-1}].
 *   otherwise E(v) = v + add1.   add1 / add2 [R][K] may be NULL.
 *   bias_partial != NULL: column sums of the block's dy rows -> bias_partial[blk * partial_stride + c], c < Nout.
 *   blk < tmf_tok_row_blocks(R); reduce the partials with tmf_colsum_finalize(partial, nblk, partial_stride, ..).
 * tmf_tok_linear_fwd and tmf_tok_linear_bwd_input each share ONE implementation with their _masked (Dropout) form
 * below: they are that implementation without a mask, and run the plain epilogue instances.
 * ---------------------------------------------------------------------------- */
int tmf_tok_row_blocks(int R);
int tmf_tok_linear_fwd(const float* x, const float* w, const float* bias, const float* residual, float* y,
                       int R, int K, int Nout, const float* ln_gamma, const float* ln_beta, float eps,
                       float* ln_mean, float* ln_rstd, float* ln_out, float* gelu_pre, void* stream);
int tmf_tok_linear_bwd_input(const float* dy, const float* w, float* dx, int R, int Nout, int K,
                             const float* gelu_pre, const float* ln_x, const float* ln_mean, const float* ln_rstd,
                             const float* ln_gamma, const float* add1, const float* add2, float* ln_partial,
                             float* bias_partial, int partial_stride, void* stream);
/* Dropout forms (networks.py:131,133,153); mask: a keep-mask already scaled by 1 / (1 - p), never NULL.  Each is one
 * implementation with its plain entry above: the same argument checks in the same order (messages carry the called entry's
 * name), tiles and instance rule; the _masked form adds the mask, the *_MASK epilogue instances and, in backward, the rules
 * below — the plain backward also takes neither epilogue (dx = dy . w + add1, add2 then refused) and ignores add1 / add2
 * beside gelu_pre.
 * forward:  y = (..) . w^T + bias,  then  y = y * mask [+ residual]   or, gelu_pre != NULL,  y = GELU(gelu_pre) * mask
 *   (gelu_pre itself unmasked); mask [R][Nout].
 * backward (mask [R][K]): exactly one of
 *   gelu_pre != NULL: dx = (dy . w) * mask * GELU'(gelu_pre)   (no add1 / add2 / dx_masked);
 *   ln_x != NULL:     dx as in tmf_tok_linear_bwd_input's LayerNorm-backward epilogue, and dx_masked = dx * mask. */
int tmf_tok_linear_fwd_masked(const float* x, const float* w, const float* bias, const float* residual, float* y,
                              int R, int K, int Nout, const float* ln_gamma, const float* ln_beta, float eps,
                              float* ln_mean, float* ln_rstd, float* ln_out, float* gelu_pre, const float* mask, void* stream);
int tmf_tok_linear_bwd_input_masked(const float* dy, const float* w, float* dx, int R, int Nout, int K,
                                    const float* gelu_pre, const float* ln_x, const float* ln_mean, const float* ln_rstd,
                                    const float* ln_gamma, const float* add1, const float* add2, float* ln_partial,
                                    float* bias_partial, int partial_stride, const float* mask, float* dx_masked,
                                    void* stream);

/* Conv weights from the reference layout (Cout, Cin, k, k, k) of nn.Conv3d (networks.py:22,28,31,37,40,46,49;
 * taps = k^3 = 1 | 27) into the forward / weight-gradient
 * layout w_fwd[t][ci][co] and, when w_dgrad != NULL, the data-gradient layout w_dgrad[taps-1-t][co][ci], in one launch
 * (what the host side otherwise does with permute / flip copies on every step).  w_fwd may be NULL when only the
 * data-gradient layout is wanted (the forward runs in the Winograd form). */
int tmf_pack_conv_weights(const float* w, float* w_fwd, float* w_dgrad, int cout, int cin, int taps, void* stream);
/* The same for the bf16 matrix-core kernels: w_fwd_bf16[t][co][ci] = bf16(w[co][ci][t]) (the layout tmf_conv3d_fwd_bf16
 * reads) and, when w_dgrad_bf16 != NULL, w_dgrad_bf16[taps-1-t][ci][co] (its data-gradient call).  RNE rounding,
 * bit-identical to torch's .to(bfloat16).  cin (and cout, with a dgrad copy) even. */
int tmf_pack_conv_weights_bf16(const float* w, void* w_fwd_bf16, void* w_dgrad_bf16, int cout, int cin, int taps, void* stream);
/* The same for tmf_conv3d_fwd_split (the fp32x mode): every weight as its EXACT three-way bf16 decomposition,
 * w3_fwd[p][t][co][ci] = part p (hi, mid, lo) of w[co][ci][t] and, when w3_dgrad != NULL, w3_dgrad[p][taps-1-t][ci][co];
 * 3 * taps * cout * cin bf16 numbers each — the operand layout torch's split3 (.to(bfloat16), subtract, repeat) gives. */
int tmf_pack_conv_weights_split3(const float* w, void* w3_fwd, void* w3_dgrad, int cout, int cin, int taps, void* stream);
/* The same for tmf_conv3d_fwd_wino: U = G g G^T along the three axes of every 3x3x3 filter (fp64 inside, rounded once),
 * u_fwd[p][cin / 8][2][cout][4] (position p = (pd, ph, pw) of the 4x4x4 transformed tile; input channel 8 g + 4 hs + s) and
 * u_dgrad[p][cout / 8][2][cin][4] (the flipped filter with the channel roles swapped).  Either may be NULL; the forward
 * form needs tmf_conv3d_wino_ok(cin, cout), the data-gradient form tmf_conv3d_wino_ok(cout, cin). */
int tmf_pack_conv_weights_wino(const float* w, float* u_fwd, float* u_dgrad, int cout, int cin, void* stream);
/* ... the same for up to 8 layers in one launch (an encoder's Winograd blocks: one launch per forward instead of one per block) */
int tmf_pack_conv_weights_wino_multi(int n, const float* const* w, float* const* u_fwd, float* const* u_dgrad,
                                     const int* cout, const int* cin, void* stream);

/* Layout conversion between the reference's NCDHW tensors and the channels-last tensors every kernel here uses
 * (voxels = D*H*W).  The model itself never needs it — its input has C == 1 (same bytes either way) and its output
 * is handed back as a strided view — it is here for callers that feed or read intermediate activations. */
int tmf_layout_ncdhw_to_ndhwc(const float* src, float* dst, int B, int C, long voxels, void* stream);
int tmf_layout_ndhwc_to_ncdhw(const float* src, float* dst, int B, int C, long voxels, void* stream);

/* Weight gradients of up to 32 Linears in one launch (the backward of to_q / to_kv / to_out, networks.py:149-155, and of
 * the two FeedForward Linears, :129-132): dw[p][n][k] = sum_r dy[p][r][n] * x[p][r][k]
 * (dy[p]: [R[p]][N[p]], x[p]: [R[p]][K[p]], dw[p]: [N[p]][K[p]] = nn.Linear.weight layout; N, K multiples of 32).
 * dy / x / dw are HOST arrays of device pointers, R / N / K host arrays.  Split over 8 row ranges into `workspace`,
 * then summed in fixed order (deterministic). */
size_t tmf_tok_wgrad_multi_workspace_bytes(int nprob, const int* N, const int* K);
int    tmf_tok_wgrad_multi(int nprob, const float* const* dy, const float* const* x, float* const* dw,
                           const int* R, const int* N, const int* K, void* workspace, size_t workspace_bytes, void* stream);

/* cls[b] = [mean_n mri | mean_n pet | max_n mri | max_n pet]  (4*dim); argmax: int32 [B][2][dim]. */
int tmf_token_pool_fwd(const float* mri, const float* pet, float* cls, int32_t* argmax,
                       int B, int N, int dim, void* stream);
int tmf_token_pool_bwd(const float* dcls, const int32_t* argmax, float* dmri, float* dpet,
                       int B, int N, int dim, void* stream);

/* ------------------------------------------------------------------------------
 * Input pipeline step ahead of the path, on the device (csrc/input_pipeline.hip).  Replaces MONAI's ScaleIntensityd and
 * RandFlipd(spatial_axis=0) of datasets/ADNI.py:64-66 (host, num_workers=0) for volumes already copied to the device
 * (kfold_train_adversarial.py:106-108).  Exact fp32 formulas (bit-identical to the numpy restatement in
 * oracle/input_oracle.py):  minmax[b] = (min, max) of volume b;  dst = (src - min) / (max - min)  (a constant volume
 * gives zeros, as monai.transforms.utils.rescale_array);  flip_d[b] != 0 reverses the first spatial axis of volume b
 * (the random decision itself stays with the caller: MONAI draws it from its own RandomState).  vol / src / dst:
 * [B][D][H][W] fp32;  workspace >= tmf_scale_intensity_workspace_bytes(B).
 * ---------------------------------------------------------------------------- */
size_t tmf_scale_intensity_workspace_bytes(int B);
/* RandRotated(range_x=0.05, prob=0.3) / RandZoomd(min_zoom=0.95, max_zoom=1, prob=0.3) of datasets/ADNI.py:67-68 with the
 * random decisions as inputs: dst[b] = Rotate(angle about the first spatial axis; bilinear, border padding, keep_size)
 * of src[b] where do_rot[b] != 0 (cos_sin[b] = {cos, sin} of the angle in fp32), a copy otherwise;  dst[b] = Zoom(mode
 * "area", edge padding, keep_size) to out_size[b] = {floor(D z), floor(H z), floor(W z)} (1 <= out <= size) where
 * do_zoom[b] != 0, a copy otherwise.  Bit-identical to oracle/input_oracle.py rotate_x / zoom_area.  Not in place. */
int    tmf_rotate_x(const float* src, float* dst, const float* cos_sin, const unsigned char* do_rot,
                    int B, int D, int H, int W, void* stream);
int    tmf_zoom_area(const float* src, float* dst, const int* out_size, const unsigned char* do_zoom,
                     int B, int D, int H, int W, void* stream);
int    tmf_volume_minmax(const float* vol, float* minmax, void* workspace, size_t workspace_bytes, int B, long voxels,
                         void* stream);
int    tmf_scale_flip(const float* src, float* dst, const float* minmax, const unsigned char* flip_d,
                      int B, int D, int H, int W, void* stream);

/* Device-resident data set: one launch writes a whole training batch of both modalities from stores that stay in HBM for
 * the run.  Replaces the reference's per-batch host pipeline — the CacheDataset of datasets/__init__.py:12-29 and the
 * DataLoader(num_workers=0) of :56 over the MONAI transforms of datasets/ADNI.py:59-84, built per fold in
 * kfold_train_adversarial.py:60-66, and the `batch['MRI'].to(device)` copies of :106-108 — with the device as the cache:
 * store_mri / store_pet [N][D][H][W] fp32 hold every subject AFTER ScaleIntensity (the deterministic part of the transform:
 * tmf_volume_minmax + tmf_scale_flip without a flip, once per run), labels [N] int64.  For sample b of the batch and both
 * modalities
 *     out[b] = zoom_area( rotate_x( flip_d( store[decisions[b].index] ) ) ),   out_label[b] = labels[decisions[b].index],
 * every stage only where the record applies it, with the formulas — the same fp32 operations in the same order — of
 * tmf_scale_flip's flip, tmf_rotate_x and tmf_zoom_area: BIT-identical to those three calls in sequence on the gathered
 * volumes (and so to oracle/input_oracle.py train_transform), without their intermediate tensors.  out_mri / out_pet
 * [B][D][H][W] fp32, out_label [B] int64; decisions: DEVICE array of B records (the random draws stay with the caller, as
 * above).  2 B <= 65535, D <= 65535; the outputs may not overlap the stores or each other.
 * PRECONDITION (the records live on the device, the entry cannot see them): 0 <= index < N, and with od != 0 each of od /
 * oh / ow in [1, D] / [1, H] / [1, W].  The kernel does not rely on it: a record outside these ranges reads nothing and
 * yields a NaN volume pair and label -1. */
typedef struct tmf_augment_decision {      /* 32 bytes */
    int32_t index;                         /* subject: row of the stores and of labels */
    int32_t flip;                          /* != 0: reverse the first spatial axis (RandFlipd(spatial_axis=0)) */
    int32_t do_rot;                        /* != 0: rotate about the first spatial axis by the angle of (cos_a, sin_a) */
    float   cos_a, sin_a;                  /* cos / sin of the angle, rounded to fp32 on the host (as tmf_rotate_x's cos_sin) */
    int32_t od, oh, ow;                    /* zoomed size floor(S z) per axis (as tmf_zoom_area's out_size); od == 0: no zoom */
} tmf_augment_decision;
int    tmf_batch_augment(const float* store_mri, const float* store_pet, const int64_t* labels,
                         const tmf_augment_decision* decisions, float* out_mri, float* out_pet, int64_t* out_label,
                         int N, int B, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------
 * Whole-encoder entries (csrc/snet_path.hip): ONE call enqueues every launch of an sNet train-mode forward, or of its
 * backward.  Replaces, per modality, `self.mri_cnn(mri)` / `self.pet_cnn(pet)` (models/mymodel.py:206-207 ->
 * networks.py:55-61) and the matching slice of `all_loss.backward()` (kfold_train_adversarial.py:131-132).  Same kernels,
 * same order and arguments as calling the per-block entries above one by one — bit-identical results — but the host
 * side of a pass is one call instead of ~100, and every intermediate tensor lives in ONE caller-allocated workspace.
 *
 * Network: channels 1 -> dim/4 -> dim/4 -> dim/2 -> dim/2 -> dim -> 2*dim -> dim, 3x3x3 except the last (1x1x1), max
 * pools after blocks 0, 2, 4 and an average pool after block 6 (TMF_SNET_BLOCKS = 7 blocks).  dim % 32 == 0, every
 * volume edge >= 16.  precision: TMF_PREC_FP32 (exact fp32 MFMA) or TMF_PREC_BF16 (operands rounded to bf16, fp32
 * accumulation; storage_bf16 != 0 keeps the activations between the 3x3x3 blocks as bf16 tensors).
 *
 * Parameters are the reference's state_dict tensors as they are: weight[l] (Cout, Cin, k, k, k), bias[l] (may be NULL),
 * gamma / beta = BatchNorm3d weight / bias, running_mean / running_var (updated in place, torch semantics; may be NULL).
 *   tmf_snet_train_fwd : vol [B][D][H][W] fp32 -> out [B][D/16][H/16][W/16][dim] fp32 (channels-last); `saved`
 *                        (>= tmf_snet_saved_bytes) receives everything backward needs and must stay untouched until then.
 *   tmf_snet_train_bwd : dout (same shape as out) -> gradients written into g: dweight[l] in the nn.Conv3d layout,
 *                        dbias[l] (exact zeros: a bias ahead of batch-statistics BatchNorm), dgamma[l], dbeta[l].  NULL
 *                        dweight / dbias entries are skipped.  `scratch` >= tmf_snet_bwd_scratch_bytes, free afterwards.
 *   tmf_snet_train_bwd_input : tmf_snet_train_bwd plus dvol [B][D][H][W], the gradient for vol (saliency, input-gradient
 *                        regularisers; training itself needs none: kfold_train_adversarial.py:106-107).  Block 0 then also runs
 *                        tmf_c1_bwd_dgrad on block 1's data gradient; fp32 and fp32x precisions (bf16: TMF_E_ARG).  dvol = NULL is
 *                        tmf_snet_train_bwd, launch for launch.  Same scratch (tmf_snet_bwd_scratch_bytes covers both).
 * ---------------------------------------------------------------------------- */
#define TMF_SNET_BLOCKS 7
#define TMF_PREC_FP32 0
#define TMF_PREC_BF16 1
#define TMF_PREC_FP32X 2          /* fp32-accurate forward / data gradient on the bf16 matrix cores (exact 3-way bf16 split of both
                                     operands, six partial products: tmf_conv3d_fwd_split); first block, 1x1x1 layer and weight
                                     gradients exact fp32 */
/* tmf_snet_desc.flags.  TMF_SNET_ALONE: the caller runs this encoder with nothing beside it on the device, so the partial
 * workgroup rounds of the pooled layers are not filled by a second stream: the fp32 forward / data-gradient convolutions
 * of those layers take the register-tiled kernel (as tmf_set_option("conv_rt", 1) would, for this call only; same results
 * up to fp32 summation order).  model_single at B = 16: 13.72 -> 13.51 ms per step. */
#define TMF_SNET_ALONE 1
/* The ALGORITHM of a call travels in its descriptor (round 6): with TMF_SNET_ALGO set, the fields below decide which kernels the
 * call's fp32 convolutions take — for this call only, whatever tmf_set_option says, so that two models with different settings
 * live in one process and a forward / backward pair cannot disagree about the plan of the `saved` workspace (the backward gets
 * the descriptor of its forward).  Without the bit the process options (tmf_set_option / TMF_* environment) are the default.
 * tmf_snet_algo_flags() encodes the process options of the moment into such a word (the Python binding pins them at forward). */
#define TMF_SNET_ALGO          0x100
#define TMF_SNET_ALGO_WINO(m)  (((m) & 3) << 9)   /* conv_wino: 0 direct kernels .. 3 forward, data and weight gradients in the Winograd form */
#define TMF_SNET_ALGO_WINO_P   0x800              /* wino_p: the persistent one-wave-per-SIMD Winograd kernels */
#define TMF_SNET_ALGO_WINO_X   0x1000             /* wino_x: forward / data gradient as exact 3-way bf16 splits (conv3d_winox.hip) */
#define TMF_SNET_ALGO_C1_GRAM  0x2000             /* c1_gram: the first block through the tap Gram matrix of its input */
#define TMF_SNET_ALGO_C1_GRAM_BF16 0x4000         /* c1_gram 2: in the bf16 mode as well (off by default: slower there) */
#define TMF_SNET_ALGO_C1_SPLIT 0x8000             /* c1_split: z of the first block (fp32) as exact 3-way bf16 splits on the bf16 pipe */
/* pool_recompute: the fp32 train passes RECOMPUTE the max-pool routing in backward instead of reading what the forward kept in
 * `saved` (z of each window's maximum, + its index in block 0) — in the first block / in the pooled BatchNorm blocks (2, 4).
 * Both clear by default: the routing is kept (tmf_snet_saved_bytes counts it); results are bit-identical either way. */
#define TMF_SNET_ALGO_POOL_REC_C1 0x10000
#define TMF_SNET_ALGO_POOL_REC_BN 0x20000
int  tmf_snet_algo_flags(void);
int  tmf_c1_split_mode(void);                     /* the option "c1_split" (tmf_set_option) */
/* The kernel family of one encoder block (Conv3d(cin -> cout, ksize) ahead of BatchNorm) per direction, under the options of the
 * moment ("conv_wino"; inside a call with TMF_SNET_ALGO that call's word): forward in bits 0-3, data gradient in bits 4-7,
 * weight gradient in bits 8-11, each a TMF_CONV_* code.  The ONE rule: the whole-encoder entries plan with it and the Python
 * binding's block-by-block path asks it, so the two run the same kernels.
 *   TMF_PREC_BF16,  ksize 3, cin > 1, cin % 8 == 0: forward and weight gradient BF16; data gradient BF16 when cout % 8 == 0;
 *   TMF_PREC_FP32X, the same condition:             forward SPLIT; data gradient SPLIT when cout % 8 == 0; weight gradient direct;
 *   TMF_PREC_FP32,  ksize 3, cin > 1:               forward WINO at conv_wino >= 2 with tmf_conv3d_wino_ok(cin, cout), data gradient
 *                                                   WINO at >= 1 with tmf_conv3d_wino_ok(cout, cin), weight gradient WINO at >= 3
 *                                                   with tmf_conv3d_wgrad_wino_ok(cin, cout);
 * everything else TMF_CONV_DIRECT (the first block, cin == 1, has its fused passes: tmf_c1_*).  -1: unknown precision. */
#define TMF_CONV_DIRECT 0         /* exact fp32 MFMA, direct form (tmf_conv3d_fwd / tmf_conv3d_wgrad) */
#define TMF_CONV_WINO   1         /* Winograd form (tmf_conv3d_fwd_wino / tmf_conv3d_wgrad_wino) */
#define TMF_CONV_BF16   2         /* operands rounded to bf16 (tmf_conv3d_fwd_bf16_t / tmf_conv3d_wgrad_bf16_t) */
#define TMF_CONV_SPLIT  3         /* exact 3-way bf16 split (tmf_conv3d_fwd_split) */
int  tmf_conv_block_algo(int precision, int cin, int cout, int ksize);
typedef struct tmf_snet_desc {
    int   B, D, H, W;                /* input volumes (B, 1, D, H, W) */
    int   dim;                       /* sNet(dim) */
    int   precision;                 /* TMF_PREC_* */
    int   storage_bf16;              /* bf16 activation storage between the 3x3x3 blocks (TMF_PREC_BF16 only) */
    float momentum[TMF_SNET_BLOCKS]; /* BatchNorm3d.momentum, .eps and LeakyReLU.negative_slope per block */
    float eps[TMF_SNET_BLOCKS];
    float slope[TMF_SNET_BLOCKS];
    int   flags;                     /* TMF_SNET_ALONE: no other encoder runs beside this one (model_single, TMF_STREAMS=1);
                                      * TMF_SNET_ALGO | ...: this call's algorithm choice (above) */
} tmf_snet_desc;
typedef struct tmf_snet_params {
    const float* weight[TMF_SNET_BLOCKS];
    const float* bias[TMF_SNET_BLOCKS];
    const float* gamma[TMF_SNET_BLOCKS];
    const float* beta[TMF_SNET_BLOCKS];
    float*       running_mean[TMF_SNET_BLOCKS];
    float*       running_var[TMF_SNET_BLOCKS];
} tmf_snet_params;
/* deep_event (optional, a hipEvent_t): recorded on `stream` as soon as every gradient of blocks TMF_SNET_DEEP_FROM .. 6
 * (conv3.0 .. conv4.3: 95 % of an encoder's gradient bytes) has been written — a data-parallel wrapper starts their
 * all-reduce there, under the backward of conv2 / conv1 (60 % of the backward's time), instead of after the call. */
#define TMF_SNET_DEEP_FROM 3
typedef struct tmf_snet_grads {
    float* dweight[TMF_SNET_BLOCKS];
    float* dbias[TMF_SNET_BLOCKS];
    float* dgamma[TMF_SNET_BLOCKS];
    float* dbeta[TMF_SNET_BLOCKS];
    void*  deep_event;
} tmf_snet_grads;
size_t tmf_snet_saved_bytes(const tmf_snet_desc* d);
size_t tmf_snet_bwd_scratch_bytes(const tmf_snet_desc* d);
int    tmf_snet_train_fwd(const tmf_snet_desc* d, const float* vol, const tmf_snet_params* params,
                          void* saved, size_t saved_bytes, float* out, void* stream);
int    tmf_snet_train_bwd(const tmf_snet_desc* d, const float* vol, const void* saved, size_t saved_bytes,
                          const float* dout, const tmf_snet_grads* grads, void* scratch, size_t scratch_bytes, void* stream);
int    tmf_snet_train_bwd_input(const tmf_snet_desc* d, const float* vol, const void* saved, size_t saved_bytes,
                                const float* dout, const tmf_snet_grads* grads, void* scratch, size_t scratch_bytes, void* stream,
                                float* dvol);
/* Inference form (val_step, kfold_train_adversarial.py:144-161; eval-mode BatchNorm folded into each block's single
 * conv + BN + LeakyReLU + pool kernel): one call per encoder, fp32 precision, running statistics required; `workspace`
 * (>= tmf_snet_eval_workspace_bytes) is scratch. */
size_t tmf_snet_eval_workspace_bytes(const tmf_snet_desc* d);
int    tmf_snet_eval_fwd(const tmf_snet_desc* d, const float* vol, const tmf_snet_params* params,
                         void* workspace, size_t workspace_bytes, float* out, void* stream);

/* ------------------------------------------------------------------------------
 * Whole-fusion entries (csrc/fusion_path.hip): ONE call enqueues every launch of CrossTransformer_MOD_AVG's train-mode
 * forward, or of its backward.  Replaces `self.fuse_transformer(mri_embeddings, pet_embeddings)` (models/mymodel.py:220
 * -> networks.py:272-281: depth x [mri <- Transformer(mri | pet) + mri; pet <- Transformer(pet | NEW mri) + pet], then
 * cat[mean, mean, max, max] over tokens) and its slice of `all_loss.backward()`.  Dropout (options/option.py:39) enters as
 * keep-masks in tmf_xformer_params, at every descriptor the entries accept (tmf_fusion_takes_masks).  dim of 64, 128 or
 * 256; heads*dim_head and mlp multiples of 64.  Dims other than 128 always run one launch per op.
 *
 * inst[2*l] / inst[2*l + 1] = the mri / pet Transformer(depth=1) of layer l, parameters = the reference's state_dict
 * tensors (nn.Linear weights (out, in)).  Gradients: small = [b2 (dim) | b1 (mlp) | bo (dim) | ln2 gamma | ln2 beta |
 * ln1 gamma | ln1 beta] contiguous (6*dim + mlp floats), lnf = [gamma | beta] of the block-final LayerNorm, dw* in the
 * nn.Linear layout.  mri_tok / pet_tok: [B][N][dim]; cls: [B][4*dim]; dmri_tok / dpet_tok: [B][N][dim].
 * ---------------------------------------------------------------------------- */
#define TMF_FUSION_MAX_DEPTH 16
/* flags: TMF_FUSION_PER_OP = enqueue one launch per Linear / attention / LayerNorm (token_gemm.hip, attention.hip,
 * token_ops.hip: 7 forward + 13 backward launches per instance) even where the fused per-instance kernels of
 * csrc/xformer_fused.hip apply (dim 128, 4 heads of 32 or — round 6 — 8 heads of 16, mlp 512, N <= 512: 1 forward + 2 backward launches per instance,
 * all weight gradients in one launch at the end).  Forward and backward of one pass must see the same desc. */
#define TMF_FUSION_PER_OP 1
typedef struct tmf_fusion_desc { int B, N, dim, heads, dim_head, mlp, depth, flags; } tmf_fusion_desc;
typedef struct tmf_xformer_params {
    const float *ln1_g, *ln1_b;         /* layers.0.0.norm                          (networks.py:117) */
    const float *wq, *wkv, *wo, *bo;    /* layers.0.0.fn.to_q / to_kv / to_out.0    (:149-155) */
    const float *ln2_g, *ln2_b;         /* layers.0.1.norm */
    const float *w1, *b1, *w2, *b2;     /* layers.0.1.fn.net.0 / net.3              (:129-132) */
    const float *lnf_g, *lnf_b;         /* norm                                     (:219) */
    float eps1, eps2, epsf;
    /* Dropout keep-masks of the instance ALREADY scaled by 1 / (1 - p), or NULL (eval, or p = 0): after to_out
     * (networks.py:153) [B*N][dim], after GELU (:131) [B*N][mlp], after the second Linear (:133) [B*N][dim].  The random
     * draw stays with the caller; the same pointers must be passed to forward and backward.  The fused kernels apply them
     * in their own epilogues, one launch per op in the masked token-GEMM / LayerNorm-backward instances. */
    const float *mask_o, *mask_g, *mask_f;
} tmf_xformer_params;
typedef struct tmf_xformer_grads {
    float *small, *lnf, *dwq, *dwkv, *dwo, *dw1, *dw2;
} tmf_xformer_grads;
/* Debugging hook (tools/xf_trace.py): when non-NULL, every wave of the fused kernels writes its phase time stamps
 * (shader clock) to fwd / bwd_q / bwd_kv, each [workgroups][4][16] uint64.  NULL (the default) turns it off. */
void   tmf_debug_xf_trace(void* fwd, void* bwd_q, void* bwd_kv);
size_t tmf_fusion_saved_bytes(const tmf_fusion_desc* d);
int    tmf_fusion_uses_fused(const tmf_fusion_desc* d);     /* 1: this descriptor's calls run the fused per-instance kernels */
int    tmf_fusion_takes_masks(const tmf_fusion_desc* d);    /* 1: this descriptor's calls take keep-masks (all it accepts) */
/* One launch per op (tmf_fusion_uses_fused = 0) always reserves room for the two masked gradients m_f * dx2, m_o * dx1
 * (2 B N dim floats), masks or not: the descriptor does not say whether masks come. */
size_t tmf_fusion_bwd_scratch_bytes(const tmf_fusion_desc* d);
int    tmf_fusion_train_fwd(const tmf_fusion_desc* d, const float* mri_tok, const float* pet_tok,
                            const tmf_xformer_params* inst, void* saved, size_t saved_bytes, float* cls, void* stream);
int    tmf_fusion_train_bwd(const tmf_fusion_desc* d, const float* mri_tok, const float* pet_tok,
                            const tmf_xformer_params* inst, const void* saved, size_t saved_bytes, const float* dcls,
                            const tmf_xformer_grads* grads, float* dmri_tok, float* dpet_tok,
                            void* scratch, size_t scratch_bytes, void* stream);
/* Forward-only form: `self.fuse_transformer(mri_embeddings, pet_embeddings)` under torch.no_grad() — val_step
 * (kfold_train_adversarial.py:144-161) and the test run after training (:229-250) — as ONE call that keeps nothing.
 * Descriptor rules, inst[], TMF_FUSION_PER_OP, the depth range (0 included: pooling only) and the keep-masks (non-NULL
 * masks are applied: a train-mode module under no_grad) are those of tmf_fusion_train_fwd, and cls is bit-identical to
 * its cls.  `workspace` (>= tmf_fusion_infer_workspace_bytes, 16-byte aligned) is scratch: never read before it is
 * written within the call, meaningless after it; mri_tok / pet_tok are not written.  It holds no per-instance
 * activations — fused geometry: the two running token buffers, the K-row / V-column panels of the current and the next
 * context, one forward weight pack (4 dim^2 + 2 mlp dim floats) per instance, the pool's argmax; one launch per op: one
 * instance's intermediates reused by every instance and the running token buffers (size independent of depth). */
size_t tmf_fusion_infer_workspace_bytes(const tmf_fusion_desc* d);
int    tmf_fusion_infer_fwd(const tmf_fusion_desc* d, const float* mri_tok, const float* pet_tok,
                            const tmf_xformer_params* inst, void* workspace, size_t workspace_bytes,
                            float* cls, void* stream);
/* The forward-only pass with the attention maps of every Transformer instance (tmf_xattn_probs after each instance's
 * attention).  Always one launch per op, whatever desc->flags says: cls is bit-identical to tmf_fusion_infer_fwd with
 * TMF_FUSION_PER_OP.  probs: [2*depth][B][heads][N][N] or NULL; recv: [2*depth][B][heads][N] (required).  Instance 2l =
 * layer l's mri encoder (queries mri, keys pet), 2l + 1 = its pet encoder (queries pet, keys the NEW mri tokens).
 * Everything else as tmf_fusion_infer_fwd; workspace >= tmf_fusion_attn_maps_workspace_bytes. */
size_t tmf_fusion_attn_maps_workspace_bytes(const tmf_fusion_desc* d);
int    tmf_fusion_attn_maps(const tmf_fusion_desc* d, const float* mri_tok, const float* pet_tok,
                            const tmf_xformer_params* inst, void* workspace, size_t workspace_bytes,
                            float* cls, float* probs, float* recv, void* stream);

/* ------------------------------------------------------------------------------
 * The dense heads of model_ad in one launch per direction (csrc/heads.hip).  Replaces `self.D(D_MRI_inp)`,
 * `self.D(D_PET_inp)` on the reversed-gradient token means and `self.fc_cls(fused_embeds)` (models/mymodel.py:209-215,
 * 221; modules :190-194) and their backward.  fc_cls = Linear(4*dim, H1)-BatchNorm1d-ReLU-Dropout-Linear(H1, H2)-
 * BatchNorm1d-ReLU-Dropout-Linear(H2, NC);  D = Linear(dim, HD)-BatchNorm1d-ReLU-Linear(HD, NC), applied to the MRI then
 * the PET mean with separate batch statistics (running statistics updated twice, in that order).  B <= 32 (round 6; instances holding 16 / 32 batch rows in registers).
 *   cls [B][4*dim]; mri_tok / pet_tok [B][N][dim] (their means over N are D's inputs); mask1 [B][H1], mask2 [B][H2]:
 *   Dropout keep-masks ALREADY scaled by 1 / (1 - p), NULL = no dropout (eval, or p = 0); the random draw stays with the
 *   caller.  training != 0: batch statistics + running update (momentum / eps index 0 = fc_cls.1, 1 = fc_cls.5, 2 = D.1);
 *   else running statistics.  Outputs: logits, d_mri_logits, d_pet_logits [B][NC]; `saved` (tmf_heads_saved_bytes) for
 *   backward.  Backward: parameter gradients into g (same shapes as the parameters; D's collect both calls), d_cls,
 *   and d_mri_tok / d_pet_tok = -revgrad_alpha * dmean / N broadcast over the tokens (gradient reversal, mymodel.py:209).
 * ---------------------------------------------------------------------------- */
typedef struct tmf_heads_desc { int B, N, dim, H1, H2, HD, NC, training; float momentum[3], eps[3]; } tmf_heads_desc;
typedef struct tmf_heads_params {
    const float *fc0_w, *fc0_b, *bn1_g, *bn1_b, *fc4_w, *fc4_b, *bn5_g, *bn5_b, *fc8_w, *fc8_b;   /* fc_cls.0/.1/.4/.5/.8 */
    const float *d0_w, *d0_b, *dbn_g, *dbn_b, *d3_w, *d3_b;                                         /* D.0/.1/.3 */
    float *bn1_rm, *bn1_rv, *bn5_rm, *bn5_rv, *dbn_rm, *dbn_rv;                                     /* running statistics */
} tmf_heads_params;
typedef struct tmf_heads_grads {
    float *fc0_w, *fc0_b, *bn1_g, *bn1_b, *fc4_w, *fc4_b, *bn5_g, *bn5_b, *fc8_w, *fc8_b, *d0_w, *d0_b, *dbn_g, *dbn_b, *d3_w, *d3_b;
} tmf_heads_grads;
size_t tmf_heads_saved_bytes(const tmf_heads_desc* d);
size_t tmf_heads_bwd_scratch_bytes(const tmf_heads_desc* d);
int    tmf_heads_fwd(const tmf_heads_desc* d, const float* cls, const float* mri_tok, const float* pet_tok,
                     const float* mask1, const float* mask2, const tmf_heads_params* params, float* logits,
                     float* d_mri_logits, float* d_pet_logits, void* saved, size_t saved_bytes, void* stream);
int    tmf_heads_bwd(const tmf_heads_desc* d, const float* cls, const float* mask1, const float* mask2,
                     const tmf_heads_params* params, const void* saved, size_t saved_bytes, const float* d_logits,
                     const float* d_d_mri_logits, const float* d_d_pet_logits, const tmf_heads_grads* grads,
                     float* d_cls, float* d_mri_tok, float* d_pet_tok, float revgrad_alpha,
                     void* scratch, size_t scratch_bytes, void* stream);

/* Scaled keep-masks of several nn.Dropout modules in ONE launch (mymodel.py:190-191: the two Dropout(0.5) of fc_cls; the
 * Dropout modules of the fusion block, networks.py:131,133,153): out[s][e] = 1 / keep[s] with probability keep[s], else 0,
 * from a counter-based generator (Philox4x32-10 keyed by `seed`, counter = (element / 4, segment, offset)): the masks are a
 * pure function of (seed, offset), `offset` distinguishes the calls of a run.  nseg <= TMF_MASK_SEGMENTS. */
#define TMF_MASK_SEGMENTS 20
int    tmf_dropout_keep_masks(int nseg, float* const* out, const long* numel, const float* keep,
                              unsigned long long seed, unsigned long long offset, void* stream);

/* The heads of the CNN-only models, one launch per direction (csrc/heads.hip).
 * reference: models/mymodel.py:143-178 model_CNN_ad — `fc_cls` = Linear(2 dim, H)-ReLU-Linear(H, NC) on
 * cat[gap(mri), gap(pet)] and `D` (as in model_ad) on revgrad(gap(mri), 2), revgrad(gap(pet), 2): M = 2, HD = 128;
 * models/mymodel.py:13-41 model_single — `fc` = Linear(dim, H)-ReLU-Linear(H, NC) on avgpool(cnn(img)): M = 1, HD = 0
 * (pet_tok, the D parameters / outputs / gradients are then NULL).  Tokens [B][N][dim] = the encoder output, channels last;
 * gap == mean over N.  B <= 32, dim % 16 == 0, M dim <= 512.  momentum / eps are D's BatchNorm1d's. */
typedef struct tmf_heads_cnn_desc { int B, N, dim, M, H, HD, NC, training; float momentum, eps; } tmf_heads_cnn_desc;
typedef struct tmf_heads_cnn_params {
    const float *fc0_w, *fc0_b, *fc2_w, *fc2_b;              /* [H][M dim], [H], [NC][H], [NC] */
    const float *d0_w, *d0_b, *dbn_g, *dbn_b;                /* [HD][dim], [HD], [HD], [HD] */
    float *dbn_rm, *dbn_rv;                                  /* running statistics: updated twice per training call, or NULL */
    const float *d3_w, *d3_b;                                /* [NC][HD], [NC] */
} tmf_heads_cnn_params;
typedef struct tmf_heads_cnn_grads { float *fc0_w, *fc0_b, *fc2_w, *fc2_b, *d0_w, *d0_b, *dbn_g, *dbn_b, *d3_w, *d3_b; } tmf_heads_cnn_grads;
size_t tmf_heads_cnn_saved_bytes(const tmf_heads_cnn_desc* d);
size_t tmf_heads_cnn_bwd_scratch_bytes(const tmf_heads_cnn_desc* d);
int    tmf_heads_cnn_fwd(const tmf_heads_cnn_desc* d, const float* mri_tok, const float* pet_tok,
                         const tmf_heads_cnn_params* params, float* logits, float* d_mri_logits, float* d_pet_logits,
                         void* saved, size_t saved_bytes, void* stream);
int    tmf_heads_cnn_bwd(const tmf_heads_cnn_desc* d, const tmf_heads_cnn_params* params, const void* saved, size_t saved_bytes,
                         const float* d_logits, const float* d_d_mri_logits, const float* d_d_pet_logits,
                         const tmf_heads_cnn_grads* grads, float* d_mri_tok, float* d_pet_tok, float revgrad_alpha,
                         void* scratch, size_t scratch_bytes, void* stream);

/* ---- optimizer step: torch.optim.Adam over ALL parameter tensors in one launch --------------------------------------
 * reference: kfold_train_adversarial.py:135 (optimizer.step()), utils/utils.py:38-39 (Adam, lr 1e-4, weight decay 0).
 * params[i] / grads[i]: device pointers of tensor i (numel[i] contiguous floats); grads[i] == NULL skips the tensor, as
 * torch does for a parameter without a gradient.  exp_avg / exp_avg_sq: the two moment estimates of ALL tensors in two
 * flat caller-owned buffers of tmf_adam_state_elems(n, numel) floats, zero before the first step (tensor i's slice
 * starts at the sum of the preceding numel, each rounded up to a multiple of 4).  step: the update count INCLUDING this
 * one (1 on the first call).  weight_decay is torch's L2 form (added to the gradient).  n <= TMF_ADAM_MAX_TENSORS per
 * call (the tensor table is a kernel argument); larger sets take several calls with their own state slices. */
#define TMF_ADAM_MAX_TENSORS 160
long   tmf_adam_state_elems(int n, const long* numel);
int    tmf_adam_step(int n, float* const* params, const float* const* grads, const long* numel,
                     float* exp_avg, float* exp_avg_sq, double lr, double beta1, double beta2, double eps,
                     double weight_decay, int step, void* stream);

/* ---- optimizer step: torch.optim.SGD (weight decay, momentum) over ALL parameter tensors in one launch -----------------
 * reference: utils/utils.py:34-37 (getOptimizer with --optimizer SGD: lr, weight_decay; options/option.py:32,35),
 * kfold_train_Mnet.py:85 (SGD(lr=0.001, momentum=0.9)).  g' = g + weight_decay p;  momentum == 0: p -= lr g';  otherwise
 * buf = g' for a tensor without a momentum buffer yet (torch: a clone of g', not scaled), else buf = momentum buf + g';
 * p -= lr buf.  dampening, nesterov and maximize are not offered (no reference caller uses them).
 * params / grads / numel / n: as for tmf_adam_step (grads[i] == NULL skips tensor i).  momentum_buf: the momentum buffers of
 * ALL tensors in one flat caller-owned buffer of tmf_adam_state_elems(n, numel) floats in that function's layout; it needs
 * no initial fill.  no_buffer_yet: n ints in HOST memory, non-zero for a tensor whose buffer holds nothing yet; tensors of both
 * kinds share the launch.  The caller clears the flag of every tensor that had a gradient after the call.  momentum_buf and
 * no_buffer_yet may be NULL exactly when momentum == 0 (they are not read then). */
int    tmf_sgd_step(int n, float* const* params, const float* const* grads, const long* numel, float* momentum_buf,
                    const int* no_buffer_yet, double lr, double momentum, double weight_decay, void* stream);

/* ---- losses (csrc/losses.hip) -------------------------------------------------------------------------------------
 * FALoss, reference models/losses.py:122-128: two (B, N, N) similarity matrices F^T F (N = h*w*d tokens of a
 * (B, C, h, w, d) map), their difference D and F.l1_loss over it.  Here D is formed tile by tile on the matrix pipe and never
 * written.  f1, f2: fp32 maps of B samples, channels_last == 0: [B][C][N] (NCDHW-contiguous), != 0: [B][N][C] (the
 * storage behind this library's sNet output).  reduction: 0 'mean' (sum |D| / (B N^2)), 1 'sum'.  loss: one float.
 * g1, g2 (both or neither; NULL: no gradient wanted): the UNSCALED gradients F1 sign(D) and -F2 sign(D) in the layout of
 * the inputs; tmf_faloss_bwd turns them into d1 = g1 * 2 grad_out[0] / (B N^2), d2 likewise ('sum': no divisor),
 * grad_out a device scalar.  The forward of a training step costs 2x the products of a no-grad one and the backward
 * none; recomputing D in the backward would cost 3x in all.  workspace: tmf_faloss_workspace_bytes(B, N) bytes, 8-byte
 * aligned: tmf_faloss_partial_rows(B, N) per-workgroup partial sums (double), reduced in a fixed order.
 * tmf_faloss_ok: 1 when (C, N, reduction) takes the kernels: C a multiple of 32 up to 256, N >= 1, C * N < 2^31.
 * Two launches forward, one backward. */
int    tmf_faloss_ok(int C, int N, int reduction);
int    tmf_faloss_partial_rows(int B, int N);
size_t tmf_faloss_workspace_bytes(int B, int N);
int    tmf_faloss_fwd(const float* f1, const float* f2, float* loss, float* g1, float* g2, void* workspace,
                      size_t workspace_bytes, int B, int C, int N, int channels_last, int reduction, void* stream);
int    tmf_faloss_bwd(const float* g1, const float* g2, const float* grad_out, float* d1, float* d2, int B, int C, int N,
                      int reduction, void* stream);
/* SupConLoss, reference models/losses.py:59-100: features [bs][views][d] fp32 contiguous; contrast row views-major
 * (row v * bs + s = features[s][v]); anchors: all rows (anchors_all != 0, contrast_mode 'all') or the bs rows of view 0
 * ('one').  Positives: labels (int64 [bs], device) equal, or mask (float [bs][bs], device, may be asymmetric), or with
 * both NULL the identity (SimCLR); the self column is excluded from positives and from the log-sum-exp.  An anchor without
 * a positive gives NaN, as the formula does.  loss: one float.  gfeat (NULL: none): dloss/dfeatures for grad_out = 1;
 * tmf_supcon_bwd scales it by the device scalar grad_out[0].  tmf_supcon_ok: 1 when bs * views <= 128 and d % 4 == 0.
 * One launch each, one workgroup. */
int    tmf_supcon_ok(int bs, int views, int d);
int    tmf_supcon_fwd(const float* features, const long long* labels, const float* mask, float* loss, float* gfeat,
                      int bs, int views, int d, int anchors_all, float temperature, float base_temperature, void* stream);
int    tmf_supcon_bwd(const float* gfeat, const float* grad_out, float* dfeat, int bs, int views, int d, void* stream);

/* ---- criterion and epoch metrics (csrc/criterion.hip) --------------------------------------------------------------
 * Cross entropy, reference kfold_train_adversarial.py:94 / kfold_train_single.py:87 (torch.nn.CrossEntropyLoss(), optionally
 * weight=...) and its call sites :119, :125, :159.  logits: fp32 [B][C] contiguous; target: int64 [B] class indices, -100
 * (torch's default ignore_index) counts with weight 0, any other value outside [0, C) makes the loss NaN and its gradient
 * row zero; weight: NULL or C floats.  reduction: 0 'mean' (torch's: sum w[y_i] l_i / sum w[y_i]), 1 'sum'.  loss: one
 * float.  g (NULL: no gradient wanted): dloss / dlogits [B][C]; tmf_ce_bwd forms dlogits = grad_out[0] * g, grad_out a
 * device scalar.  Accurate expf / logf, the row maximum subtracted first; sums over samples in double in a fixed order.
 * tmf_ce_ok: 1 when 1 <= B <= 4096 and 2 <= C <= 16.  One launch each, one workgroup forward. */
int    tmf_ce_ok(int B, int C);
int    tmf_ce_fwd(const float* logits, const long long* target, const float* weight, float* loss, float* g, int B, int C,
                  int reduction, void* stream);
int    tmf_ce_bwd(const float* g, const float* grad_out, float* dlogits, int B, int C, void* stream);
/* The whole criterion of kfold_train_adversarial.py:119-125 in one launch: losses[0] = CE(logits, label) ('mean', weight
 * NULL or C floats), losses[1] = (CE(d_mri, all ones) + CE(d_pet, all zeros)) / 2.  d_mri, d_pet: fp32 [B][2] (the domain
 * discriminator's logits); their targets are formed in the kernel.  g_logits [B][C], g_mri, g_pet [B][2] (all three or
 * none): the gradient of losses[0] (g_logits) or of losses[1] (g_mri, g_pet: the 1/2 included) by its own logits.
 * tmf_adv_criterion_bwd, replacing the autograd backward of :131-132: dlogits = grad_ce[0] * g_logits, dmri = grad_ad[0] *
 * g_mri, dpet = grad_ad[0] * g_pet in one launch; grad_ce, grad_ad: device scalars, NULL meaning zero. */
int    tmf_adv_criterion_fwd(const float* logits, const float* d_mri, const float* d_pet, const long long* label,
                             const float* weight, float* losses, float* g_logits, float* g_mri, float* g_pet, int B, int C,
                             void* stream);
int    tmf_adv_criterion_bwd(const float* g_logits, const float* g_mri, const float* g_pet, const float* grad_ce,
                             const float* grad_ad, float* dlogits, float* dmri, float* dpet, int B, int C, void* stream);
/* The trainer's metrics of kfold_train_adversarial.py:178-182 (ignite Accuracy of the three heads, Average of the two
 * losses read at :127-128) as one read-add-write of a device state: one launch, one workgroup; calls on one stream
 * serialize, the caller zeroes the state to reset.  state: 8 words of 8 bytes, 8-byte aligned — [0] updates, [1] samples
 * (int64); [2] sum of losses[0], [3] sum of losses[1] (double); [4], [5], [6] samples whose argmax (the first maximal
 * index; a NaN counts as the maximum, as in torch.argmax) equals the target, for logits / label, d_mri / 1, d_pet / 0
 * (int64); [7] unused.  losses: the two device floats of tmf_adv_criterion_fwd. */
#define TMF_TRAIN_METRICS_WORDS 8
int    tmf_train_metrics_update(void* state, const float* losses, const float* logits, const float* d_mri, const float* d_pet,
                                const long long* label, int B, int C, void* stream);
/* The evaluator's metrics of :183-187 (ignite Accuracy, ConfusionMatrix, ROC_AUC, Loss): one launch, one workgroup.
 * state: (2 + C * C) words of 8 bytes — [0] sum of the per-sample cross entropy (double), [1] samples (int64),
 * [2 + t * C + p] samples of true class t predicted as p = argmax (int64; row true, column predicted: the convention of
 * ignite, scikit-learn and utils/utils.py:44-51).  scores[offset + i] = softmax(logits_i)[C - 1] (fp32),
 * labels_out[offset + i] = label[i]: the epoch buffers tmf_auc reads; the host keeps `offset`. */
int    tmf_eval_metrics_update(void* state, float* scores, long long* labels_out, long offset, const float* logits,
                               const long long* label, int B, int C, void* stream);
/* Exact ROC AUC (ignite ROC_AUC -> sklearn.metrics.roc_auc_score) as the Mann-Whitney statistic in integers:
 * out[0] = T = sum over (positive i, negative j) of 2 [s_i > s_j] + [s_i == s_j], out[1] = P, out[2] = N (uint64; a label
 * of 0 is negative, any other positive); AUC = T / (2 P N), formed by the host in double.  Pair tiles over many workgroups,
 * per-workgroup counts in `workspace` (tmf_auc_workspace_bytes(n) bytes, 8-byte aligned), summed by a second launch:
 * integer counts, so the result does not depend on any order.  tmf_auc_ok: 1 when 1 <= n <= 65536. */
int    tmf_auc_ok(long n);
size_t tmf_auc_workspace_bytes(long n);
int    tmf_auc(const float* scores, const long long* labels, long n, void* workspace, void* out, void* stream);

/* ------------------------------------------------------------------------------
 * Class activation maps at an encoder block (csrc/cam.hip): act = the block's channels-last output A[B][V][C] (V = d*h*w),
 * grad = d score / d A, same layout.
 *   TMF_CAM_GRAD  (Grad-CAM):  w[b][c] = (1/V) sum_v grad[b][v][c],  cam[b][v] = sum_c w[b][c] act[b][v][c]
 *   TMF_CAM_HIRES (HiResCAM):  cam[b][v] = sum_c grad[b][v][c] act[b][v][c]
 * flags: TMF_CAM_RELU clamps the map at 0; TMF_CAM_NORMALIZE then divides each sample's map by its maximum — a sample
 * whose maximum is <= 0 comes out as zeros, never NaN or Inf.
 * cam [B][V]; weights [B][C] (TMF_CAM_GRAD only) or NULL; peak [B] = each sample's maximum before the division (after the
 * clamp) or NULL.  cam may be NULL when weights is not (the weights alone; peak then NULL).  act, grad and workspace are
 * 16-byte aligned.  C: tmf_cam_ok = a multiple of 4 in 8..512; any B, V >= 1.  act and grad are read once (grad's
 * Grad-CAM pass reads grad only, the map pass act only), 16 bytes per lane; no atomics: per-workgroup partials in
 * `workspace` (tmf_cam_workspace_bytes, 0 for a shape tmf_cam refuses) combined in a fixed order — two calls give the same
 * bits.  Launches: 3 (Grad: column sums, map, normalise) or 2 (HiRes); the last one only with TMF_CAM_NORMALIZE or peak. */
#define TMF_CAM_GRAD      0
#define TMF_CAM_HIRES     1
#define TMF_CAM_RELU      1
#define TMF_CAM_NORMALIZE 2
int    tmf_cam_ok(int C);
size_t tmf_cam_workspace_bytes(int B, long V, int C, int method);
int    tmf_cam(const float* act, const float* grad, float* cam, float* weights, float* peak, void* workspace,
               size_t workspace_bytes, int B, long V, int C, int method, int flags, void* stream);

/* ------------------------------------------------------------------------------
 * Occlusion sensitivity (csrc/occlusion.hip): blank a region of a volume, run the network again, record how far the class
 * score falls.  The reference has no such function; these entries replace the loop its user writes around the deployed
 * model: `for w in windows: x = vol.clone(); x[..., z0:z1, y0:y1, x0:x1] = fill; drop[w] = base - score(model(x))` and, for
 * the voxel map, `for w in windows: acc[..., z0:z1, y0:y1, x0:x1] += drop[w]; cnt[z0:z1, y0:y1, x0:x1] += 1; acc / cnt`.
 *
 * Window grid.  Per axis with extent S, patch p and stride s, 1 <= s <= p: n = ceil(max(S - p, 0) / s) + 1 windows, window
 * i covers [i*s, min(i*s + p, S)) — the last one may be shorter, S <= p gives one window, and every voxel lies in at least
 * one window.  nW = nd*nh*nw, window w = (id*nh + ih)*nw + iw.
 * Regions.  Instead of a grid, `labels` is an int32 volume [D][H][W] with labels 0..R: 0 is background and never occluded,
 * job r-1 occludes the voxels with label r (nW = R); a label outside 0..R occludes nothing and maps to 0.
 * Jobs.  Job j = b*nW + w is sample b with window / region w replaced by fill[b] (one float per sample).
 * Drop.  drops[b][w] = score(unoccluded) - score(job), computed by the caller.
 * Voxel map.  Grid: vmap[b][z][y][x] = the mean of drops[b][w] over the windows that contain the voxel — the sum in
 * ascending w in fp32, then ONE division by the count.  Regions: vmap = drops[b][label - 1], 0 elsewhere.
 *
 * tmf_occlusion_windows: nW of a geometry, or the negative TMF_E_* the other entries return for it.
 * tmf_occlude_windows / tmf_occlude_labels: out[k] ([K][D][H][W]) = vol[(j0+k) / nW] with window / region (j0+k) % nW set to
 *   fill[(j0+k) / nW]; a chunk may straddle samples.  ONE launch, a pure copy: the bits of clone() plus slice assignment.
 * tmf_occlusion_volume / tmf_occlusion_volume_labels: drops [B][nW] -> vmap [B][D][H][W], ONE launch, a gather (one output
 *   voxel per lane element, no atomics): two calls give the same bits.
 * 16 bytes per lane where D*H*W % 4 == 0 and vol, out, vmap (and labels) are 16-byte aligned, one element per lane
 * otherwise; every pointer 4-byte aligned (TMF_E_ALIGN).  Limits (TMF_E_SHAPE / TMF_E_ARG, nothing launched): extents >= 1
 * with D*H*W < 2^31 (element offsets inside a volume are 32-bit, between volumes 64-bit); patch >= 1, 1 <= stride <= patch
 * per axis; R >= 1; B >= 1 with B*nW < 2^31; j0 >= 0, 1 <= K <= 65536, j0 + K <= B*nW; B <= 65536 for the voxel maps. */
int    tmf_occlusion_windows(int D, int H, int W, int pd, int ph, int pw, int sd, int sh, int sw);
int    tmf_occlude_windows(const float* vol, const float* fill, float* out, int B, int D, int H, int W, int pd, int ph, int pw,
                           int sd, int sh, int sw, int j0, int K, void* stream);
int    tmf_occlude_labels(const float* vol, const int* labels, const float* fill, float* out, int B, int D, int H, int W, int R,
                          int j0, int K, void* stream);
int    tmf_occlusion_volume(const float* drops, float* vmap, int B, int D, int H, int W, int pd, int ph, int pw, int sd, int sh,
                            int sw, void* stream);
int    tmf_occlusion_volume_labels(const float* drops, const int* labels, float* vmap, int B, int D, int H, int W, int R,
                                   void* stream);

/* ------------------------------------------------------------------------------
 * Deletion / insertion curves (csrc/faithfulness.hip; Petsiuk et al., RISE, 2018): rank the voxels of a volume by an
 * attribution, blank (deletion) or reveal (insertion) the top n_1 <= n_2 <= ... <= n_S of them, run the network each time.
 * The reference has no such function; these entries replace the loop its user writes around the deployed model:
 * `srt = attr.sort(descending=True); for k: x = torch.where(attr >= srt[n_k - 1], fill, vol); score[k] = model(x)`.
 *
 * Ordering.  Voxels are ordered by a = attr + 0.0f (-0.0 ranks with +0.0), compared as floats; infinities are ordinary
 * values.  NaN is not supported: the values written are then unspecified, but nothing faults or is written out of bounds.
 * Ties go together, there is no tie-break by index: a step removes every voxel at or above its threshold.
 *
 * tmf_rank_thresholds: attr [B][V], counts[S] (HOST memory, read during the call; non-decreasing, each in 1..V, repeats
 *   allowed) -> thr [B][S] float, thr[b][k] = the counts[k]-th largest a of row b, one of the row's values bit for bit; and
 *   removed [B][S] int32 = the number of voxels of row b with a >= thr[b][k] (>= counts[k], equal where the values are
 *   distinct).  Both exact: a multi-quantile radix select on the order-preserving uint32 image of a, digits of 11, 11 and
 *   10 bits, integer counting only — two calls give the same bits; no sort.  Seven stream operations whatever B and V (one
 *   hipMemsetAsync of the workspace — the ENTRY zeroes it, the caller need not — and six launches), no host
 *   synchronisation, no device-to-host copy.  workspace: tmf_rank_workspace_bytes(B, V, S) bytes (0 for arguments the
 *   entry refuses), 16-byte aligned.
 * tmf_mask_by_rank: job j = b*(S+1) + s, s in 0..S; m(v) = false for s == 0, else a[b][v] >= thr[b][s-1].  out[k]
 *   ([K][V], job j0 + k) = m ? f : vol[b] (mode TMF_RANK_DELETION) or m ? vol[b] : f (TMF_RANK_INSERTION), with
 *   f = base[b][v] where `base` ([B][V], e.g. a blurred copy) is non-NULL, else fill[b] (one float per sample; `fill` may be
 *   NULL where base is given).  A chunk may straddle samples.  ONE launch, a pure select: the bits of torch.where.
 * 16 bytes per lane where V % 4 == 0 and attr (and vol, base, out) are 16-byte aligned, one element per lane otherwise;
 * every pointer 4-byte aligned, the workspace 16-byte (TMF_E_ALIGN).  Limits (TMF_E_SHAPE / TMF_E_ARG / TMF_E_WORKSPACE, nothing launched):
 * B >= 1 (<= 65536 for the thresholds), 1 <= V < 2^31, 1 <= S <= TMF_RANK_MAX_STEPS, B*(S+1) < 2^31; j0 >= 0,
 * 1 <= K <= 65536, j0 + K <= B*(S+1). */
#define TMF_RANK_MAX_STEPS 64
#define TMF_RANK_DELETION  0
#define TMF_RANK_INSERTION 1
size_t tmf_rank_workspace_bytes(int B, long V, int S);
int    tmf_rank_thresholds(const float* attr, const int* counts, float* thr, int* removed, void* workspace,
                           size_t workspace_bytes, int B, long V, int S, void* stream);
int    tmf_mask_by_rank(const float* vol, const float* attr, const float* thr, const float* fill, const float* base, float* out,
                        int B, long V, int S, int mode, int j0, int K, void* stream);

/* ------------------------------------------------------------------------------
 * Atlas region statistics of attribution maps (csrc/region_stats.hip): which brain regions carry a voxel map.  The reference
 * has no such function; these entries replace what its user writes with stock ops for every map:
 * `cnt = bincount(lab); s = bincount(lab, weights=a); s_abs = bincount(lab, weights=a.abs()); s_pos = bincount(lab,
 * weights=a.clamp(min=0)); mx = full(-inf).scatter_reduce(0, lab, a, "amax"); arg = per region the first index where a == mx`
 * - five or more passes over the volume with float atomics, whose sums change in their last bits from run to run - and, for
 * the group table, `for b: n[cls[b]] += 1; sx[cls[b]] += x[b]; sxx[cls[b]] += x[b]**2` in fp64.
 *
 * Bins.  a [B][V] float, labels [V] int32 (ONE atlas for all samples: the volumes are registered), R >= 1.  Bin r in 1..R
 * collects the voxels with label r, bin 0 every other voxel: label 0, negative labels and labels above R (the range is
 * checked before any index is formed from a label).
 * Outputs, [B][R+1] but for count: count [R+1] int32 (a property of the atlas alone); sum = the sum of a; abs_sum of |a|;
 * pos_sum of max(a, 0); max = the largest a + 0.0f of the bin, one of its values bit for bit, -inf for an empty bin; argmax
 * int32 = the lowest linear voxel index that attains max, -1 for an empty bin.  Each of the five per-sample outputs may be
 * NULL and is then not written.  count, max and argmax are exact.
 * Sums.  Integers only, so the bits depend on neither the grid nor the order of arrival, and two calls give the same bits.
 * With peak_b = max |a[b]|, 2^(e-1) <= peak_b < 2^e and shift = 62 - ceil(log2 V), every |a| is scaled by the power of two
 * 2^(shift-e) and rounded ONCE to an integer (half away from zero); the positive and the negative voxels of a bin are added
 * up apart in 64-bit integers (V values below 2^shift stay below 2^62), sum = P - N, abs_sum = P + N, pos_sum = P, each
 * scaled back in fp64 and rounded once to float.  Against exact arithmetic, with n_r = count[r]:
 *     |got - exact| <= n_r * peak_b * 2^-shift + 2^-23 * |exact|
 * (shift >= 31; 42 at 96^3), which lies below n_r * 2^-24 * max(peak_b, sum |a|) + 2^-23 * |exact| for every V.  Sums of
 * integers below 2^24 are exact.  An all-zero sample gives sums 0, max 0 and argmax = the bin's lowest index.  Non-finite
 * inputs are not supported: the values written are then unspecified, but nothing faults or is written out of bounds.
 * Passes.  The map is read TWICE (once for peak_b, once for the bins: the second read of a 96^3 batch comes from the
 * last-level cache), the labels once per sample, 16 bytes per lane where V % 4 == 0 and `a` and `labels` are 16-byte
 * aligned, one element per lane otherwise.  Four stream operations whatever B, V and R: one hipMemsetAsync of the
 * workspace (the ENTRY zeroes it, the caller need not) and three launches; no host synchronisation, no device-to-host copy.
 * workspace: tmf_region_workspace_bytes(B, V, R) bytes (0 for arguments the entry refuses), 16-byte aligned.
 *
 * tmf_region_group_update: values [B][R+1] float (abs_sum, a share, ...; first = 0) or [B][R] for the regions 1..R alone
 * (occlusion's drops with an atlas; first = 1: bin 0 of the state is not touched), cls [B] int64, state [C][R+1][3] double =
 * (n, sum x, sum x^2) per class and region, updated in place: ONE launch, one thread per (c, r) walks b in ascending order and
 * adds 1, x and x*x (x widened to double, the product rounded before it is added) for the samples with cls[b] == c; a sample
 * with a class outside 0..C-1 is skipped.  No atomics: the bits of that loop in fp64.
 *
 * Every pointer 4-byte aligned (cls and state 8-byte), the workspace 16-byte (TMF_E_ALIGN).  Limits (TMF_E_SHAPE / TMF_E_ARG
 * / TMF_E_WORKSPACE, nothing launched): 1 <= B <= 65536, 1 <= V < 2^31, 1 <= R <= TMF_REGION_MAX, 1 <= C <=
 * TMF_REGION_MAX_CLASSES. */
#define TMF_REGION_MAX         1024
#define TMF_REGION_MAX_CLASSES 16
size_t tmf_region_workspace_bytes(int B, long V, int R);
int    tmf_region_stats(const float* a, const int* labels, int* count, float* sum, float* abs_sum, float* pos_sum, float* max_value,
                        int* argmax, void* workspace, size_t workspace_bytes, int B, long V, int R, void* stream);
int    tmf_region_group_update(const float* values, const int64_t* cls, double* state, int B, int R, int C, int first,
                               void* stream);

/* ------------------------------------------------------------------------------
 * Connected clusters of voxel maps and the cluster table (csrc/clusters.hip): threshold a map, find its connected clusters,
 * report each cluster's size, peak, peak voxel, centre and extent.  The reference has no such function; these entries replace a
 * device-to-host copy and `scipy.ndimage.label` per sample, or a `max_pool3d` propagation loop whose number of launches
 * depends on the data and which reads a "changed" flag on the host every round.
 *
 * tmf_cluster_label.  a [B][D][H][W] float, W fastest; thr [B] float in DEVICE memory (a threshold of tmf_rank_thresholds
 * needs no host read).  Foreground: a >= thr[b] (TMF_CLUSTER_POS), a <= -thr[b] (TMF_CLUSTER_NEG), |a| >= thr[b]
 * (TMF_CLUSTER_ABS), compared as floats: a NaN voxel is never foreground, a NaN threshold gives no foreground, -0.0 equals +0.0.
 * Neighbours.  connectivity 6: the voxels that share a face; 18: a face or an edge; 26: a face, an edge or a corner -
 * scipy's generate_binary_structure(3, 1 / 2 / 3).  Two foreground voxels lie in one cluster iff a chain of neighbouring
 * foreground voxels joins them; samples never connect.
 * Numbering.  Per sample, the clusters with at least min_size voxels are numbered 1, 2, ... in ASCENDING ORDER OF THEIR LOWEST
 * LINEAR VOXEL INDEX (the order of scipy.ndimage.label); smaller clusters and the background get 0.  labels [B][D][H][W]
 * int32: EVERY element is written.  n_clusters [B] int32 = the number of surviving clusters, or -1 if a chain-following loop
 * exceeded its bound (V trips) - that does not happen on a correct build; the labels of that sample are then unspecified.
 * The result is a function of the inputs alone - not of the grid, the scheduling or the order of arrival: two calls give the
 * same bits.
 * How.  Union-find by lowest index: a cluster's root is its lowest linear index, a union points the larger of two roots at the
 * smaller by an integer atomic min.  One workgroup labels one 8 x 8 x 32 tile in LDS; a second launch unites neighbours across
 * tile faces in memory (every access to the parents in that launch is a relaxed agent-scope atomic, as another XCD may have
 * written them); a third follows each voxel's chain to its root into a separate array and counts sizes by integer atomics at
 * the root; a three-launch prefix sum over V ranks the surviving roots; the last launch writes the labels.  No lane waits for
 * another workgroup (no flag, no ticket, no look-back), every chain-following loop is bounded.  EIGHT stream operations
 * whatever B, the data and the number of clusters: one hipMemsetAsync (the ENTRY zeroes the part of the workspace that needs
 * it, the caller need not) and seven launches; no host synchronisation, no device-to-host copy.
 * workspace: tmf_cluster_workspace_bytes(B, D, H, W) bytes (8 bytes per voxel and a little; 0 for a shape the entry refuses),
 * 16-byte aligned.
 *
 * tmf_cluster_table.  a as above; labels [B][D][H][W] int32 from tmf_cluster_label or anywhere else: a label outside 1..K is
 * ignored (the range is checked before any index is formed from it), row k-1 collects the voxels with label k.  s(a) = a (POS),
 * -a (NEG), |a| (ABS).  Outputs, [B][K] per field, each may be NULL and is then not written:
 *   size       int32: the voxels of the cluster;
 *   peak       float: the value a of the voxel `argmax`, bit for bit; NaN (0x7FC00000) for an empty row;
 *   argmax     int32: the lowest linear index (inside the sample) among the voxels whose s(a) is the row's largest (-0.0 ranks
 *              with +0.0), -1 for an empty row;
 *   coord_sum  int64 [B][K][3]: the sums of d, h and w over the cluster (the centroid is exact on the host side);
 *   bbox       int32 [B][K][6] = min d, min h, min w, max d, max h, max w; (D, H, W, -1, -1, -1) for an empty row.
 * A NaN voxel inside a labelled cluster makes that row's peak and argmax unspecified; nothing faults.  Integer atomics only
 * (add, min, max, compare-and-swap), so the bits depend on neither the grid nor the order of arrival.  The entry has no
 * workspace, so max / argmax is ONE 32-bit word per row: the index of the best voxel so far in the order of
 * (fc_key(s(a)) << 32) | ~index, raised by compare-and-swap (the key is read back from `a`).  Runs of equal labels inside a wave
 * are combined by shuffles, then in a 64-slot LDS cache of the workgroup, before memory is touched.  THREE launches whatever
 * the data (initialise, accumulate, peak values).
 *
 * Every pointer 4-byte aligned, coord_sum 8-byte, the workspace 16-byte (TMF_E_ALIGN).  Limits (TMF_E_SHAPE / TMF_E_ARG /
 * TMF_E_WORKSPACE, nothing launched): 1 <= B <= 65536; D, H, W >= 1 with V = D*H*W < 2^31 (and B * ceil(D/8) * ceil(H/8) *
 * ceil(W/32), B * ceil(V/2048) and B*K/256 below 2^31: one workgroup each - shapes that do not fit a device's memory anyway);
 * mode in 0..2; connectivity 6, 18 or 26; min_size >= 1; 1 <= K <= V. */
#define TMF_CLUSTER_POS 0
#define TMF_CLUSTER_NEG 1
#define TMF_CLUSTER_ABS 2
size_t tmf_cluster_workspace_bytes(int B, int D, int H, int W);
int    tmf_cluster_label(const float* a, const float* thr, int* labels, int* n_clusters, void* workspace, size_t workspace_bytes,
                         int B, int D, int H, int W, int mode, int connectivity, int min_size, void* stream);
int    tmf_cluster_table(const float* a, const int* labels, int* size, float* peak, int* argmax, int64_t* coord_sum, int* bbox,
                         int B, int D, int H, int W, int mode, int K, void* stream);

/* ------------------------------------------------------------------------------
 * Gaussian smoothing of volumes and voxel maps (csrc/smooth.hip): the separable 3-D Gaussian filter of
 * scipy.ndimage.gaussian_filter, optionally normalised inside a mask.  The reference has no such function; this entry replaces
 * what its user writes with stock ops - F.pad plus three F.conv3d calls with 1-D kernels, whose result depends on the
 * convolution algorithm the backend picks, or a copy to the host - for a blurred baseline (tmf_mask_by_rank's `base`, the
 * blurred-input baseline of integrated gradients) and for smoothing an attribution map before tmf_cluster_label / tmf_region_stats.
 *
 * a [B][D][H][W] float, W fastest -> out of the same shape, EVERY element written; out must not overlap a.
 * Taps.  Per axis a sigma in voxels, >= 0, and one truncate > 0.  sigma == 0: the axis is not filtered (r = 0, one tap 1).
 * Otherwise r = (int)(truncate*sigma + 0.5) and w[i] = exp(-0.5*i*i/sigma^2), i = -r..r, computed in double, divided by their
 * double sum (tmf_gaussian_taps_f64), then rounded once to float (tmf_gaussian_taps) - scipy's kernel.  r <=
 * TMF_SMOOTH_MAX_RADIUS; a larger radius is refused with TMF_E_ARG.
 * Border.  The source index for output o and tap i on an axis of extent n is j = o + i, mapped by mode:
 *   TMF_SMOOTH_REFLECT   p = j mod 2n (non-negative), source p if p < n, else 2n-1-p: d c b a | a b c d | d c b a (scipy's
 *                        default "reflect"), valid for any r, including r >= n and n == 1;
 *   TMF_SMOOTH_CONSTANT  a tap with j outside 0..n-1 contributes 0;
 *   TMF_SMOOTH_NEAREST   j clamped to 0..n-1.
 * Result.  The three 1-D filters are applied one after another in fp32 - W, then H, then D -, each output element a chain of
 * fused multiply-adds from 0.0f in ascending tap order.  The bits are a function of the shape and the arguments alone: two
 * calls give the same bits, a sample filtered alone gives the bits it has at any batch position, and the 16-byte path gives
 * the bits of the one-element path.  No atomics, no workgroup waits for another.
 * Error bound.  The weights are positive and sum to 1 within rounding, each pass is a K = 2r+1 term fp32 dot product.  With
 * E = the sum over the filtered axes of (2*r_axis + 4) and peak_b = max |a[b]|:
 *     |out - exact| <= E * 2^-24 * peak_b,
 * exact = the fp64 filter with the double taps.  A zero map gives exact zeros, a map without negative values no negative output.
 * Mask (may be NULL).  mask [D][H][W] int32, ONE for all samples (the convention of tmf_region_stats' atlas): a voxel is inside
 * where mask != 0, so an atlas or a label volume of tmf_cluster_label is a mask as it is.  With m the 0/1 inside indicator:
 *     out = G(a*m) / G(m) inside, 0 outside,
 * G the filter above under the chosen border mode - normalised convolution: values outside never enter, the weights are
 * renormalised near the edge.  Inside, G(m) >= w_d[0]*w_h[0]*w_w[0] > 0.  Bound: (2*E + 2) * 2^-24 * max |a[b]*m|.
 * All three sigmas 0 is allowed: a copy without a mask, a*m with one.
 * NaN and +-inf propagate as the arithmetic has it: the values written are then unspecified, but nothing faults.
 * Passes.  TWO launches whatever the data, no memset, no host synchronisation, no allocation; the taps travel by value in the
 * kernel arguments (3 x 65 floats: no host-to-device copy).  Launch 1 filters W and H on tiles of one d-plane in LDS, the
 * border mode applied as the tile and its halo are loaded, and writes the intermediate; launch 2 filters D on slabs of planes
 * in LDS.  With a mask, launch 1 also writes G_hw(m) - once, by the workgroups of sample 0 - and launch 2 filters it along D
 * and divides; the mask is read once per launch.  16 bytes per lane where W % 4 == 0 and a, out (and mask) are 16-byte aligned,
 * one element per lane otherwise.
 * workspace: tmf_smooth_workspace_bytes(B, D, H, W, masked) bytes = the intermediate, B*D*H*W floats (rounded up to 16 bytes),
 * plus D*H*W floats (likewise) with a mask; 0 for a shape the entry refuses; 16-byte aligned; the entry need not find it zeroed.
 *
 * tmf_gaussian_taps / tmf_gaussian_taps_f64: HOST arrays; write the 2r+1 taps of (sigma, truncate) and return r >= 0, or a
 * TMF_E_*: TMF_E_ARG for a sigma that is negative or not finite, a truncate that is not a finite number > 0, a radius above the
 * limit and a capacity below 2r+1.  THE definition of the taps: the entry calls it, and so does the package's stock-torch twin.
 *
 * a, out and mask 4-byte aligned, the workspace 16-byte (TMF_E_ALIGN).  Limits (TMF_E_SHAPE / TMF_E_ARG / TMF_E_WORKSPACE,
 * nothing launched): 1 <= B <= 65536; D, H, W >= 1 with D*H*W < 2^31; mode in 0..2; sigmas finite and >= 0, truncate finite
 * and > 0, every radius <= TMF_SMOOTH_MAX_RADIUS; out overlapping a (TMF_E_ARG). */
#define TMF_SMOOTH_REFLECT    0
#define TMF_SMOOTH_CONSTANT   1
#define TMF_SMOOTH_NEAREST    2
#define TMF_SMOOTH_MAX_RADIUS 32
int    tmf_gaussian_taps(double sigma, double truncate, float* taps, int capacity);
int    tmf_gaussian_taps_f64(double sigma, double truncate, double* taps, int capacity);
size_t tmf_smooth_workspace_bytes(int B, int D, int H, int W, int masked);
int    tmf_gaussian_smooth(const float* a, const int* mask, float* out, double sigma_d, double sigma_h, double sigma_w,
                           double truncate, int mode, void* workspace, size_t workspace_bytes, int B, int D, int H, int W,
                           void* stream);

/* ------------------------------------------------------------------------------
 * RISE saliency maps (csrc/rise.hip; Petsiuk et al., RISE, 2018): score the network on the volume under N smooth random
 * masks, add the masks up weighted by their scores.  Black-box like occlusion, but at voxel resolution and with no patch size
 * to choose.  The reference has no such function; these entries replace the loop its user writes with stock ops: an upsample,
 * a crop and a multiply per mask - twice, once to perturb and once to accumulate - or N full-resolution masks kept in memory.
 *
 * Geometry.  Per axis with extent S and s cells, 1 <= s <= S: cell size c = ceil(S / s), n = s + 2 nodes.  A mask m owns a
 * node grid g_m[n_d][n_h][n_w] of bytes 0 / 1 and a shift t_m[3] with 0 <= t_a < c_a.  For voxel coordinate v_a:
 * q = v_a + t_a, i_a = q / c_a (i_a + 1 <= s + 1 always holds), r_a = q % c_a, w1_a = float(r_a) * invc_a with
 * invc_a = 1.0f / float(c_a) computed once on the host, w0_a = 1.0f - w1_a.
 * Mask value.  Every operation is rounded on its own, nothing is contracted:
 *     x[a][b] = g[i_d+a][i_h+b][i_w] * w0_w + g[i_d+a][i_h+b][i_w+1] * w1_w
 *     y[a]    = x[a][0] * w0_h + x[a][1] * w1_h
 *     M       = y[0] * w0_d + y[1] * w1_d
 * so W is interpolated first, then H, then D.  E[M(v)] = p exactly for every voxel, 0 <= M <= 1 + 2^-22, and
 * |M - M_exact| <= 16 * 2^-24, M_exact the same interpolation with weights r / c in fp64.
 * Nodes and shifts.  Philox4x32-10 under the key (seed_lo ^ 0x52495345, seed_hi ^ 0x6D61736B).  The node with linear index
 * e = (i_d * n_h + i_h) * n_w + i_w takes word e & 3 of counter (e >> 2, m, 0, 0) and is 1 iff
 * float(word >> 8) < float(p) * 2^24.  The shift of axis a is (word_a * c_a) >> 32 in 64-bit arithmetic, from counter
 * (0, m, 1, 0).  Grids and shifts are a pure function of (seed, m, geometry, p): independent of N, of the chunking and of the call.
 * Jobs.  Job j = b * N + m is sample b under mask m; the masks are shared by the samples.  The perturbed volume is
 * out = f + M * (vol - f), each operation rounded on its own, f = base[b][v] where a `base` volume is given (a blurred copy,
 * for example), else fill[b].  With f = 0 this is M * vol bit for bit, the RISE of the paper.
 * Map.  sal[b][v] = scale * sum_m scores[b][m] * M_m(v) over m = m_first, m_first + m_step, ... < N: an fp32 chain in
 * ascending m from 0.0f (one rounded product and one rounded sum per term), then ONE multiplication by scale.  No atomics: two
 * calls give the same bits, a sample alone gives the bits it has inside a batch.  With n terms,
 *     |sal - exact| <= scale * (n + 18) * 2^-24 * sum_m |scores[b][m]|     per voxel,
 * exact with M_exact and fp64 sums.
 *
 * tmf_rise_geometry: HOST arrays cell3[3], nodes3[3]; returns the bytes of one node grid, n_d*n_h*n_w, or a negative TMF_E_*.
 * tmf_rise_masks: nodes [N][n_d][n_h][n_w] bytes and shifts [N][3] int32 of masks m0 .. m0+N-1.  ONE launch.
 * tmf_rise_apply: out [K][D][H][W] for jobs j0 .. j0+K-1 (nodes / shifts hold masks 0 .. N-1); a chunk may straddle samples.
 *   ONE launch; 16 bytes per lane where D*H*W % 4 == 0 and vol, out (and base) are 16-byte aligned, one element per lane
 *   otherwise, with equal bits on both paths.
 * tmf_rise_accumulate: scores [B][N] -> sal [B][D][H][W], EVERY element written.  ONE launch: a workgroup owns a tile of
 *   voxels, rebuilds every mask in registers from node grids staged in LDS and feeds up to 8 samples' accumulators per
 *   evaluation (a larger B in groups of 8); a grid-stride loop over the tiles bounds the grid.
 * Refusals (negative code, nothing launched, the buffers untouched).  TMF_E_NULL: a null pointer, except fill where base is
 * given and base where fill is given.  TMF_E_SHAPE: an extent below 1, D*H*W >= 2^31 or a node grid of 2^31 bytes or more; B
 * outside 1..65536; B*N >= 2^31.  TMF_E_ARG: s outside 1..S; p outside (0, 1) or not finite; N < 1, m0 < 0, m0 + N >= 2^31;
 * K outside 1..65536, j0 < 0 or j0 + K > B*N; m_step < 1 or m_first outside 0..N-1; out overlapping vol.  TMF_E_ALIGN: a
 * float or int32 pointer that is not 4-byte aligned. */
int    tmf_rise_geometry(int D, int H, int W, int sd, int sh, int sw, int* cell3, int* nodes3);
int    tmf_rise_masks(unsigned char* nodes, int* shifts, int D, int H, int W, int sd, int sh, int sw, float p,
                      unsigned long long seed, int m0, int N, void* stream);
int    tmf_rise_apply(const float* vol, const unsigned char* nodes, const int* shifts, const float* fill, const float* base,
                      float* out, int B, int D, int H, int W, int sd, int sh, int sw, int N, int j0, int K, void* stream);
int    tmf_rise_accumulate(const float* scores, const unsigned char* nodes, const int* shifts, float* sal, float scale, int B,
                           int D, int H, int W, int sd, int sh, int sw, int N, int m_first, int m_step, void* stream);

/* ------------------------------------------------------------------------------
 * Atlas-region Shapley values (csrc/shap.hip; KernelSHAP, Lundberg & Lee 2017, in the paired-sampling form of Covert & Lee
 * 2021): the players are the atlas regions of the volumes, a coalition keeps its members and replaces the other regions, and
 * a least-squares fit under the efficiency constraint gives every player its share of score(scan) - score(all replaced).  The
 * reference has no such function; these entries replace the loop its user writes with stock ops: a sampler, one torch.where
 * per coalition and volume, and a dense solve.
 *
 * Players.  P players, 2 <= P <= TMF_SHAP_MAX_PLAYERS (= TMF_REGION_MAX).  A coalition is a bitset of Wd = ceil(P / 32) uint32
 * words: player i is bit i & 31 of word i >> 5; the padding bits are 0 in every row, complements included.
 * Coalition m.  Philox4x32-10 under the key (seed_lo ^ 0x53484150, seed_hi ^ 0x636F616C).  paired = 1: k = m >> 1 and an odd m
 * is the complement of row m - 1 over the P players; paired = 0: k = m.
 *   Size.  u = word 0 of counter (0, k, 1, 0); s = 1 + #{t in 0..P-3 : thr[t] <= u}, so 1 <= s <= P - 1.  thr is the table of
 *     tmf_shap_size_table: w_r = 1.0 / ((double)r * (double)(P - r)) for r = 1..P-1, F_s = (w_1 + ... + w_s, added in
 *     ascending r in fp64) / (the total, added the same way), thr[t] = min(2^32 - 1, floor(2^32 * F_{t+1})): the Shapley
 *     kernel's distribution of sizes.  P = 2 has no thresholds and s = 1.
 *   Members.  key_i = word i & 3 of counter (i >> 2, k, 0, 0).  Player i is in the coalition iff fewer than s players j have
 *     (key_j, j) < (key_i, i) lexicographically: a uniform subset of size s, ties resolved by index.
 *   Row m is a pure function of (seed, m, P, paired): independent of N, of m0 and of the call.
 * Jobs.  Job j = b * N + m is sample b under row m of an [N][Wd] array (the caller may append rows of its own, an all-zero
 * one for the empty coalition).  `labels` is an int32 volume [D][H][W] shared by the samples, as in tmf_occlude_labels; p0 is
 * the first player of this volume, label l belongs to player p0 + l - 1.  Per voxel v with l = labels[v]:
 *     out = vol[b][v]   if l <= 0, or l > R, or bit (p0 + l - 1) of the row is set;
 *     out = f           otherwise, f = base[b][v] where a base is given, else fill[b].
 * A pure select, the bits of torch.where.  Background is never replaced: the all-ones row gives the volume itself.
 * Fit.  z_mi = bit i of row m, y[b][m] = (double)scores[b][m] - (double)offset[b].  A[i][j] = sum_m z_mi * z_mj in int32,
 * exact.  rhs[b][i] = the sum of y[b][m] over the m with z_mi = 1, an fp64 chain in ascending m from 0.0.  No atomics: two
 * calls give the same bits.
 * Solve.  In fp64: M = A + ridge * I = L L^T (Cholesky), X = M^-1 [rhs_1 .. rhs_B, 1], and
 *     phi_b = x_b - x_1 * (sum(x_b) - delta[b]) / sum(x_1),
 * the minimiser of sum_m (y_m - sum_i z_mi phi_i)^2 subject to sum_i phi_i = delta[b].  info[0] = 0: solved; otherwise the
 * 1-based index of the first pivot <= 0 (A is singular: too few coalitions for P) and every phi is NaN - not an error code.
 * Two calls give the same bits.  Error: a Cholesky solve of M x = r has the relative forward error <= cond_2(M) * gamma with
 * gamma ~ 3 P u to first order (u = 2^-53; Higham, Accuracy and Stability of Numerical Algorithms, Theorem 10.4 with
 * || |L||L^T| || ~ ||M||).  phi takes two such solves (x_b and x_1): 6 P u; a reference solved in fp64 by another
 * factorisation carries an error of the same size: 12 P u; rounded up to the next power of two,
 *     |phi - phi_ref| <= 16 * P * 2^-53 * cond_2(M) * max|phi_ref|     per sample.
 *
 * tmf_shap_size_table: HOST array thr[max(P - 2, 0)] (thr may be NULL for P = 2).  No launch.
 * tmf_shap_coalitions: coal [N][Wd], rows m0 .. m0+N-1; thr: the table in DEVICE memory (NULL allowed for P = 2).  ONE
 *   launch; with `paired` an odd m0 or N is allowed.
 * tmf_shap_apply: out [K][D][H][W] for jobs j0 .. j0+K-1 (coal holds rows 0 .. N-1); a chunk may straddle samples.  ONE
 *   launch: a workgroup reads its voxels of vol, labels and base once per run of jobs of a sample and writes them once per job; 16 bytes
 *   per lane where D*H*W % 4 == 0 and vol, out, labels (and base) are 16-byte aligned, one element per lane otherwise, with
 *   equal bits on both paths.
 * tmf_shap_gram: coal [N][Wd], scores [B][N], offset [B] -> A [P][P] int32 and rhs [B][P] fp64, EVERY element written.  Two
 *   launches.
 * tmf_shap_solve_workspace: the bytes tmf_shap_solve needs (0 for B or P outside their limits).
 * tmf_shap_solve: A, rhs [B][P], delta [B] -> phi [B][P] fp64 and info[1], EVERY element written.  A fixed sequence of
 *   launches (two per panel of 32 columns, three more), no cooperative grid.
 * Refusals (negative code, nothing launched, the buffers untouched).  TMF_E_NULL: a null pointer, except fill where base is
 * given, base where fill is given, and thr for P = 2.  TMF_E_SHAPE: P outside 2..TMF_SHAP_MAX_PLAYERS; an extent below 1 or
 * D*H*W >= 2^31; B outside 1..65536; B*N >= 2^31.  TMF_E_ARG: paired not 0 / 1; N < 1, m0 < 0, m0 + N >= 2^31; R < 1, p0 < 0,
 * p0 + R > P; K outside 1..65536, j0 < 0 or j0 + K > B*N; a ridge that is negative or not finite; out overlapping vol.
 * TMF_E_ALIGN: a float, int32 or uint32 pointer that is not 4-byte aligned, a double pointer that is not 8-byte aligned, a
 * workspace that is not 16-byte aligned.  TMF_E_WORKSPACE: fewer bytes than tmf_shap_solve_workspace(B, P). */
#define TMF_SHAP_MAX_PLAYERS 1024     /* = TMF_REGION_MAX */
int    tmf_shap_size_table(int P, unsigned* thr);
int    tmf_shap_coalitions(unsigned* coal, const unsigned* thr, int P, int paired, unsigned long long seed, int m0, int N,
                           void* stream);
int    tmf_shap_apply(const float* vol, const int* labels, const unsigned* coal, const float* fill, const float* base, float* out,
                      int B, int D, int H, int W, int R, int p0, int P, int N, int j0, int K, void* stream);
int    tmf_shap_gram(const unsigned* coal, const float* scores, const float* offset, int* A, double* rhs, int B, int P, int N,
                     void* stream);
size_t tmf_shap_solve_workspace(int B, int P);
int    tmf_shap_solve(const int* A, const double* rhs, const double* delta, double ridge, double* phi, int* info, void* workspace,
                      size_t workspace_bytes, int B, int P, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TMF_HIP_H */
