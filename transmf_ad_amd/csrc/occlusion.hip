// occlusion.hip — occlusion sensitivity (include/tmf_hip.h states the semantics): the batch writer (tmf_occlude_windows,
// tmf_occlude_labels: K occluded copies of volumes in ONE launch, the bits of clone() plus slice assignment) and the map
// builder (tmf_occlusion_volume, tmf_occlusion_volume_labels: the per-window drops back on the voxel grid).  gfx950.
// Pure memory traffic: 16 bytes per lane where D*H*W % 4 == 0 and the pointers are 16-byte aligned, one element per lane
// otherwise; 64-bit element offsets between samples / jobs, 32-bit ones inside a volume (D*H*W < 2^31).  The map builder is
// a GATHER: every output voxel adds the drops of the windows that cover it in ascending window order and divides once by
// their count — no atomics, two calls give the same bits.  Grids follow the shape: about OCC_ITEMS 16-byte (or 4-byte) items
// per lane, capped at OCC_MAX_BLOCKS workgroups that then stride.
#include "tmf_common.h"
#include <limits.h>

namespace {

constexpr int OCC_THREADS = 256;
constexpr int OCC_ITEMS = 4;               // items a lane walks at least, the volume permitting
constexpr long OCC_MAX_BLOCKS = 1 << 16;   // workgroups of a launch over all jobs / samples

typedef int i32x4 __attribute__((ext_vector_type(4)));

// One axis of the window grid: n windows of `p` voxels every `s`, the last one cut at the extent S.  p arrives clamped to S
// (a larger patch is the same single window); a window starts inside the axis, (n-1)*s < S.
struct OccAxis {
    int S, p, s, n;
};
struct OccGeom {
    OccAxis d, h, w;
    int nW;          // d.n * h.n * w.n, or R for the label entries
    int V;           // D*H*W
};

__device__ __forceinline__ void occ_coords(int e, int H, int W, int& z, int& y, int& x) {
    const int HW = H * W;
    z = e / HW;
    const int r = e - z * HW;
    y = r / W;
    x = r - y * W;
}
__device__ __forceinline__ void occ_step(int H, int W, int& z, int& y, int& x) {
    if (++x == W) {
        x = 0;
        if (++y == H) {
            y = 0;
            ++z;
        }
    }
}

// voxel (z, y, x) lies in the window that starts at (z0, y0, x0) and spans (nz, ny, nx) voxels: three unsigned compares and
// two ANDs, no short-circuit branches.  (Written with && on six signed compares, the unrolled 16-byte loop came out of the
// compiler's if-conversion storing the fill into element 0 of a quad whose z and y were inside and whose x was not:
// tests/test_gpu_occlusion.py::test_occlude_windows_kernel caught it on the 4^3 case.  Keep this form.)
__device__ __forceinline__ bool occ_inside(int z, int y, int x, int z0, int y0, int x0, unsigned nz, unsigned ny, unsigned nx) {
    return ((unsigned)(z - z0) < nz) & ((unsigned)(y - y0) < ny) & ((unsigned)(x - x0) < nx);
}

// out[k][e] = vol[b][e], or fill[b] where voxel e lies in window w (LABELS: where labels[e] == w + 1), for job j0 + k = b*nW + w.
// Workgroup blockIdx.x = k*nblk + blk strides over the items of job k.
template <bool VEC, bool LABELS>
__global__ __launch_bounds__(OCC_THREADS) void occlude_kernel(const float* __restrict__ vol, const int* __restrict__ labels,
                                                              const float* __restrict__ fill, float* __restrict__ out,
                                                              OccGeom g, int j0, int nblk) {
    const int k = blockIdx.x / nblk, blk = blockIdx.x - k * nblk;
    const int j = j0 + k;
    const int b = j / g.nW, w = j - b * g.nW;
    const float f = fill[b];
    const float* src = vol + (size_t)b * g.V;
    float* dst = out + (size_t)k * g.V;
    int z0 = 0, y0 = 0, x0 = 0;                  // the window's first voxel
    unsigned nz = 0, ny = 0, nx = 0;            // ... and its extents: min(p, S - i*s), the last window of an axis may be cut
    if (!LABELS) {
        const int id = w / (g.h.n * g.w.n), r = w - id * (g.h.n * g.w.n);
        const int ih = r / g.w.n, iw = r - ih * g.w.n;
        z0 = id * g.d.s; y0 = ih * g.h.s; x0 = iw * g.w.s;
        nz = (unsigned)min(g.d.p, g.d.S - z0); ny = (unsigned)min(g.h.p, g.h.S - y0); nx = (unsigned)min(g.w.p, g.w.S - x0);
    }
    const int region = w + 1;
    const long step = (long)nblk * OCC_THREADS;
    if (VEC) {
        const long n4 = g.V >> 2;
        for (long i = (long)blk * OCC_THREADS + threadIdx.x; i < n4; i += step) {
            const int e = (int)(i << 2);
            f32x4 v = TmfIO<float, 4>::ld(src + e);
            if (LABELS) {
                const i32x4 l = *reinterpret_cast<const i32x4*>(labels + e);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = l[q] == region ? f : v[q];
            } else {
                int z, y, x;
                occ_coords(e, g.h.S, g.w.S, z, y, x);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = occ_inside(z, y, x, z0, y0, x0, nz, ny, nx) ? f : v[q];
                    occ_step(g.h.S, g.w.S, z, y, x);
                }
            }
            TmfIO<float, 4>::st(dst + e, v);
        }
    } else {
        for (long i = (long)blk * OCC_THREADS + threadIdx.x; i < g.V; i += step) {
            const int e = (int)i;
            float v = src[e];
            if (LABELS) {
                v = labels[e] == region ? f : v;
            } else {
                int z, y, x;
                occ_coords(e, g.h.S, g.w.S, z, y, x);
                v = occ_inside(z, y, x, z0, y0, x0, nz, ny, nx) ? f : v;
            }
            dst[e] = v;
        }
    }
}

// the windows of one axis that contain coordinate c: lo..hi, never empty (s <= p)
__device__ __forceinline__ void occ_cover(const OccAxis& a, int c, int& lo, int& hi) {
    const int t = c - a.p + 1;                       // ceil(t / s) for t > 0, else window 0
    lo = t > 0 ? (t + a.s - 1) / a.s : 0;
    hi = min(a.n - 1, c / a.s);
}

__device__ __forceinline__ float occ_mean_drop(const float* __restrict__ drops, const OccGeom& g, int z, int y, int x) {
    int dl, dh, hl, hh, wl, wh;
    occ_cover(g.d, z, dl, dh);
    occ_cover(g.h, y, hl, hh);
    occ_cover(g.w, x, wl, wh);
    float s = 0.f;
    for (int id = dl; id <= dh; ++id)
        for (int ih = hl; ih <= hh; ++ih) {
            const float* row = drops + ((long)id * g.h.n + ih) * g.w.n;
            for (int iw = wl; iw <= wh; ++iw) s += row[iw];        // ascending w = (id*nh + ih)*nw + iw
        }
    const int count = (dh - dl + 1) * (hh - hl + 1) * (wh - wl + 1);
    return s / (float)count;
}

// vmap[b][e] = the mean of drops[b][w] over the windows w that contain voxel e (LABELS: drops[b][labels[e] - 1], 0 on
// background and on labels outside 1..R).  Workgroup blockIdx.x = b*nblk + blk.
template <bool VEC, bool LABELS>
__global__ __launch_bounds__(OCC_THREADS) void occlusion_volume_kernel(const float* __restrict__ drops,
                                                                       const int* __restrict__ labels,
                                                                       float* __restrict__ vmap, OccGeom g, int nblk) {
    const int b = blockIdx.x / nblk, blk = blockIdx.x - b * nblk;
    const float* dr = drops + (size_t)b * g.nW;
    float* dst = vmap + (size_t)b * g.V;
    const long step = (long)nblk * OCC_THREADS;
    if (VEC) {
        const long n4 = g.V >> 2;
        for (long i = (long)blk * OCC_THREADS + threadIdx.x; i < n4; i += step) {
            const int e = (int)(i << 2);
            f32x4 v;
            if (LABELS) {
                const i32x4 l = *reinterpret_cast<const i32x4*>(labels + e);
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = (l[q] >= 1 && l[q] <= g.nW) ? dr[l[q] - 1] : 0.f;
            } else {
                int z, y, x;
                occ_coords(e, g.h.S, g.w.S, z, y, x);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    v[q] = occ_mean_drop(dr, g, z, y, x);
                    occ_step(g.h.S, g.w.S, z, y, x);
                }
            }
            TmfIO<float, 4>::st(dst + e, v);
        }
    } else {
        for (long i = (long)blk * OCC_THREADS + threadIdx.x; i < g.V; i += step) {
            const int e = (int)i;
            float v;
            if (LABELS) {
                const int l = labels[e];
                v = (l >= 1 && l <= g.nW) ? dr[l - 1] : 0.f;
            } else {
                int z, y, x;
                occ_coords(e, g.h.S, g.w.S, z, y, x);
                v = occ_mean_drop(dr, g, z, y, x);
            }
            dst[e] = v;
        }
    }
}

// ---- host side ----

// n = ceil(max(S - p, 0) / s) + 1; p clamped to S for the kernels
int occ_axis(const char* fn, char name, int S, int p, int s, OccAxis* a) {
    TMF_REQUIRE(S >= 1, TMF_E_SHAPE, "%s: extent %c = %d", fn, name, S);
    TMF_REQUIRE(p >= 1, TMF_E_ARG, "%s: patch %c = %d", fn, name, p);
    TMF_REQUIRE(s >= 1 && s <= p, TMF_E_ARG, "%s: stride %c = %d outside 1..patch (%d): voxels would lie in no window", fn,
                name, s, p);
    a->S = S;
    a->p = p < S ? p : S;
    a->s = s;
    a->n = S > p ? (int)(((long)S - p + s - 1) / s) + 1 : 1;
    return TMF_OK;
}

int occ_volume_size(const char* fn, int D, int H, int W, int* V) {
    TMF_REQUIRE(D >= 1 && H >= 1 && W >= 1, TMF_E_SHAPE, "%s: volume %d x %d x %d", fn, D, H, W);
    const long long v = (long long)D * H;            // (two ints: no overflow)
    TMF_REQUIRE(v <= INT_MAX / W, TMF_E_SHAPE, "%s: D*H*W = %d*%d*%d does not stay below 2^31", fn, D, H, W);
    *V = (int)(v * W);
    return TMF_OK;
}

int occ_grid_geom(const char* fn, int D, int H, int W, int pd, int ph, int pw, int sd, int sh, int sw, OccGeom* g) {
    TMF_TRY(occ_volume_size(fn, D, H, W, &g->V));
    TMF_TRY(occ_axis(fn, 'd', D, pd, sd, &g->d));
    TMF_TRY(occ_axis(fn, 'h', H, ph, sh, &g->h));
    TMF_TRY(occ_axis(fn, 'w', W, pw, sw, &g->w));
    g->nW = g->d.n * g->h.n * g->w.n;                 // <= D*H*W < 2^31: a window starts at a voxel of its own
    return TMF_OK;
}

int occ_label_geom(const char* fn, int D, int H, int W, int R, OccGeom* g) {
    TMF_TRY(occ_volume_size(fn, D, H, W, &g->V));
    TMF_REQUIRE(R >= 1, TMF_E_ARG, "%s: R = %d regions", fn, R);
    g->d = OccAxis{D, D, 1, 1};
    g->h = OccAxis{H, H, 1, 1};
    g->w = OccAxis{W, W, 1, 1};
    g->nW = R;
    return TMF_OK;
}

// jobs j0 .. j0 + K - 1 exist
int occ_jobs(const char* fn, int B, const OccGeom& g, int j0, int K) {
    TMF_REQUIRE(B >= 1, TMF_E_SHAPE, "%s: B = %d", fn, B);
    TMF_REQUIRE((long long)B * g.nW <= INT_MAX, TMF_E_SHAPE, "%s: B * nW = %d * %d does not stay below 2^31", fn, B, g.nW);
    TMF_REQUIRE(K >= 1 && j0 >= 0, TMF_E_ARG, "%s: jobs j0 = %d, K = %d", fn, j0, K);
    TMF_REQUIRE((long long)j0 + K <= (long long)B * g.nW, TMF_E_ARG, "%s: jobs %d .. %lld of %lld", fn, j0, (long long)j0 + K - 1,
                (long long)B * g.nW);
    return TMF_OK;
}

bool occ_f32(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
bool occ_vec(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// workgroups per job / sample: `items` strided by lanes that walk OCC_ITEMS each, `outer` jobs share OCC_MAX_BLOCKS
int occ_blocks(long items, int outer) {
    long n = (items + (long)OCC_THREADS * OCC_ITEMS - 1) / ((long)OCC_THREADS * OCC_ITEMS);
    long cap = OCC_MAX_BLOCKS / outer;
    if (cap < 1) cap = 1;
    return (int)(n < 1 ? 1 : n > cap ? cap : n);
}

template <bool LABELS>
int occ_write(const char* fn, const float* vol, const int* labels, const float* fill, float* out, const OccGeom& g, int j0,
              int K, hipStream_t s) {
    TMF_REQUIRE(K <= OCC_MAX_BLOCKS, TMF_E_ARG, "%s: K = %d jobs in one call (at most %ld)", fn, K, OCC_MAX_BLOCKS);
    const bool vec = g.V % 4 == 0 && occ_vec(vol) && occ_vec(out) && (!LABELS || occ_vec(labels));
    const int nblk = occ_blocks(vec ? g.V / 4 : g.V, K);
    if (vec)
        hipLaunchKernelGGL((occlude_kernel<true, LABELS>), dim3(K * nblk), dim3(OCC_THREADS), 0, s, vol, labels, fill, out, g, j0,
                           nblk);
    else
        hipLaunchKernelGGL((occlude_kernel<false, LABELS>), dim3(K * nblk), dim3(OCC_THREADS), 0, s, vol, labels, fill, out, g, j0,
                           nblk);
    return tmf_launch_result(fn);
}

template <bool LABELS>
int occ_map(const char* fn, const float* drops, const int* labels, float* vmap, int B, const OccGeom& g, hipStream_t s) {
    TMF_REQUIRE(B >= 1 && B <= OCC_MAX_BLOCKS, TMF_E_SHAPE, "%s: B = %d (1 .. %ld)", fn, B, OCC_MAX_BLOCKS);
    const bool vec = g.V % 4 == 0 && occ_vec(vmap) && (!LABELS || occ_vec(labels));
    const int nblk = occ_blocks(vec ? g.V / 4 : g.V, B);
    if (vec)
        hipLaunchKernelGGL((occlusion_volume_kernel<true, LABELS>), dim3(B * nblk), dim3(OCC_THREADS), 0, s, drops, labels, vmap, g,
                           nblk);
    else
        hipLaunchKernelGGL((occlusion_volume_kernel<false, LABELS>), dim3(B * nblk), dim3(OCC_THREADS), 0, s, drops, labels, vmap,
                           g, nblk);
    return tmf_launch_result(fn);
}

}  // namespace

extern "C" int tmf_occlusion_windows(int D, int H, int W, int pd, int ph, int pw, int sd, int sh, int sw) {
    OccGeom g;
    TMF_TRY(occ_grid_geom("tmf_occlusion_windows", D, H, W, pd, ph, pw, sd, sh, sw, &g));
    return g.nW;
}

extern "C" int tmf_occlude_windows(const float* vol, const float* fill, float* out, int B, int D, int H, int W, int pd, int ph,
                                   int pw, int sd, int sh, int sw, int j0, int K, void* stream) {
    TMF_REQUIRE_PTR(vol); TMF_REQUIRE_PTR(fill); TMF_REQUIRE_PTR(out);
    OccGeom g;
    TMF_TRY(occ_grid_geom(__func__, D, H, W, pd, ph, pw, sd, sh, sw, &g));
    TMF_TRY(occ_jobs(__func__, B, g, j0, K));
    TMF_REQUIRE(occ_f32(vol) && occ_f32(fill) && occ_f32(out), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    return occ_write<false>(__func__, vol, nullptr, fill, out, g, j0, K, (hipStream_t)stream);
}

extern "C" int tmf_occlude_labels(const float* vol, const int* labels, const float* fill, float* out, int B, int D, int H, int W,
                                  int R, int j0, int K, void* stream) {
    TMF_REQUIRE_PTR(vol); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(fill); TMF_REQUIRE_PTR(out);
    OccGeom g;
    TMF_TRY(occ_label_geom(__func__, D, H, W, R, &g));
    TMF_TRY(occ_jobs(__func__, B, g, j0, K));
    TMF_REQUIRE(occ_f32(vol) && occ_f32(labels) && occ_f32(fill) && occ_f32(out), TMF_E_ALIGN,
                "%s: a pointer is not 4-byte aligned", __func__);
    return occ_write<true>(__func__, vol, labels, fill, out, g, j0, K, (hipStream_t)stream);
}

extern "C" int tmf_occlusion_volume(const float* drops, float* vmap, int B, int D, int H, int W, int pd, int ph, int pw, int sd,
                                    int sh, int sw, void* stream) {
    TMF_REQUIRE_PTR(drops); TMF_REQUIRE_PTR(vmap);
    OccGeom g;
    TMF_TRY(occ_grid_geom(__func__, D, H, W, pd, ph, pw, sd, sh, sw, &g));
    TMF_REQUIRE(occ_f32(drops) && occ_f32(vmap), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    return occ_map<false>(__func__, drops, nullptr, vmap, B, g, (hipStream_t)stream);
}

extern "C" int tmf_occlusion_volume_labels(const float* drops, const int* labels, float* vmap, int B, int D, int H, int W, int R,
                                           void* stream) {
    TMF_REQUIRE_PTR(drops); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(vmap);
    OccGeom g;
    TMF_TRY(occ_label_geom(__func__, D, H, W, R, &g));
    TMF_REQUIRE(occ_f32(drops) && occ_f32(labels) && occ_f32(vmap), TMF_E_ALIGN, "%s: a pointer is not 4-byte aligned", __func__);
    return occ_map<true>(__func__, drops, labels, vmap, B, g, (hipStream_t)stream);
}
