// clusters.hip — connected clusters of thresholded voxel maps (include/tmf_hip.h states the semantics): the label volume of the
// clusters of every sample, numbered in raster order of their first voxel (tmf_cluster_label), and the cluster table - size, peak,
// peak index, coordinate sums and bounding box per cluster (tmf_cluster_table).  gfx950.
//
// Labelling is union-find by lowest index: the root of a cluster is its lowest linear voxel index, a parent never lies above its
// child, and a union points the larger of two roots at the smaller with atomicMin - roots only ever decrease, so no lane waits
// for another and every chain ends.  Launches of tmf_cluster_label, each handing over to the next at the launch boundary:
//   1 tile      one workgroup labels one CL_TD x CL_TH x CL_TW tile in LDS and writes parent[v] = the global index of the
//               tile-local root (-1: background), size[v] = 0
//   2 boundary  every pair of foreground neighbours in different tiles is united in global memory
//   3 flatten   root[v] = the end of v's chain, written into `labels` (a SEPARATE array); size[root] += 1 (runs of one root
//               combined inside a wave, then in the workgroup's LDS slots, then integer atomics)
//   4 count     per chunk of CL_CHUNK voxels the number of roots with size >= min_size
//   5 scan      one workgroup per sample: exclusive prefix sum of the chunk counts, n_clusters
//   6 number    number[v] = 1 + the rank of a surviving root in raster order, else 0 (over `parent`, which is no longer needed)
//   7 write     labels[v] = number[root[v]], 0 for background
// plus ONE hipMemsetAsync of the status words in front: eight stream operations whatever the data.
//
// Coherence.  In launch 2 `parent` is written by other workgroups, possibly on another XCD, whose L2 a plain load does not see:
// EVERY access to it there is a relaxed agent-scope atomic.  All other arrays are read only in a later launch than the one that
// wrote them.  Every chain-following loop is bounded (by the tile size in LDS, by V in memory); a lane that exceeds the bound
// sets status[b], which turns n_clusters[b] into -1, and leaves the loop.
#include "tmf_device.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;

constexpr int CL_THREADS = 256;
constexpr int CL_TD = 8, CL_TH = 8, CL_TW = 32;            // the LDS tile, W-major
constexpr int CL_TILE = CL_TD * CL_TH * CL_TW;             // 2048 voxels: 8 KiB of parents
constexpr int CL_PER = CL_TILE / CL_THREADS;
constexpr int CL_CHUNK = 2048;                             // voxels of a workgroup in the flat launches
constexpr int CL_ITEMS = CL_CHUNK / CL_THREADS;
constexpr int CL_MAX_B = 1 << 16;

#define CL_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

struct ClGeom {
    int D, H, W, V;
    int nth, ntw, ntiles;       // tiles along h and w, tiles of a sample
    int nchunks;                // chunks of a sample
};

// s(a): the value a cluster is thresholded and ranked by
__device__ __forceinline__ float cl_score(float a, int mode) { return mode == TMF_CLUSTER_POS ? a : mode == TMF_CLUSTER_NEG ? -a : fabsf(a); }

// the 13 neighbours that lie BEFORE a voxel in raster order, restricted to |dd| + |dh| + |dw| <= maxnz (1: faces, 2: + edges,
// 3: + corners).  Every pair of neighbours is met once, from its later voxel.
template <class F> __device__ __forceinline__ void cl_backward(int maxnz, F f) {
#pragma unroll
    for (int o = 0; o < 13; ++o) {
        const int dd = o < 9 ? -1 : 0;
        const int dh = o < 9 ? o / 3 - 1 : (o < 12 ? -1 : 0);
        const int dw = o < 9 ? o % 3 - 1 : (o < 12 ? o - 10 : -1);
        const int nz = (dd != 0) + (dh != 0) + (dw != 0);
        if (nz <= maxnz) f(dd, dh, dw);
    }
}

// ---- union-find in LDS (one tile) --------------------------------------------------------------------------------------------
__device__ __forceinline__ int cl_lds_find(int* sp, int x, bool& bad) {
    for (int t = 0; t <= CL_TILE; ++t) {
        const int p = __hip_atomic_load(&sp[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
    bad = true;
    return x;
}

__device__ __forceinline__ void cl_lds_union(int* sp, int x, int y, bool& bad) {
    for (int t = 0; t <= CL_TILE; ++t) {
        x = cl_lds_find(sp, x, bad);
        y = cl_lds_find(sp, y, bad);
        if (x == y || bad) return;
        if (x < y) { const int s = x; x = y; y = s; }
        const int old = atomicMin(&sp[x], y);       // x > y: point the larger root at the smaller
        if (old == x) return;
        x = old;                                    // x had a parent by now: go on from there (old < x, so max(x, y) falls)
    }
    bad = true;
}

// ---- union-find in memory (launch 2: atomics only) -----------------------------------------------------------------------------
__device__ __forceinline__ int cl_find_atomic(int* parent, int x, int bound, bool& bad) {
    for (int t = 0; t <= bound; ++t) {
        const int p = CL_LOAD(&parent[x]);
        if (p == x) return x;
        x = p;
    }
    bad = true;
    return x;
}

__device__ __forceinline__ void cl_union(int* parent, int x, int y, int bound, bool& bad) {
    for (int t = 0; t <= bound; ++t) {
        x = cl_find_atomic(parent, x, bound, bad);
        y = cl_find_atomic(parent, y, bound, bad);
        if (x == y || bad) return;
        if (x < y) { const int s = x; x = y; y = s; }
        const int old = atomicMin(&parent[x], y);
        if (old == x) return;
        x = old;
    }
    bad = true;
}

// Launch 1.  Workgroup blockIdx.x = b*ntiles + tile.
__global__ __launch_bounds__(CL_THREADS) void cluster_tile_kernel(const float* __restrict__ a, const float* __restrict__ thr,
                                                                  int* __restrict__ parent, int* __restrict__ size,
                                                                  int* __restrict__ status, ClGeom g, int mode, int maxnz) {
    __shared__ int sp[CL_TILE];
    const int b = blockIdx.x / g.ntiles, tile = blockIdx.x - b * g.ntiles;
    const int td = tile / (g.nth * g.ntw), th = tile / g.ntw % g.nth, tw = tile % g.ntw;
    const long d0 = (long)td * CL_TD, h0 = (long)th * CL_TH, w0 = (long)tw * CL_TW;
    const size_t off = (size_t)b * g.V;
    const float t = thr[b];
    for (int k = 0; k < CL_PER; ++k) {
        const int i = k * CL_THREADS + threadIdx.x;
        const long d = d0 + i / (CL_TH * CL_TW), h = h0 + i / CL_TW % CL_TH, w = w0 + i % CL_TW;   // long: up to extent + 31
        int p = -1;
        if (d < g.D && h < g.H && w < g.W) {
            const size_t v = off + ((size_t)d * g.H + h) * g.W + w;
            if (cl_score(a[v], mode) >= t) p = i;            // false for a NaN voxel and for a NaN threshold
            size[v] = 0;
        }
        sp[i] = p;
    }
    __syncthreads();
    bool bad = false;
    for (int k = 0; k < CL_PER; ++k) {
        const int i = k * CL_THREADS + threadIdx.x;
        if (sp[i] < 0) continue;                                // the sign of a parent never changes
        const int ld = i / (CL_TH * CL_TW), lh = i / CL_TW % CL_TH, lw = i % CL_TW;
        cl_backward(maxnz, [&](int dd, int dh, int dw) {
            const int nd = ld + dd, nh = lh + dh, nw = lw + dw;
            if (nd < 0 || nh < 0 || nh >= CL_TH || nw < 0 || nw >= CL_TW) return;
            const int n = (nd * CL_TH + nh) * CL_TW + nw;
            if (sp[n] >= 0) cl_lds_union(sp, i, n, bad);
        });
    }
    __syncthreads();
    for (int k = 0; k < CL_PER; ++k) {
        const int i = k * CL_THREADS + threadIdx.x;
        const long d = d0 + i / (CL_TH * CL_TW), h = h0 + i / CL_TW % CL_TH, w = w0 + i % CL_TW;   // long: up to extent + 31
        if (d >= g.D || h >= g.H || w >= g.W) continue;
        int r = -1;
        if (sp[i] >= 0) {
            const int l = cl_lds_find(sp, i, bad);              // no writes to sp behind the barrier
            r = (int)(((d0 + l / (CL_TH * CL_TW)) * g.H + h0 + l / CL_TW % CL_TH) * g.W + w0 + l % CL_TW);
        }
        parent[off + ((size_t)d * g.H + h) * g.W + w] = r;
    }
    if (bad) atomicOr(&status[b], 1);
}

// Launch 2.  The same grid; only voxels with a backward neighbour in another tile act.
__global__ __launch_bounds__(CL_THREADS) void cluster_boundary_kernel(int* parent, int* __restrict__ status, ClGeom g, int maxnz) {
    const int b = blockIdx.x / g.ntiles, tile = blockIdx.x - b * g.ntiles;
    const int td = tile / (g.nth * g.ntw), th = tile / g.ntw % g.nth, tw = tile % g.ntw;
    int* par = parent + (size_t)b * g.V;
    bool bad = false;
    for (int k = 0; k < CL_PER; ++k) {
        const int i = k * CL_THREADS + threadIdx.x;
        const int ld = i / (CL_TH * CL_TW), lh = i / CL_TW % CL_TH, lw = i % CL_TW;
        if (ld > 0 && lh > 0 && lh < CL_TH - 1 && lw > 0 && lw < CL_TW - 1) continue;      // every backward neighbour in the tile
        const long dl = (long)td * CL_TD + ld, hl = (long)th * CL_TH + lh, wl = (long)tw * CL_TW + lw;
        if (dl >= g.D || hl >= g.H || wl >= g.W) continue;
        const int d = (int)dl, h = (int)hl, w = (int)wl;
        const int v = (d * g.H + h) * g.W + w;
        if (CL_LOAD(&par[v]) < 0) continue;
        cl_backward(maxnz, [&](int dd, int dh, int dw) {
            const int nld = ld + dd, nlh = lh + dh, nlw = lw + dw;
            if (nld >= 0 && nlh >= 0 && nlh < CL_TH && nlw >= 0 && nlw < CL_TW) return;        // united in LDS
            const int nd = d + dd, nh = h + dh, nw = w + dw;
            if (nd < 0 || nh < 0 || nh >= g.H || nw < 0 || nw >= g.W) return;
            const int n = (nd * g.H + nh) * g.W + nw;
            if (CL_LOAD(&par[n]) >= 0) cl_union(par, v, n, g.V, bad);
        });
    }
    if (bad) atomicOr(&status[b], 1);
}

// the lanes lane .. end of a wave that share `key` with their left neighbours form a run headed by `lane`
__device__ __forceinline__ bool cl_run(int key, int lane, int& end) {
    const int before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    const u64 heads = __ballot(head);
    const u64 after = lane == 63 ? 0ull : heads >> (lane + 1);
    end = after ? lane + __ffsll((long long)after) - 1 : 63;
    return head;
}

// A workgroup keeps up to CL_CACHE keys (roots, table rows) in LDS: a run's first lane claims the slot key % CL_CACHE for its key
// by compare-and-swap and adds there; a run whose slot belongs to another key goes to memory itself.  The slots are flushed by
// global atomics at the end, so a cluster that fills the workgroup's voxels costs memory one visit, not one per run.
constexpr int CL_CACHE = 64;

__device__ __forceinline__ bool cl_claim(int* tag, int key) {
    const int t = atomicCAS(&tag[key & (CL_CACHE - 1)], -1, key);
    return t == -1 || t == key;
}

// Launch 3.  Workgroup blockIdx.x = b*nchunks + chunk; `parent` is final, plain loads.
__global__ __launch_bounds__(CL_THREADS) void cluster_flatten_kernel(const int* __restrict__ parent, int* __restrict__ root,
                                                                     int* __restrict__ size, int* __restrict__ status, ClGeom g) {
    __shared__ int tag[CL_CACHE], cnt[CL_CACHE];
    const int b = blockIdx.x / g.nchunks, chunk = blockIdx.x - b * g.nchunks;
    const size_t off = (size_t)b * g.V;
    const int* par = parent + off;
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < CL_CACHE) { tag[threadIdx.x] = -1; cnt[threadIdx.x] = 0; }
    __syncthreads();
    bool bad = false;
    for (int k = 0; k < CL_ITEMS; ++k) {                    // the same trips for every lane: shuffles inside
        const long i = (long)chunk * CL_CHUNK + k * CL_THREADS + threadIdx.x;
        int r = -1;
        if (i < g.V) {
            r = par[i];
            if (r >= 0) {
                int t = 0;
                for (; t <= g.V; ++t) {
                    const int p = par[r];
                    if (p == r) break;
                    r = p;
                }
                bad = bad || t > g.V;
            }
            root[off + i] = r;
        }
        int end;
        const bool head = cl_run(r, lane, end);              // neighbouring voxels mostly share a root: one atomic per run
        if (head && r >= 0) {
            if (cl_claim(tag, r)) atomicAdd(&cnt[r & (CL_CACHE - 1)], end - lane + 1);
            else atomicAdd(&size[off + r], end - lane + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < CL_CACHE && tag[threadIdx.x] >= 0) atomicAdd(&size[off + tag[threadIdx.x]], cnt[threadIdx.x]);
    if (bad) atomicOr(&status[b], 1);
}

__device__ __forceinline__ int cl_block_sum(int x, int* sw) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = x;
    __syncthreads();
    return sw[0] + sw[1] + sw[2] + sw[3];
}

// exclusive prefix of x over the workgroup; total = the sum
__device__ __forceinline__ int cl_block_scan(int x, int* sw, int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                        // sw may still be read from the previous round
    if (lane == 63) sw[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int q = 0; q < wave; ++q) base += sw[q];
    total = sw[0] + sw[1] + sw[2] + sw[3];
    return base + inc - x;
}

// the flags of the thread's CL_ITEMS CONSECUTIVE voxels as a bit mask
__device__ __forceinline__ unsigned cl_flags(const int* __restrict__ root, const int* __restrict__ size, long first, int V, int min_size) {
    unsigned m = 0;
    for (int q = 0; q < CL_ITEMS; ++q) {
        const long i = first + q;
        if (i < V && root[i] == (int)i && size[i] >= min_size) m |= 1u << q;
    }
    return m;
}

// Launch 4.
__global__ __launch_bounds__(CL_THREADS) void cluster_count_kernel(const int* __restrict__ root, const int* __restrict__ size,
                                                                   int* __restrict__ counts, ClGeom g, int min_size) {
    __shared__ int sw[4];
    const int b = blockIdx.x / g.nchunks, chunk = blockIdx.x - b * g.nchunks;
    const size_t off = (size_t)b * g.V;
    const unsigned m = cl_flags(root + off, size + off, (long)chunk * CL_CHUNK + threadIdx.x * CL_ITEMS, g.V, min_size);
    const int n = cl_block_sum(__popc(m), sw);
    if (threadIdx.x == 0) counts[blockIdx.x] = n;
}

// Launch 5.  One workgroup per sample: counts -> exclusive prefix, in place (a thread reads and writes its own elements).
__global__ __launch_bounds__(CL_THREADS) void cluster_scan_kernel(int* __restrict__ counts, const int* __restrict__ status,
                                                                  int* __restrict__ n_clusters, ClGeom g) {
    __shared__ int sw[4];
    const int b = blockIdx.x;
    int* c = counts + (size_t)b * g.nchunks;
    int carry = 0;
    for (int base = 0; base < g.nchunks; base += CL_THREADS) {
        const int i = base + threadIdx.x;
        const int x = i < g.nchunks ? c[i] : 0;
        int total;
        const int ex = cl_block_scan(x, sw, total);
        if (i < g.nchunks) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) n_clusters[b] = status[b] ? -1 : carry;
}

// Launch 6.
__global__ __launch_bounds__(CL_THREADS) void cluster_number_kernel(const int* __restrict__ root, const int* __restrict__ size,
                                                                    const int* __restrict__ counts, int* __restrict__ number,
                                                                    ClGeom g, int min_size) {
    __shared__ int sw[4];
    const int b = blockIdx.x / g.nchunks, chunk = blockIdx.x - b * g.nchunks;
    const size_t off = (size_t)b * g.V;
    const long first = (long)chunk * CL_CHUNK + threadIdx.x * CL_ITEMS;
    const unsigned m = cl_flags(root + off, size + off, first, g.V, min_size);
    int total;
    int next = counts[blockIdx.x] + cl_block_scan(__popc(m), sw, total) + 1;
    for (int q = 0; q < CL_ITEMS; ++q) {
        if (first + q >= g.V) break;
        number[off + first + q] = (m >> q & 1u) ? next++ : 0;
    }
}

// Launch 7.  A thread reads root[v] out of labels[v] and writes the same element; number is another array.
__global__ __launch_bounds__(CL_THREADS) void cluster_write_kernel(const int* __restrict__ number, int* labels, ClGeom g) {
    const int b = blockIdx.x / g.nchunks, chunk = blockIdx.x - b * g.nchunks;
    const size_t off = (size_t)b * g.V;
    for (int k = 0; k < CL_ITEMS; ++k) {
        const long i = (long)chunk * CL_CHUNK + k * CL_THREADS + threadIdx.x;
        if (i >= g.V) break;
        const int r = labels[off + i];
        labels[off + i] = r >= 0 ? number[off + r] : 0;
    }
}

// ---- the cluster table ---------------------------------------------------------------------------------------------------------
// `slot` ([B][K] int32, argmax where given, else peak's words) holds the index of the best voxel so far, -1 for none.

__global__ __launch_bounds__(CL_THREADS) void cluster_table_init_kernel(int* __restrict__ size, int* __restrict__ slot,
                                                                        long long* __restrict__ coord_sum, int* __restrict__ bbox,
                                                                        long n, int D, int H, int W) {
    const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n) return;
    if (size) size[i] = 0;
    if (slot) slot[i] = -1;
    if (coord_sum) { coord_sum[3 * i] = 0; coord_sum[3 * i + 1] = 0; coord_sum[3 * i + 2] = 0; }
    if (bbox) {
        int* q = bbox + 6 * i;
        q[0] = D; q[1] = H; q[2] = W; q[3] = -1; q[4] = -1; q[5] = -1;
    }
}

__device__ __forceinline__ u64 cl_shfl_down(u64 v, int d) {
    const unsigned lo = (unsigned)__shfl_down((int)(unsigned)v, d), hi = (unsigned)__shfl_down((int)(unsigned)(v >> 32), d);
    return ((u64)hi << 32) | lo;
}

// One combined record (n voxels, best M, coordinate sums, box) into row `at` of the outputs.  max / argmax: the order of
// (fc_key(s(a)) << 32) | ~index, kept in memory as the INDEX alone (the key is read back from `src`, which does not change) and
// raised by compare-and-swap; a failed swap means the slot rose, so the loop ends after at most V trips.
__device__ __forceinline__ void cl_commit(const float* __restrict__ src, int* size, int* slot, u64* coord_sum, int* bbox, size_t at,
                                          int n, u64 M, u64 sd, u64 sh, u64 sw, const int* lo, const int* hi, int mode, int V) {
    if (size) atomicAdd(&size[at], n);
    if (coord_sum) {
        atomicAdd(&coord_sum[3 * at], sd); atomicAdd(&coord_sum[3 * at + 1], sh); atomicAdd(&coord_sum[3 * at + 2], sw);
    }
    if (bbox) {
        int* q = bbox + 6 * at;
        atomicMin(&q[0], lo[0]); atomicMin(&q[1], lo[1]); atomicMin(&q[2], lo[2]);
        atomicMax(&q[3], hi[0]); atomicMax(&q[4], hi[1]); atomicMax(&q[5], hi[2]);
    }
    if (slot) {
        const unsigned mykey = (unsigned)(M >> 32);
        const int mine = (int)~(unsigned)M;
        int cur = CL_LOAD(&slot[at]);
        for (int t = 0; t <= V; ++t) {
            if ((unsigned)cur < (unsigned)V) {
                const unsigned ck = fc_key(cl_score(src[cur], mode));
                if (ck > mykey || (ck == mykey && cur <= mine)) break;
            }
            const int prev = atomicCAS(&slot[at], cur, mine);
            if (prev == cur) break;
            cur = prev;
        }
    }
}

// Workgroup blockIdx.x = b*nchunks + chunk.  The lanes of a wave walk neighbouring voxels, which mostly share a label: every run
// of equal labels is combined by a segmented shuffle reduction, its first lane adds the record to the workgroup's LDS slot of
// that row (cl_claim; to memory where the slot is taken), and the slots go to memory at the end.
__global__ __launch_bounds__(CL_THREADS) void cluster_table_kernel(const float* __restrict__ a, const int* __restrict__ labels,
                                                                   int* size, int* slot, u64* coord_sum, int* bbox, ClGeom g,
                                                                   int mode, int K) {
    __shared__ int tag[CL_CACHE], cn[CL_CACHE], clo[3][CL_CACHE], chi[3][CL_CACHE];
    __shared__ u64 cM[CL_CACHE], cs[3][CL_CACHE];
    const int b = blockIdx.x / g.nchunks, chunk = blockIdx.x - b * g.nchunks;
    const size_t off = (size_t)b * g.V;
    const float* src = a + off;
    const int lane = threadIdx.x & 63;
    const int HW = g.H * g.W;
    if (threadIdx.x < CL_CACHE) {
        const int c = threadIdx.x;
        tag[c] = -1; cn[c] = 0; cM[c] = 0;
        cs[0][c] = 0; cs[1][c] = 0; cs[2][c] = 0;
        clo[0][c] = g.D; clo[1][c] = g.H; clo[2][c] = g.W;
        chi[0][c] = -1; chi[1][c] = -1; chi[2][c] = -1;
    }
    __syncthreads();
    for (int k = 0; k < CL_ITEMS; ++k) {                    // the same trips for every lane: shuffles inside
        const long i = (long)chunk * CL_CHUNK + k * CL_THREADS + threadIdx.x;
        int key = -1;
        if (i < g.V) {
            const int l = labels[off + i];
            key = (unsigned)(l - 1) < (unsigned)K ? l - 1 : -1;            // before any index is formed from it
        }
        if (__ballot(key >= 0) == 0ull) continue;                          // wave-uniform
        u64 M = 0, sd = 0, sh = 0, sw = 0;
        int lo[3] = {g.D, g.H, g.W}, hi[3] = {-1, -1, -1};
        if (key >= 0) {
            const int v = (int)i, d = v / HW, h = (v - d * HW) / g.W, w = v - d * HW - h * g.W;
            M = ((u64)fc_key(cl_score(src[v], mode)) << 32) | (unsigned)~(unsigned)v;
            sd = d; sh = h; sw = w;
            lo[0] = hi[0] = d; lo[1] = hi[1] = h; lo[2] = hi[2] = w;
        }
        int end;
        const bool head = cl_run(key, lane, end);
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const u64 tM = cl_shfl_down(M, s), td = cl_shfl_down(sd, s), th = cl_shfl_down(sh, s), tw = cl_shfl_down(sw, s);
            int tlo[3], thi[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) { tlo[c] = __shfl_down(lo[c], s); thi[c] = __shfl_down(hi[c], s); }
            if (lane + s <= end) {
                M = max(M, tM); sd += td; sh += th; sw += tw;
#pragma unroll
                for (int c = 0; c < 3; ++c) { lo[c] = min(lo[c], tlo[c]); hi[c] = max(hi[c], thi[c]); }
            }
        }
        if (!head || key < 0) continue;
        if (cl_claim(tag, key)) {
            const int c = key & (CL_CACHE - 1);
            atomicAdd(&cn[c], end - lane + 1);
            atomicMax(&cM[c], M);
            atomicAdd(&cs[0][c], sd); atomicAdd(&cs[1][c], sh); atomicAdd(&cs[2][c], sw);
#pragma unroll
            for (int q = 0; q < 3; ++q) { atomicMin(&clo[q][c], lo[q]); atomicMax(&chi[q][c], hi[q]); }
        } else {
            cl_commit(src, size, slot, coord_sum, bbox, (size_t)b * K + key, end - lane + 1, M, sd, sh, sw, lo, hi, mode, g.V);
        }
    }
    __syncthreads();
    if (threadIdx.x < CL_CACHE && tag[threadIdx.x] >= 0) {
        const int c = threadIdx.x;
        const int lo[3] = {clo[0][c], clo[1][c], clo[2][c]}, hi[3] = {chi[0][c], chi[1][c], chi[2][c]};
        cl_commit(src, size, slot, coord_sum, bbox, (size_t)b * K + tag[c], cn[c], cM[c], cs[0][c], cs[1][c], cs[2][c], lo, hi, mode, g.V);
    }
}

// peak = the value at the best index, NaN for an empty row; argmax already holds the index or -1
__global__ __launch_bounds__(CL_THREADS) void cluster_table_final_kernel(const float* __restrict__ a, const int* slot, float* peak,
                                                                         long n, int K, int V) {
    const long i = (long)blockIdx.x * CL_THREADS + threadIdx.x;
    if (i >= n || !peak) return;
    const int idx = slot[i];
    peak[i] = (unsigned)idx < (unsigned)V ? a[(size_t)(i / K) * V + idx] : __uint_as_float(0x7FC00000u);
}

// ---- host side ----

bool cl_al(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// false where the entries refuse the shape
bool cl_geom(int B, int D, int H, int W, ClGeom& g) {
    if (B < 1 || B > CL_MAX_B || D < 1 || H < 1 || W < 1) return false;
    const long long V = (long long)D * H * W;
    if (V > INT_MAX || (long long)D * H > INT_MAX) return false;
    g.D = D; g.H = H; g.W = W; g.V = (int)V;
    const long long ntd = ((long long)D + CL_TD - 1) / CL_TD;
    g.nth = (int)(((long long)H + CL_TH - 1) / CL_TH);
    g.ntw = (int)(((long long)W + CL_TW - 1) / CL_TW);
    const long long ntiles = ntd * g.nth * g.ntw;
    g.nchunks = (int)((V + CL_CHUNK - 1) / CL_CHUNK);
    if (ntiles * B > INT_MAX || (long long)g.nchunks * B > INT_MAX) return false;      // one workgroup each
    g.ntiles = (int)ntiles;
    return true;
}

// workspace: parent int [B][V] | size int [B][V] | counts int [B][nchunks] | status int [B]
size_t cl_cells(int B, const ClGeom& g) { return (size_t)B * (size_t)g.V; }

}  // namespace

extern "C" size_t tmf_cluster_workspace_bytes(int B, int D, int H, int W) {
    ClGeom g;
    if (!cl_geom(B, D, H, W, g)) return 0;
    const size_t n = (2 * cl_cells(B, g) + (size_t)B * g.nchunks + (size_t)B) * sizeof(int);
    return (n + 15) & ~(size_t)15;
}

extern "C" int tmf_cluster_label(const float* a, const float* thr, int* labels, int* n_clusters, void* workspace,
                                 size_t workspace_bytes, int B, int D, int H, int W, int mode, int connectivity, int min_size,
                                 void* stream) {
    TMF_REQUIRE_PTR(a); TMF_REQUIRE_PTR(thr); TMF_REQUIRE_PTR(labels); TMF_REQUIRE_PTR(n_clusters); TMF_REQUIRE_PTR(workspace);
    ClGeom g;
    TMF_REQUIRE(cl_geom(B, D, H, W, g), TMF_E_SHAPE,
                "%s: B = %d (1 .. %d), D, H, W = %d, %d, %d (>= 1, D*H*W < 2^31, B * tiles < 2^31)", __func__, B, CL_MAX_B, D, H, W);
    TMF_REQUIRE(mode >= TMF_CLUSTER_POS && mode <= TMF_CLUSTER_ABS, TMF_E_ARG, "%s: mode = %d (0 .. 2)", __func__, mode);
    TMF_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, TMF_E_ARG, "%s: connectivity = %d (6, 18 or 26)",
                __func__, connectivity);
    TMF_REQUIRE(min_size >= 1, TMF_E_ARG, "%s: min_size = %d (>= 1)", __func__, min_size);
    TMF_REQUIRE(cl_al(a, 4) && cl_al(thr, 4) && cl_al(labels, 4) && cl_al(n_clusters, 4), TMF_E_ALIGN,
                "%s: a pointer is not 4-byte aligned", __func__);
    TMF_REQUIRE_ALIGNED(workspace);
    const size_t need = tmf_cluster_workspace_bytes(B, D, H, W);
    TMF_REQUIRE(workspace_bytes >= need, TMF_E_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", __func__, workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    int* parent = static_cast<int*>(workspace);
    int* size = parent + cl_cells(B, g);
    int* counts = size + cl_cells(B, g);
    int* status = counts + (size_t)B * g.nchunks;
    const int maxnz = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    hipError_t e = hipMemsetAsync(status, 0, (size_t)B * sizeof(int), s);
    if (e != hipSuccess) {
        tmf_set_error("%s: clearing the status words failed: %s", __func__, hipGetErrorString(e));
        return (int)e;
    }
    const dim3 block(CL_THREADS), tiles(B * g.ntiles), chunks(B * g.nchunks);
    hipLaunchKernelGGL(cluster_tile_kernel, tiles, block, 0, s, a, thr, parent, size, status, g, mode, maxnz);
    hipLaunchKernelGGL(cluster_boundary_kernel, tiles, block, 0, s, parent, status, g, maxnz);
    hipLaunchKernelGGL(cluster_flatten_kernel, chunks, block, 0, s, parent, labels, size, status, g);
    hipLaunchKernelGGL(cluster_count_kernel, chunks, block, 0, s, labels, size, counts, g, min_size);
    hipLaunchKernelGGL(cluster_scan_kernel, dim3(B), block, 0, s, counts, status, n_clusters, g);
    hipLaunchKernelGGL(cluster_number_kernel, chunks, block, 0, s, labels, size, counts, parent, g, min_size);
    hipLaunchKernelGGL(cluster_write_kernel, chunks, block, 0, s, parent, labels, g);
    return tmf_launch_result(__func__);
}

extern "C" int tmf_cluster_table(const float* a, const int* labels, int* size, float* peak, int* argmax, int64_t* coord_sum,
                                 int* bbox, int B, int D, int H, int W, int mode, int K, void* stream) {
    TMF_REQUIRE_PTR(a); TMF_REQUIRE_PTR(labels);
    ClGeom g;
    TMF_REQUIRE(cl_geom(B, D, H, W, g), TMF_E_SHAPE,
                "%s: B = %d (1 .. %d), D, H, W = %d, %d, %d (>= 1, D*H*W < 2^31, B * chunks < 2^31)", __func__, B, CL_MAX_B, D, H, W);
    TMF_REQUIRE(mode >= TMF_CLUSTER_POS && mode <= TMF_CLUSTER_ABS, TMF_E_ARG, "%s: mode = %d (0 .. 2)", __func__, mode);
    TMF_REQUIRE(K >= 1 && K <= g.V, TMF_E_ARG, "%s: K = %d rows (1 .. D*H*W = %d)", __func__, K, g.V);
    const long n = (long)B * K;
    TMF_REQUIRE((n + CL_THREADS - 1) / CL_THREADS <= INT_MAX, TMF_E_SHAPE, "%s: B * K = %ld rows are more than one launch holds", __func__, n);
    TMF_REQUIRE(cl_al(a, 4) && cl_al(labels, 4) && cl_al(size, 4) && cl_al(peak, 4) && cl_al(argmax, 4) && cl_al(bbox, 4) &&
                    cl_al(coord_sum, 8),
                TMF_E_ALIGN, "%s: a pointer is not 4-byte (coord_sum: 8-byte) aligned", __func__);
    hipStream_t s = (hipStream_t)stream;
    int* slot = argmax ? argmax : reinterpret_cast<int*>(peak);
    const dim3 block(CL_THREADS), rows((unsigned)((n + CL_THREADS - 1) / CL_THREADS));
    hipLaunchKernelGGL(cluster_table_init_kernel, rows, block, 0, s, size, slot, reinterpret_cast<long long*>(coord_sum), bbox, n, D,
                       H, W);
    hipLaunchKernelGGL(cluster_table_kernel, dim3(B * g.nchunks), block, 0, s, a, labels, size, slot,
                       reinterpret_cast<u64*>(coord_sum), bbox, g, mode, K);
    hipLaunchKernelGGL(cluster_table_final_kernel, rows, block, 0, s, a, slot, peak, n, K, g.V);
    return tmf_launch_result(__func__);
}
