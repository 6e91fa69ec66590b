// The one-launch optimizer steps (adam.hip, sgd.hip) share ONE copy of: the tensor table that rides in the kernel
// arguments, the chunk -> tensor search every workgroup does, the layout rule of the flat state buffers and the host loop
// that fills the table.  An update rule adds only its arithmetic and whatever per-tensor word it needs beside the table.
#pragma once
#include "tmf_common.h"

constexpr int TMF_OPT_CHUNK = 2048;            // elements per workgroup: 256 threads x 2 float4

struct TmfTensorTable {
    float* p[TMF_ADAM_MAX_TENSORS];
    const float* g[TMF_ADAM_MAX_TENSORS];
    int off[TMF_ADAM_MAX_TENSORS];             // element offset of the tensor's state in the flat buffers
    int first[TMF_ADAM_MAX_TENSORS + 1];       // first chunk of tensor i (prefix sums); first[n] = number of chunks
    int numel[TMF_ADAM_MAX_TENSORS];
    int n;
};
static_assert(sizeof(TmfTensorTable) <= 6144 - TMF_ADAM_MAX_TENSORS,
              "the table (plus one byte per tensor of an update rule's own) is a kernel argument (AMD kernarg segments are not limited to 4 KB)");

#ifdef __HIPCC__
// the tensor whose chunk range contains `chunk`
__device__ __forceinline__ int tmf_table_find(const TmfTensorTable& t, int chunk) {
    int lo = 0, hi = t.n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.first[mid] <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}
#endif

// elements tensor i occupies in a flat state buffer: every tensor's slice starts 16-byte aligned
static inline long tmf_state_padded(long numel) { return (numel + 3) & ~3L; }

// Fill the table from the caller's arrays: a tensor without a gradient (or without elements) is skipped, as torch skips a
// parameter without a gradient, but keeps its slice of the state.  src[k] (may be NULL): the caller's index of table row k.
// *chunks: workgroups to launch; t.n == 0: nothing to do.  Host code only: no device call.
static inline int tmf_table_fill(const char* who, int n, float* const* params, const float* const* grads, const long* numel,
                                 TmfTensorTable& t, int* chunks_out, int* src) {
    long off = 0;
    int chunks = 0, k = 0;
    for (int i = 0; i < n; ++i) {
        TMF_REQUIRE(numel[i] >= 0 && numel[i] < (1L << 31), TMF_E_SHAPE, "%s: tensor %d has %ld elements", who, i, numel[i]);
        if (grads[i] != nullptr && numel[i] > 0) {
            TMF_REQUIRE(params[i] != nullptr, TMF_E_NULL, "%s: parameter %d is NULL", who, i);
            t.p[k] = params[i]; t.g[k] = grads[i]; t.off[k] = (int)off; t.numel[k] = (int)numel[i]; t.first[k] = chunks;
            chunks += (int)((numel[i] + TMF_OPT_CHUNK - 1) / TMF_OPT_CHUNK);
            if (src != nullptr) src[k] = i;
            ++k;
        }
        off += tmf_state_padded(numel[i]);
        TMF_REQUIRE(off < (1L << 31), TMF_E_SHAPE, "%s: more than 2^31 elements of optimizer state", who);
    }
    t.first[k] = chunks;
    t.n = k;
    *chunks_out = chunks;
    return TMF_OK;
}
