// rise_mask.h — THE mask evaluation of the RISE kernels (csrc/rise.hip; include/tmf_hip.h states the formula): the apply and the
// accumulate kernel rebuild a mask value from node bytes, a shift and the voxel's coordinates through the functions below and
// through nothing else, so that a perturbed volume and the map are built from the same bits.  A file that includes this header
// is compiled with -ffp-contract=off (build.FILE_FLAGS): every * + - below is one rounded operation.
#pragma once
#include "tmf_common.h"

// One axis: extent S, cell size c = ceil(S / s), n = s + 2 nodes, invc = 1.0f / float(c) from the host.
struct RiseAxis {
    int S, c, n;
    float invc;
};
struct RiseGeom {
    RiseAxis d, h, w;
    int V;          // D*H*W
    int G;          // bytes of one node grid, n_d*n_h*n_w
};

// r = q % c -> w1 = float(r) * invc, w0 = 1.0f - w1
__device__ __forceinline__ void rise_weights(int r, float invc, float& w0, float& w1) {
    w1 = (float)r * invc;
    w0 = 1.0f - w1;
}

// M of the header: g = the mask's node grid (global memory or LDS), at = (i_d*n_h + i_h)*n_w + i_w, plane = n_h*n_w, row = n_w.
// W first, then H, then D.  The nodes are 0 / 1, so every product is 0 or the weight itself.
__device__ __forceinline__ float rise_mask_value(const unsigned char* g, int at, int plane, int row, float w0d, float w1d,
                                                 float w0h, float w1h, float w0w, float w1w) {
    const unsigned char* p = g + at;
    const float x00 = (float)p[0] * w0w + (float)p[1] * w1w;
    const float x01 = (float)p[row] * w0w + (float)p[row + 1] * w1w;
    const float x10 = (float)p[plane] * w0w + (float)p[plane + 1] * w1w;
    const float x11 = (float)p[plane + row] * w0w + (float)p[plane + row + 1] * w1w;
    const float y0 = x00 * w0h + x01 * w1h;
    const float y1 = x10 * w0h + x11 * w1h;
    return y0 * w0d + y1 * w1d;
}
