// Launch interface of the fused per-instance transformer kernels: defined in xformer_fused.hip, called by fusion_path.hip
// (C++ linkage, library-internal).  The one definition of the two io structs and of the launcher prototypes.
#ifndef TMF_XFORMER_LAUNCH_H
#define TMF_XFORMER_LAUNCH_H

#include "tmf_common.h"

struct tmf_xf_fwd_io {
    const float *x, *KR, *VC, *pk, *pkv_next, *mask_o, *mask_g, *mask_f;      // pk: this instance's forward pack buffer
    float *a, *QR, *QC, *out, *lse, *x1, *f, *h, *g, *x2, *y, *m1, *r1, *m2, *r2, *mf, *rf, *KRn, *KCn, *VRn, *VCn;
};
struct tmf_xf_bwd_io {
    const float *dy, *x, *KR, *KC, *VR, *pk, *mask_o, *mask_g, *mask_f;        // pk: this instance's backward pack buffer
    const float *QR, *QC, *out, *lse, *x1, *h, *x2, *m1, *r1, *m2, *r2, *mf, *rf;
    float *dx2, *dh, *dx1, *dq, *DR, *DC, *delta, *dx, *part, *dkv, *dctx;
    const float* dctx_acc;
};

bool tmf_xf_supported(int N, int dim, int heads, int dim_head, int mlp);
int tmf_xf_npad(int N);
int tmf_xf_tiles(int N);
int tmf_xf_part_stride(void);
int tmf_xf_pack_floats(void);
int tmf_xf_pack_kv_offset(void);
int tmf_xf_launch_pack(int n_inst, const tmf_xformer_params* inst, float* const* pk_fwd, float* const* pk_bwd, hipStream_t s);
int tmf_xf_launch_fwd(int B, int N, const tmf_xformer_params* w, const tmf_xf_fwd_io* io, float scale, int only_kv, int h2, int infer,
                      hipStream_t s);
int tmf_xf_launch_bwd(int B, int N, const tmf_xformer_params* w, const tmf_xf_bwd_io* io, float scale, int h2, hipStream_t s);
int tmf_xf_launch_colsum(int n_inst, const float* const* part, float* const* small, float* const* lnf, int nblk, hipStream_t s);

#endif
