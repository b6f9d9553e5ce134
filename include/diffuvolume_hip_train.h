/* diffuvolume_hip_train.h -- C ABI of libdiffuvolume_hip.so, second table: training entries that arrived after the
 * inference table of diffuvolume_hip.h was closed over by its tests.
 *
 * The entries live in the same library and follow the same rules; they are declared apart because every name of
 * diffuvolume_hip.h must be a row of the inference arena table (tests/test_gpu_abi_arena.py) or an exclusion next to it,
 * and the decision about a training entry's pointer and bounds contract is recorded beside the training tests instead
 * (tests/test_regress_train_host.py).  Bound by `_lib.TRAIN_SIGNATURES`.  Each entry names the reference code it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions (those of diffuvolume_hip.h)
 *  - every pointer is a DEVICE pointer to a dense, contiguous row-major tensor in
 *    the reference's own layout (NCHW / NCDHW); outputs are caller-allocated;
 *  - nothing here allocates, frees, synchronises or keeps global mutable state;
 *    calls are re-entrant and are enqueued on `stream` of the current device;
 *  - alignment: a tensor operand needs only the alignment of its element type (4 bytes for float).  No entry of this
 *    header selects code by the alignment of an operand: an offset view gives the same bits;
 *  - every element of an output is written exactly once, in a fixed summation order, without atomics: the same inputs give
 *    the same bits on every launch, and a batch gives the bits of its items run one by one;
 *  - a refused call launches nothing and writes nothing;
 *  - return value: 0 = ok, <0 = DV_ERR_* (bad argument), >0 = hipError_t.
 */
#ifndef DIFFUVOLUME_HIP_TRAIN_H
#define DIFFUVOLUME_HIP_TRAIN_H

#include "diffuvolume_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- regression tail, backward ------------------------------------------------------------------------------------
 * Gradient of dv_upsample_softmax_regress_f32 with respect to its cost: what autograd computes in training for
 *   F.interpolate(cost, [4D,4h,4w], mode='trilinear') + F.softmax(dim=1) + disparity_regression
 * (SceneFlow/models/acv_ddim.py:457-480 with submodule.py:173-177, four heads; KITTI12/models/pwcnet_ddim.py:682-710,
 * five heads, align_corners=1), where it keeps a [B,4D,4h,4w] softmax per head until backward and adds the trilinear
 * gradient with atomics.  Here the softmax is recomputed from `cost`; nothing of size [B,4D,4h,4w] exists.
 *   cost [B,D,h,w], disp [B,4h,4w] (the forward's output), grad_disp [B,4h,4w] -> dcost [B,D,h,w]
 *   dv_k = g p_k (k - disp);  dc_d = sum_k (l0 [i0(k)=d] + l1 [i1(k)=d]) dv_k;  dcost = the bilinear taps' transpose of dc.
 * grad_disp == 0 at a pixel contributes exactly 0 from it; NaN / Inf in grad_disp or cost propagate.
 * D == 48 with a cost below 2^31 bytes (the forward's predicate) is one fused kernel and takes no workspace;
 * any other D <= 128, or a larger volume, goes through `workspace` (dv_..._workspace_floats floats, [B,D,4h,4w]) in two
 * passes.  D > 128 on that route: DV_ERR_UNSUPPORTED.  `workspace` may be NULL where the size is 0.
 * The workspace is 16 times the cost: for D == 48 it is asked for only at 2^31 bytes of cost and more, i.e. 32 GiB and
 * more.  The two-pass route is tested at small D; a D == 48 volume of that size has not been run. */
size_t dv_upsample_softmax_regress_bwd_workspace_floats(int B, int D, int h, int w);
int dv_upsample_softmax_regress_bwd_f32(const float* cost, const float* disp, const float* grad_disp, float* dcost,
                                        float* workspace, int B, int D, int h, int w, int align_corners,
                                        dv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFUVOLUME_HIP_TRAIN_H */
