/* diffuvolume_hip_amp3d_bf16.h -- C ABI of libdiffuvolume_hip.so, fifth table: the three products of the 3x3x3 stride-1
 * convolutions of the ACV and PCW aggregation stacks in mixed-precision training at train precision "bf16", on the bf16
 * matrix instruction v_mfma_f32_16x16x32_bf16.  The twins of the fourth table (diffuvolume_hip_amp3d.h, "f16"): the same
 * signatures, the same kernels (csrc/conv3d_mp.h, csrc/conv3d_wgrad_mp.h) instantiated for the other element type.
 *
 * Bound by `_lib.AMP3D_BF16_SIGNATURES`, where every entry also carries the decision about its pointer and bounds contract
 * ("size only" or the GPU test that holds it); tests/test_amp3d_bf16_host.py reads that table.
 *
 * Arithmetic (the whole specification of the kernels).  Tensors are float32 in memory in both directions.  rb16 is
 * round-to-nearest-even to bfloat16, done by the hardware conversion (v_cvt_pk_bf16_f32) while an operand is staged.  NaN
 * stays NaN.  A finite float32 above about 3.3895e38 rounds to Inf; below that the range is float32's, so there is no
 * loss scaling and no skipped step.  A product of two bf16 numbers is exact in fp32 unless it leaves the fp32 exponent
 * range; sums are fp32; NO output is rounded to bf16.
 *   forward          y  = conv(rb16(x), rb16(w)) (+ bias)
 *   input gradient   dx = conv(rb16(g), rb16(w')),  w' = w.flip(2,3,4).transpose(0,1): the same entry with transpose_flip = 1
 *   weight gradient  dW[co,ci,t] = sum rb16(g) rb16(x)
 * Operands below 2^-126 (bf16 subnormals) may be flushed to zero.
 * Everything else is as at fp16: the summation order, the tap pairing, the dummy tap slot with zero weights, Cout >= 2,
 * the shape refusals.
 *
 * Conventions (those of diffuvolume_hip.h)
 *  - every pointer is a DEVICE pointer to a dense, contiguous row-major tensor (NCDHW; weights [Cout,Cin,3,3,3]); outputs
 *    and the workspace are caller-allocated;
 *  - nothing here allocates, frees, synchronises or keeps global mutable state; there is no packed-weight image and no
 *    tuning hook; calls are re-entrant and are enqueued on `stream` of the current device;
 *  - alignment: 4 bytes for every operand.  The forward entry stores 16 bytes at a time when W % 4 == 0 and `out` lies on
 *    a 16-byte line and one float at a time otherwise: the same bits either way;
 *  - every element of an output is written exactly once, in a fixed summation order, without atomics: the bits are a
 *    function of the shape only, and a batch gives the forward bits of its items run one by one;
 *  - a refused call launches nothing and writes nothing;
 *  - return value: 0 = ok, <0 = DV_ERR_* (bad argument), >0 = hipError_t.
 */
#ifndef DIFFUVOLUME_HIP_AMP3D_BF16_H
#define DIFFUVOLUME_HIP_AMP3D_BF16_H

#include "diffuvolume_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Conv3d(k = 3, stride 1, padding 1), forward and input gradient --------------------------------------------------
 *   in [B,Cin,D,H,W], bias [Cout] or NULL -> out [B,Cout,D,H,W]
 *   transpose_flip = 0: w is [Cout,Cin,3,3,3], the module's raw float32 weight;
 *   transpose_flip = 1: w is [Cin,Cout,3,3,3] (the weight of the layer whose input gradient this is, `in` being its
 *                       output gradient) and the kernel reads it as w.flip(2,3,4).transpose(0,1).
 * Any B, D, H, W, Cin >= 1; Cout >= 2 (Cout == 1: DV_ERR_UNSUPPORTED, the single-channel heads keep their float32
 * kernels); k != 3: DV_ERR_UNSUPPORTED; D*H*W > 2^29 - 1 or Cout*Cin*27 > 2^31 - 1: DV_ERR_SHAPE. */
int dv_conv3d_k3s1_bf16_f32(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int D, int H,
                            int W, int Cout, int k, int transpose_flip, dv_stream_t stream);

/* ---- Conv3d(k = 3, stride 1, padding 1), weight gradient -------------------------------------------------------------
 *   x [B,Cin,D,H,W], g [B,Cout,D,H,W] -> dw [Cout,Cin,3,3,3]
 * Split-K as dv_conv3d_wgrad_f16_f32, with its workspace plan: bricks of 2 x 2 x 32 output positions in one sequence over
 * the batch, split into contiguous ranges; every split writes its partial into `workspace` ([splits][Cout,Cin,27],
 * dv_conv3d_wgrad_bf16_workspace_floats floats, at most 48 MB), a second launch sums the splits in split order.
 * Non-finite operands, as at fp16: the positions of a brick that lie outside the volume are staged as g = 0 (and x = 0)
 * and multiplied like any other.  An Inf or NaN of x (a float32 that rounds to Inf included) whose window reaches such a
 * position -- next to the far edge of a volume that is no multiple of the brick -- meets a 0 of g: NaN in taps of dW of
 * that INPUT channel where the exact sum has no such product.  This is the one departure from the contract above.  It
 * stays inside the input channel's entries dw[:, ci]; an Inf of g stays in dw[co].
 * The size entry returns 0 for a shape the launching entry refuses (DV_ERR_SHAPE): a dimension < 1, D*H*W >= 2^30,
 * Cout*Cin*27 floats beyond the workspace bound. */
size_t dv_conv3d_wgrad_bf16_workspace_floats(int B, int Cin, int D, int H, int W, int Cout);
int dv_conv3d_wgrad_bf16_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D, int H,
                             int W, int Cout, dv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
