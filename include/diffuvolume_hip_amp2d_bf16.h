/* diffuvolume_hip_amp2d_bf16.h -- C ABI of libdiffuvolume_hip.so, sixth table: IGEV's recurrent update block
 * (KITTI15/core/update.py:26-142) in mixed-precision training at train precision "bf16" -- the loop of
 * train_stereo.py:146-173 under `torch.autocast("cuda", dtype=torch.bfloat16)` -- on the bf16 matrix instruction
 * v_mfma_f32_16x16x32_bf16.  The twins of the fp16 entries of diffuvolume_hip.h (dv_conv2d_f16_*, dv_conv2d_1in_f16,
 * dv_gru_*_f16, dv_conv2d_wgrad_cat_f16*): the same signatures, the same kernel bodies (csrc/conv2d_mp.h,
 * csrc/conv2d_wgrad_cat_mp.h, csrc/gru_gates.h, csrc/update_glue.hip) instantiated for the other element type.
 *
 * Bound by `_lib.AMP2D_BF16_SIGNATURES`, where every entry also carries the decision about its pointer and bounds contract
 * ("size only", "packs weights" or the GPU test that holds it); tests/test_update_bf16_host.py reads that table.
 *
 * Arithmetic (the whole specification of the kernels): that of the fp16 twins, operation for operation, with rb16 in place
 * of r16.  Tensors are float32 in memory in both directions and hold bf16-exact values on the route.  rb16 is
 * round-to-nearest-even to bfloat16, done by the hardware conversion (v_cvt_pk_bf16_f32).  NaN stays NaN.  A finite float32
 * above about 3.3895e38 rounds to Inf; below that the range is float32's, so there is no loss scaling and no skipped step.
 *   convolution      input, weight and bias rounded while staged, products accumulated in fp32, then
 *                    v = rb16(acc + rb16(bias)); v = rb16(v + residual); v = rb16(act(v)); v = rb16(v * mul);
 *                    blend: v = rb16(rb16(rb16(1 - z) * h) + rb16(z * v))
 *   gates            rh = rb16(r * h);  out = rb16(rb16(rb16(1 - z) * h) + rb16(z * q))   (torch's bfloat16 arithmetic)
 *   weight gradient  dW[co,ci,ky,kx] = sum rb16(g) rb16(x), written as the UNROUNDED fp32 sum (a product of two bf16
 *                    numbers is exact in fp32 unless it leaves the fp32 exponent range)
 * This is what bf16 autocast does to the block, apart from the unrounded dW and the gate backward, which stays float32
 * (dv_gru_gates_bwd_*_f32), as does dv_conv2d_1in_wgrad_f32: the two deliberate differences of the "f16" route.
 * Operands below 2^-126 (bf16 subnormals) may be flushed to zero: the contract claims nothing about them.
 *
 * Sizes and the launch choice do not depend on the element type: the packed image has dv_conv2d_f16_packed_bytes bytes and
 * the K-split factor is dv_conv2d_f16_auto_kslices (diffuvolume_hip.h); there are no bf16 twins of those two, no tuning
 * hook and no environment switch.
 *
 * Conventions (those of diffuvolume_hip.h)
 *  - every pointer is a DEVICE pointer to a dense, contiguous row-major tensor (NCHW; weights [Cout,Cin,k,k]), except the
 *    HOST arrays `inputs` / `channels` of a virtual concatenation; outputs, scratch and workspace are caller-allocated;
 *  - nothing here allocates, frees, synchronises or keeps global mutable state; calls are re-entrant and are enqueued on
 *    `stream` of the current device;
 *  - alignment: 4 bytes for every float operand (the gate entries take their float4 form iff every pointer lies on a
 *    16-byte line: the same bits either way); the packed weight image: 16 bytes;
 *  - every element of an output is written exactly once, in a fixed summation order, without atomics: the bits are a
 *    function of the shape only, and a batch gives the forward bits of its items run one by one;
 *  - a refused call launches nothing and writes nothing;
 *  - return value: 0 = ok, <0 = DV_ERR_* (bad argument), >0 = hipError_t.
 */
#ifndef DIFFUVOLUME_HIP_AMP2D_BF16_H
#define DIFFUVOLUME_HIP_AMP2D_BF16_H

#include "diffuvolume_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Conv2d(k in {1, 3}, stride 1, dilation 1, "same" padding) over a virtual concatenation, forward and input gradient
 * Arguments, shapes and refusals as dv_conv2d_f16_pack_weights / dv_conv2d_f16_cat / _cat_ksplit / _cat_pair /
 * _cat_pair_ksplit: `inputs` / `channels` are HOST arrays of n_inputs (1..4; more: DV_ERR_UNSUPPORTED) sources; k other
 * than 1 or 3: DV_ERR_UNSUPPORTED; act NONE / RELU / SIGMOID / TANH; residual / mul / blend_z / blend_h are [B,Cout,H,W]
 * or NULL; the _ksplit forms take scratch of kslices * B * (Cout1 + Cout2) * H * W floats, 1 <= kslices <= 8.
 * dv_conv2d_bf16_pack_weights: w [Cout,Cin,k,k] fp32 -> the kernel's bf16 image (dv_conv2d_f16_packed_bytes bytes). */
int dv_conv2d_bf16_pack_weights(const float* w, void* wpacked, int Cin, int Cout, int k, dv_stream_t stream);
int dv_conv2d_bf16_cat(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                       const float* bias, const float* residual, const float* mul, const float* blend_z,
                       const float* blend_h, float* out, int B, int H, int W, int Cout, int k, int act,
                       dv_stream_t stream);
int dv_conv2d_bf16_cat_ksplit(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                              const float* bias, const float* residual, const float* mul, const float* blend_z,
                              const float* blend_h, float* out, float* scratch, int kslices, int B, int H, int W,
                              int Cout, int k, int act, dv_stream_t stream);
int dv_conv2d_bf16_cat_pair(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                            const float* bias, const float* residual1, const float* mul1, float* out1,
                            const float* residual2, const float* mul2, float* out2, int B, int H, int W, int Cout1,
                            int Cout2, int act, dv_stream_t stream);
int dv_conv2d_bf16_cat_pair_ksplit(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                                   const float* bias, const float* residual1, const float* mul1, float* out1,
                                   const float* residual2, const float* mul2, float* out2, float* scratch, int kslices,
                                   int B, int H, int W, int Cout1, int Cout2, int act, dv_stream_t stream);

/* ---- nn.Conv2d(1, Cout, k in {3,5,7}, padding k/2) + bias + activation (`convd1`, update.py:86,:92) as
 * dv_conv2d_1in_f16: input, weights and bias rounded by rb16, fp32 accumulation, the output rounded before the activation
 * (sigmoid / tanh results rounded again). */
int dv_conv2d_1in_bf16(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cout,
                       int k, int act, dv_stream_t stream);

/* ---- ConvGRU gate arithmetic of the training forward (update.py:36-39) as dv_gru_reset_mul_f16 / dv_gru_blend_f16: flat
 * arrays of n floats (n == 0: DV_ERR_SHAPE), every result rounded by rb16, the operands taken as they are. */
int dv_gru_reset_mul_bf16(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream);
int dv_gru_blend_bf16(const float* z, const float* q, const float* h, float* out, size_t n, dv_stream_t stream);

/* ---- weight gradient over the virtual concatenation as dv_conv2d_wgrad_cat_f16 (same arguments, same split-K plan, same
 * workspace size: at most 48 MB, 0 = a shape the launching entry refuses with DV_ERR_SHAPE -- five sources included;
 * k other than 1 or 3: DV_ERR_UNSUPPORTED).
 * Non-finite operands, as at fp16: the positions of a brick that lie outside the image are staged as g = 0 (and x = 0)
 * and multiplied like any other.  An Inf or NaN of x (a float32 that rounds to Inf included) next to the bottom / right
 * edge of a plane that is no multiple of the brick meets a 0 of g: NaN in the rows of dw of that INPUT channel where the
 * exact sum has no such product.  At bf16 this applies to real Inf / NaN only: no finite float32 below 3.3895e38
 * overflows.  An Inf of g stays in the rows dw[co] of its output channel. */
size_t dv_conv2d_wgrad_cat_bf16_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout, int k);
int dv_conv2d_wgrad_cat_bf16(const float* const* inputs, const int* channels, int n_inputs, const float* g, float* dw,
                             float* workspace, int B, int H, int W, int Cout, int k, dv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
