// Weight gradient of the convolutions of IGEV's recurrent update block at train precision "bf16"
// (KITTI15/core/update.py:26-142, the loop of train_stereo.py:146-173 under bf16 autocast) on v_mfma_f32_16x16x32_bf16:
//   dW = sum rb16(g) * rb16(X) over the virtual channel concatenation, an unrounded float32 sum,
// rb16 = round to nearest even bfloat16 by v_cvt_pk_bf16_f32 while an operand is staged (NaN stays NaN, a finite float32
// above about 3.3895e38 rounds to Inf, operands below 2^-126 may be flushed to zero).  The kernel, its staging, the
// split-K plan and the checks are csrc/conv2d_wgrad_cat_mp.h's, written once for fp16 and bf16; this file is the bf16
// instantiation and its entries.
#include "conv2d_wgrad_cat_mp.h"
#include "../../include/diffuvolume_hip_amp2d_bf16.h"

extern "C" size_t dv_conv2d_wgrad_cat_bf16_workspace_floats(const int* channels, int n_inputs, int B, int H, int W,
                                                            int Cout, int k) {
  return conv2d_wgrad_cat_mp_workspace_floats(channels, n_inputs, B, H, W, Cout, k);
}

extern "C" int dv_conv2d_wgrad_cat_bf16(const float* const* inputs, const int* channels, int n_inputs, const float* g,
                                        float* dw, float* workspace, int B, int H, int W, int Cout, int k,
                                        dv_stream_t stream) {
  return conv2d_wgrad_cat_mp_launch<MpBf16>(inputs, channels, n_inputs, g, dw, workspace, B, H, W, Cout, k, stream);
}
