// Weight gradient of the convolutions of IGEV's recurrent update block under fp16 autocast (mixed-precision training at
// train precision "f16": KITTI15/core/update.py:26-142 run inside `autocast(enabled=args.mixed_precision)`,
// train_stereo.py:146-173) on v_mfma_f32_16x16x32_f16:  dW = sum r16(g) * r16(X) over the virtual channel concatenation,
// an unrounded float32 sum.  The kernel, its staging, the split-K plan and the checks are csrc/conv2d_wgrad_cat_mp.h's,
// written once for fp16 and bf16; this file is the fp16 instantiation and its entries.
#include "conv2d_wgrad_cat_mp.h"

extern "C" size_t dv_conv2d_wgrad_cat_f16_workspace_floats(const int* channels, int n_inputs, int B, int H, int W,
                                                           int Cout, int k) {
  return conv2d_wgrad_cat_mp_workspace_floats(channels, n_inputs, B, H, W, Cout, k);
}

extern "C" int dv_conv2d_wgrad_cat_f16(const float* const* inputs, const int* channels, int n_inputs, const float* g,
                                       float* dw, float* workspace, int B, int H, int W, int Cout, int k,
                                       dv_stream_t stream) {
  return conv2d_wgrad_cat_mp_launch<MpF16>(inputs, channels, n_inputs, g, dw, workspace, B, H, W, Cout, k, stream);
}
