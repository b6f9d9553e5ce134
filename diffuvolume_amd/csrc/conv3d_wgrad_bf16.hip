// Weight gradient of the 3x3x3 stride-1 aggregation convolutions at train precision "bf16":
//   dW = sum rb16(g) rb16(x),  rb16 = round to nearest even bfloat16 by v_cvt_pk_bf16_f32 while the operand is staged
//   (NaN stays NaN, a finite float32 above about 3.3895e38 rounds to Inf, operands below 2^-126 may be flushed to zero),
// on v_mfma_f32_16x16x32_bf16, split-K through wgrad_splitk.h with the workspace plan of the fp16 entry.  The kernel, its
// staging, the plan and the launch helper are csrc/conv3d_wgrad_mp.h's, written once for fp16 and bf16; this file is the
// bf16 instantiation (the only kernel of this translation unit) and its two entries.
#include "conv3d_wgrad_mp.h"
#include "../../include/diffuvolume_hip_amp3d_bf16.h"

extern "C" size_t dv_conv3d_wgrad_bf16_workspace_floats(int B, int Cin, int D, int H, int W, int Cout) {
  return conv3d_wgrad_mp_workspace_floats(B, Cin, D, H, W, Cout);
}

extern "C" int dv_conv3d_wgrad_bf16_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D,
                                        int H, int W, int Cout, dv_stream_t stream) {
  return conv3d_wgrad_mp_launch<MpBf16>(x, g, dw, workspace, B, Cin, D, H, W, Cout, stream);
}
