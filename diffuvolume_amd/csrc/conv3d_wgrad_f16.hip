// Weight gradient of the 3x3x3 stride-1 aggregation convolutions at train precision "f16":
//   dW = sum r16(g) r16(x),  r16 = round to nearest even fp16 (subnormals kept, beyond 65504: Inf),
// on v_mfma_f32_16x16x32_f16, split-K through wgrad_splitk.h.  The kernel, its staging, the plan and the launch helper
// are csrc/conv3d_wgrad_mp.h's, written once for fp16 and bf16; this file is the fp16 instantiation (the only kernel of
// this translation unit) and its two entries.
#include "conv3d_wgrad_mp.h"
#include "../../include/diffuvolume_hip_amp3d.h"

extern "C" size_t dv_conv3d_wgrad_f16_workspace_floats(int B, int Cin, int D, int H, int W, int Cout) {
  return conv3d_wgrad_mp_workspace_floats(B, Cin, D, H, W, Cout);
}

extern "C" int dv_conv3d_wgrad_f16_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D,
                                       int H, int W, int Cout, dv_stream_t stream) {
  return conv3d_wgrad_mp_launch<MpF16>(x, g, dw, workspace, B, Cin, D, H, W, Cout, stream);
}
