// The 3x3x3 stride-1 aggregation convolution of mixed-precision training at train precision "f16", forward and input
// gradient:  y = conv(r16(x), r16(w)) (+ bias),  r16 = round to nearest even fp16 (subnormals kept, beyond 65504: Inf),
// on v_mfma_f32_16x16x32_f16.  The kernel, its staging and the launch helper are csrc/conv3d_mp.h's, written once for
// fp16 and bf16; this file is the fp16 instantiation (the only kernel of this translation unit) and its entry.
#include "conv3d_mp.h"
#include "../../include/diffuvolume_hip_amp3d.h"

extern "C" int dv_conv3d_k3s1_f16_f32(const float* in, const float* w, const float* bias, float* out, int B, int Cin,
                                      int D, int H, int W, int Cout, int k, int transpose_flip, dv_stream_t stream) {
  return conv3d_mp_launch<MpF16>(in, w, bias, out, B, Cin, D, H, W, Cout, k, transpose_flip, stream);
}
