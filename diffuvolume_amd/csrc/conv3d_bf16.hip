// The 3x3x3 stride-1 aggregation convolution of mixed-precision training at train precision "bf16", forward and input
// gradient:  y = conv(rb16(x), rb16(w)) (+ bias),  rb16 = round to nearest even bfloat16 by v_cvt_pk_bf16_f32 while the
// operand is staged (NaN stays NaN, a finite float32 above about 3.3895e38 rounds to Inf, operands below 2^-126 may be
// flushed to zero), on v_mfma_f32_16x16x32_bf16.  The kernel, its staging and the launch helper are csrc/conv3d_mp.h's,
// written once for fp16 and bf16; this file is the bf16 instantiation (the only kernel of this translation unit) and its
// entry.
#include "conv3d_mp.h"
#include "../../include/diffuvolume_hip_amp3d_bf16.h"

extern "C" int dv_conv3d_k3s1_bf16_f32(const float* in, const float* w, const float* bias, float* out, int B, int Cin,
                                       int D, int H, int W, int Cout, int k, int transpose_flip, dv_stream_t stream) {
  return conv3d_mp_launch<MpBf16>(in, w, bias, out, B, Cin, D, H, W, Cout, k, transpose_flip, stream);
}
