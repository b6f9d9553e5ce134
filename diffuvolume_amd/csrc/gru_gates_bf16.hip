// The ConvGRU gate arithmetic of IGEV's update block at train precision "bf16" (KITTI15/core/update.py:36-39): r * h and
// (1 - z) h + z q with every elementwise result rounded by rb16, the rounding points of csrc/conv2d_bf16.hip's epilogues
// and of torch's bfloat16 arithmetic.  The functors and the map kernel are csrc/gru_gates.h's, the templates of the fp16
// gate entries with the other rounding function; the gate backward stays float32 (csrc/gru_gates.hip).
#include "gru_gates.h"
#include "../../include/diffuvolume_hip_amp2d_bf16.h"

extern "C" int dv_gru_reset_mul_bf16(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream) {
  return gru_reset_mul_mp<MpBf16>(r, h, rh, n, stream);
}

extern "C" int dv_gru_blend_bf16(const float* z, const float* q, const float* h, float* out, size_t n,
                                 dv_stream_t stream) {
  return gru_blend_mp<MpBf16>(z, q, h, out, n, stream);
}
