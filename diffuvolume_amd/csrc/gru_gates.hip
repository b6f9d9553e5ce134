// The elementwise gate arithmetic of IGEV's ConvGRU on its training routes (KITTI15/core/update.py:36-39): the products
// and blends between the gate convolutions, forward-for-training and backward, in fp32 (the route of
// conv2d_wgrad_cat.hip) and with the fp16 rounding points of autocast (the route of conv2d_wgrad_cat_f16.hip).
// The kernel template that maps a per-element functor over flat float32 arrays is csrc/gru_gates.h's, with the 16-bit
// gate functors; the bf16 entries of train precision "bf16" are csrc/gru_gates_bf16.hip.
#include "gru_gates.h"

namespace {

// (1 - z) h + z q in the form of the inference epilogue (csrc/conv2d.hip: blend_h + blend_z * (v - blend_h)), so that the
// training forward and the eval forward round the hidden state alike
__device__ __forceinline__ float gru_blend1(float z, float q, float h) { return h + z * (q - h); }

// from dh', z, q, h:  dq_pre = dh' z (1 - q^2),  dz_pre = dh' (q - h) z (1 - z),  dh = dh' (1 - z)
__device__ __forceinline__ void gru_bwd_blend1(float d, float z, float q, float h, float& dq, float& dz, float& dh) {
  dq = d * z * (1.0f - q * q);
  dz = d * (q - h) * z * (1.0f - z);
  dh = d * (1.0f - z);
}

// from d(rh), r, h:  dr_pre = d(rh) h r (1 - r),  dh += d(rh) r
__device__ __forceinline__ void gru_bwd_reset1(float d, float r, float h, float& dr, float& dh) {
  dr = d * h * r * (1.0f - r);
  dh += d * r;
}

// The fp32 functors (the fp16 ones are GruMulMp<MpF16> / GruBlendMp<MpF16> of gru_gates.h).
struct GruMul {
  static constexpr int NIN = 2, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) { out[0] = in[0] * in[1]; }
};
struct GruBlend {
  static constexpr int NIN = 3, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) { out[0] = gru_blend1(in[0], in[1], in[2]); }
};
struct GruBwdBlend {
  static constexpr int NIN = 4, NOUT = 3, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) {
    gru_bwd_blend1(in[0], in[1], in[2], in[3], out[0], out[1], out[2]);
  }
};
struct GruBwdReset {
  static constexpr int NIN = 3, NOUT = 2, RMW = 2;                 // dh accumulates
  static __device__ __forceinline__ void apply(const float* in, float* out) {
    gru_bwd_reset1(in[0], in[1], in[2], out[0], out[1]);
  }
};
}  // namespace

extern "C" int dv_gru_reset_mul_f32(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(rh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruMul>(r, h, nullptr, nullptr, rh, nullptr, nullptr, n, stream);
}

extern "C" int dv_gru_blend_f32(const float* z, const float* q, const float* h, float* out, size_t n,
                                dv_stream_t stream) {
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruBlend>(z, q, h, nullptr, out, nullptr, nullptr, n, stream);
}

extern "C" int dv_gru_gates_bwd_blend_f32(const float* dh_new, const float* z, const float* q, const float* h,
                                          float* dq_pre, float* dz_pre, float* dh, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(dh_new);
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(dq_pre);
  DV_REQUIRE_PTR(dz_pre);
  DV_REQUIRE_PTR(dh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruBwdBlend>(dh_new, z, q, h, dq_pre, dz_pre, dh, n, stream);
}

extern "C" int dv_gru_gates_bwd_reset_f32(const float* drh, const float* r, const float* h, float* dr_pre, float* dh,
                                          size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(drh);
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(dr_pre);
  DV_REQUIRE_PTR(dh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruBwdReset>(drh, r, h, nullptr, dr_pre, dh, nullptr, n, stream);
}

extern "C" int dv_gru_reset_mul_f16(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream) {
  return gru_reset_mul_mp<MpF16>(r, h, rh, n, stream);
}

extern "C" int dv_gru_blend_f16(const float* z, const float* q, const float* h, float* out, size_t n,
                                dv_stream_t stream) {
  return gru_blend_mp<MpF16>(z, q, h, out, n, stream);
}
