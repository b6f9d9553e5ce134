// The elementwise gate arithmetic of IGEV's ConvGRU on its training routes (KITTI15/core/update.py:36-39): the products
// and blends between the gate convolutions, forward-for-training and backward, in fp32 (the route of
// conv2d_wgrad_cat.hip) and with the fp16 rounding points of autocast (the route of conv2d_wgrad_cat_f16.hip).
// One kernel template maps a per-element functor over flat float32 arrays: float4 body, scalar tail; the entry takes the
// float4 form iff every pointer is 16-byte aligned and the scalar form for any other view.
#include "dv_common.h"

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

// The epilogue chain of conv2d_f16.hip, operation for operation: every elementwise RESULT is rounded to fp16, the
// operands are taken as they are (fp16-exact on the route; on any other float32 input the kernels still give the bits of
// the eval forward's epilogues under fp16 autocast, which do not round them either).
__device__ __forceinline__ float hr16(float v) { return (float)(_Float16)v; }
__device__ __forceinline__ float gru_mul16(float r, float h) { return hr16(r * h); }
__device__ __forceinline__ float gru_blend16(float z, float q, float h) {
  return hr16(hr16(hr16(1.0f - z) * h) + hr16(z * q));
}

// The functors: NIN inputs, NOUT outputs, apply(in, out) for one element.  Output k enters apply() with its old value where
// bit k of RMW is set.
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
struct GruMul16 {
  static constexpr int NIN = 2, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) { out[0] = gru_mul16(in[0], in[1]); }
};
struct GruBlend16 {
  static constexpr int NIN = 3, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) { out[0] = gru_blend16(in[0], in[1], in[2]); }
};

constexpr int GRU_MAX_IN = 4, GRU_MAX_OUT = 3;

// the first F::NIN of i0 .. i3 and the first F::NOUT of o0 .. o2 are used; V = 4: float4 body and scalar tail, V = 1: scalar
template <class F, int V>
__global__ __launch_bounds__(256) void gru_map_kernel(const float* __restrict__ i0, const float* __restrict__ i1,
                                                      const float* __restrict__ i2, const float* __restrict__ i3,
                                                      float* __restrict__ o0, float* __restrict__ o1,
                                                      float* __restrict__ o2, size_t n) {
  const float* const in[GRU_MAX_IN] = {i0, i1, i2, i3};
  float* const out[GRU_MAX_OUT] = {o0, o1, o2};
  const size_t stride = (size_t)gridDim.x * blockDim.x, t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = V == 4 ? n / 4 : 0;
  for (size_t i = t0; i < nv; i += stride) {
    f32x4 x[F::NIN], y[F::NOUT];
#pragma unroll
    for (int k = 0; k < F::NIN; ++k) x[k] = ((const f32x4*)in[k])[i];
#pragma unroll
    for (int k = 0; k < F::NOUT; ++k)
      if ((F::RMW >> k) & 1) y[k] = ((const f32x4*)out[k])[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float a[F::NIN], r[F::NOUT];
#pragma unroll
      for (int k = 0; k < F::NIN; ++k) a[k] = x[k][j];
#pragma unroll
      for (int k = 0; k < F::NOUT; ++k)
        if ((F::RMW >> k) & 1) r[k] = y[k][j];
      F::apply(a, r);
#pragma unroll
      for (int k = 0; k < F::NOUT; ++k) y[k][j] = r[k];
    }
#pragma unroll
    for (int k = 0; k < F::NOUT; ++k) ((f32x4*)out[k])[i] = y[k];
  }
  for (size_t i = nv * 4 + t0; i < n; i += stride) {
    float a[F::NIN], r[F::NOUT];
#pragma unroll
    for (int k = 0; k < F::NIN; ++k) a[k] = in[k][i];
#pragma unroll
    for (int k = 0; k < F::NOUT; ++k)
      if ((F::RMW >> k) & 1) r[k] = out[k][i];
    F::apply(a, r);
#pragma unroll
    for (int k = 0; k < F::NOUT; ++k) out[k][i] = r[k];
  }
}

unsigned gru_grid(size_t n) {
  const size_t nb = (n / 4 + 255) / 256 + 1;
  return (unsigned)(nb < 4096 ? nb : 4096);
}

// pointers the functor does not use are null (and count as aligned)
template <class F>
int gru_launch(const float* i0, const float* i1, const float* i2, const float* i3, float* o0, float* o1, float* o2, size_t n,
               dv_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (dv_aligned16(i0) && dv_aligned16(i1) && dv_aligned16(i2) && dv_aligned16(i3) && dv_aligned16(o0) &&
      dv_aligned16(o1) && dv_aligned16(o2))
    hipLaunchKernelGGL((gru_map_kernel<F, 4>), dim3(gru_grid(n)), dim3(256), 0, s, i0, i1, i2, i3, o0, o1, o2, n);
  else
    hipLaunchKernelGGL((gru_map_kernel<F, 1>), dim3(gru_grid(n)), dim3(256), 0, s, i0, i1, i2, i3, o0, o1, o2, n);
  return dv_launch_status();
}

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
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(rh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruMul16>(r, h, nullptr, nullptr, rh, nullptr, nullptr, n, stream);
}

extern "C" int dv_gru_blend_f16(const float* z, const float* q, const float* h, float* out, size_t n,
                                dv_stream_t stream) {
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruBlend16>(z, q, h, nullptr, out, nullptr, nullptr, n, stream);
}
