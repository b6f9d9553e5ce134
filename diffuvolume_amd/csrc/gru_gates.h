// The map template of the ConvGRU gate kernels (csrc/gru_gates.hip: fp32 and fp16; csrc/gru_gates_bf16.hip: bf16): one
// kernel maps a per-element functor over flat float32 arrays: float4 body, scalar tail; the launch takes the float4 form
// iff every pointer is 16-byte aligned and the scalar form for any other view.  A functor has NIN inputs, NOUT outputs and
// apply(in, out) for one element; output k enters apply() with its old value where bit k of RMW is set.
// Also here, written once for the two 16-bit element types of csrc/mp_elem.h: the gate arithmetic with the rounding points
// of conv2d_mp.h's epilogues.
#pragma once
#include "mp_elem.h"

namespace {

// The epilogue chain of conv2d_mp.h, operation for operation: every elementwise RESULT is rounded to 16 bits (T::round:
// r16 or rb16), the operands are taken as they are (16-bit-exact on the route; on any other float32 input the kernels
// still give the bits of the forward's epilogues, which do not round them either).
template <class T>
__device__ __forceinline__ float gru_r(float v) { return (float)T::round(v); }
template <class T>
struct GruMulMp {
  static constexpr int NIN = 2, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) { out[0] = gru_r<T>(in[0] * in[1]); }
};
template <class T>
struct GruBlendMp {                                      // in: z, q, h
  static constexpr int NIN = 3, NOUT = 1, RMW = 0;
  static __device__ __forceinline__ void apply(const float* in, float* out) {
    out[0] = gru_r<T>(gru_r<T>(gru_r<T>(1.0f - in[0]) * in[2]) + gru_r<T>(in[0] * in[1]));
  }
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

// the two 16-bit entries of a table
template <class T>
int gru_reset_mul_mp(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(rh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruMulMp<T>>(r, h, nullptr, nullptr, rh, nullptr, nullptr, n, stream);
}

template <class T>
int gru_blend_mp(const float* z, const float* q, const float* h, float* out, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  return gru_launch<GruBlendMp<T>>(z, q, h, nullptr, out, nullptr, nullptr, n, stream);
}

}  // namespace
