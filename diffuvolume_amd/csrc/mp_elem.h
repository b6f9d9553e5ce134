// The two 16-bit element types of mixed-precision training (train precisions "f16" and "bf16") as traits: the staged
// element, its vector of 8 (one ds_read_b128, one operand of the matrix instruction), the rounding from float32 and the
// matrix instruction.  csrc/conv3d_mp.h and csrc/conv3d_wgrad_mp.h are written once over these.
//   MpF16   r16:  round to nearest even to fp16, subnormals kept, beyond 65504: Inf      v_mfma_f32_16x16x32_f16
//   MpBf16  rb16: round to nearest even to bfloat16 by the hardware conversion            v_mfma_f32_16x16x32_bf16
//                 (v_cvt_pk_bf16_f32), NaN stays NaN, a finite float32 above about 3.3895e38 rounds to Inf; operands
//                 below 2^-126 (bf16 subnormals) may be flushed to zero
#pragma once
#include "dv_common.h"

struct MpF16 {
  typedef _Float16 elem;
  typedef _Float16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ elem round(float v) { return (_Float16)v; }
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

struct MpBf16 {
  typedef __bf16 elem;
  typedef __bf16 v8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ elem round(float v) { return (__bf16)v; }
  static __device__ __forceinline__ f32x4 mfma(v8 a, v8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};

// the 16 bits of a rounded operand
template <class T>
__device__ __forceinline__ unsigned mp_bits(float v) {
  return (unsigned)__builtin_bit_cast(unsigned short, T::round(v));
}
