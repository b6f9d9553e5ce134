// Index arithmetic of the regression tail (trilinear x4 -> softmax -> soft-argmax), shared by the forward (regress.hip) and
// its backward (regress_bwd.hip): both must place every output on the same two sources with the same two weights, and
// both must shift the softmax by the same bins.
#pragma once
#include "dv_common.h"

// PyTorch's linear source index (area_pixel_compute_source_index, non-cubic).
template <bool ALIGN>
__device__ __forceinline__ void lin_src(int dst, int in_size, int out_size, int& i0, int& i1, float& l0,
                                        float& l1) {
  float src;
  if (ALIGN) {
    const float scale = out_size > 1 ? (float)(in_size - 1) / (float)(out_size - 1) : 0.f;
    src = scale * (float)dst;
  } else {
    const float scale = (float)in_size / (float)out_size;
    src = scale * ((float)dst + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
  }
  i0 = (int)src;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = src - (float)i0;
  l0 = 1.f - l1;
}

// The bins whose maximum is the softmax shift.  Between two neighbouring slices the four bins are a linear ramp, so the
// maximum sits on the outer bins of a segment (align_corners=False: k = 4d + 1 and 4d + 2; k = 0 and 4D - 1 are the clamped
// ends): half the bins are enough.  With align_corners=True the bins are not periodic and all of them are taken.
// (In floating point an inner bin can exceed that by an ulp when the two slices are nearly equal: its exponential is then
// 1 + O(ulp), harmless.  The maximum of the D SLICES is not a valid shift: bins never reach a slice value, and with steep
// costs every exponential would underflow.)
template <bool ALIGN>
__device__ __forceinline__ constexpr bool tail_shift_bin(int k, int K) {
  return ALIGN || (k & 3) == 1 || (k & 3) == 2 || k == 0 || k == K - 1;
}

// ---- the transposed view, for the backward -------------------------------------------------------------------------
// Weight with which output index `dst` reads source index `src` (0 when it does not): l0 through i0, l1 through i1, and
// both when the clamp at the far border makes i1 == i0.
template <bool ALIGN>
__device__ __forceinline__ float tail_tap_weight(int dst, int src, int in_size, int out_size) {
  int i0, i1;
  float l0, l1;
  lin_src<ALIGN>(dst, in_size, out_size, i0, i1, l0, l1);
  return (i0 == src ? l0 : 0.f) + (i1 == src ? l1 : 0.f);
}

// The outputs that read source index `src`: lin_src's source position is monotone in dst, so they are one contiguous
// range [lo, hi].  It is found by asking lin_src itself, not by inverting its float arithmetic: clamping widens the range
// at the borders and align_corners=True stretches it (up to 11 outputs at in_size = 3), so no fixed width holds.  The
// centre of the range lies in [4 src, 4 src + 3] and its half width is at most (out_size - 1) / (in_size - 1) <= 7 for
// out_size = 4 in_size, so the window below contains it.
template <bool ALIGN>
__device__ __forceinline__ void tail_tap_range(int src, int in_size, int out_size, int& lo, int& hi) {
  const int a = max(0, 4 * src - 12), b = min(out_size - 1, 4 * src + 16);
  lo = out_size;
  hi = -1;
  for (int dst = a; dst <= b; ++dst) {
    int i0, i1;
    float l0, l1;
    lin_src<ALIGN>(dst, in_size, out_size, i0, i1, l0, l1);
    if (i0 == src || i1 == src) {
      lo = min(lo, dst);
      hi = max(hi, dst);
    }
  }
}
