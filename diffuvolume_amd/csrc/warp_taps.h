// The bilinear taps of `warp` (KITTI12/models/submodule.py:137-176), shared by the eval kernel that assembles the refinement
// network's input (refine_inputs.hip) and the training pair (warp_corr.hip): forward and backward must place every output
// pixel on the same four sources with the same four weights and take the same decision about its validity.
#pragma once
#include "dv_common.h"

// bilinear taps of grid_sample(align_corners=False, zeros padding) for output pixel (y, x) shifted by d
struct Taps {
  int x0, y0;           // north-west corner
  float nw, ne, sw, se; // weights
  float valid;          // 1 if the sampled all-ones image is >= 0.999, else 0
};

__device__ __forceinline__ Taps make_taps(float x, float y, float d, int W, int H) {
  const float gx = 2.0f * (x - d) / (float)(W > 1 ? W - 1 : 1) - 1.0f;
  const float gy = 2.0f * y / (float)(H > 1 ? H - 1 : 1) - 1.0f;
  const float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float fx = floorf(ix), fy = floorf(iy);
  Taps t;
  t.x0 = (int)fx; t.y0 = (int)fy;
  t.nw = (fx + 1.f - ix) * (fy + 1.f - iy);
  t.ne = (ix - fx) * (fy + 1.f - iy);
  t.sw = (fx + 1.f - ix) * (iy - fy);
  t.se = (ix - fx) * (iy - fy);
  const bool xl = (unsigned)t.x0 < (unsigned)W, xr = (unsigned)(t.x0 + 1) < (unsigned)W;
  const bool yt = (unsigned)t.y0 < (unsigned)H, yb = (unsigned)(t.y0 + 1) < (unsigned)H;
  float m = 0.f;
  if (xl && yt) m += t.nw;
  if (xr && yt) m += t.ne;
  if (xl && yb) m += t.sw;
  if (xr && yb) m += t.se;
  t.valid = m < 0.999f ? 0.f : 1.f;
  if (!(xl && yt)) t.nw = 0.f;
  if (!(xr && yt)) t.ne = 0.f;
  if (!(xl && yb)) t.sw = 0.f;
  if (!(xr && yb)) t.se = 0.f;
  return t;
}

__device__ __forceinline__ float warp_one(const float* __restrict__ plane, const Taps& t, int W, int H) {
  // out-of-range taps carry weight 0; clamp their addresses
  const int xa = min(max(t.x0, 0), W - 1), xb = min(max(t.x0 + 1, 0), W - 1);
  const int ya = min(max(t.y0, 0), H - 1), yb = min(max(t.y0 + 1, 0), H - 1);
  float v = plane[(size_t)ya * W + xa] * t.nw;
  v += plane[(size_t)ya * W + xb] * t.ne;
  v += plane[(size_t)yb * W + xa] * t.sw;
  v += plane[(size_t)yb * W + xb] * t.se;
  return v * t.valid;
}

// The vertical weights of the two tap rows of output row y, (fy + 1 - iy, iy - fy) with make_taps' iy: what the gradient
// with respect to the sample column multiplies the horizontal differences of the two rows by.
__device__ __forceinline__ void warp_row_weights(float y, int H, float& top, float& bottom) {
  const float gy = 2.0f * y / (float)(H > 1 ? H - 1 : 1) - 1.0f;
  const float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  const float fy = floorf(iy);
  top = fy + 1.f - iy;
  bottom = iy - fy;
}
