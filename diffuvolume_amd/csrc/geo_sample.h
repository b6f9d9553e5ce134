// Sample positions of IGEV's geometry lookup, shared by the forward (geo_lookup.hip) and its backward
// (geo_lookup_bwd.hip): both must place every tap on the same two entries with the same two weights.
#pragma once
#include "dv_common.h"

// bilinear_sampler + grid_sample(align_corners=True, zeros) along one axis of length n, in the
// reference's float order: xg = 2x/(n-1) - 1 ; ix = ((xg+1)/2)*(n-1)
__device__ __forceinline__ void sample_pos(float x, int n, int& i0, float& w0, float& w1) {
  const float xg = 2.0f * x / (float)(n - 1) - 1.0f;
  const float ix = ((xg + 1.0f) / 2.0f) * (float)(n - 1);
  const float fl = floorf(ix);
  i0 = (int)fl;
  w0 = (fl + 1.0f) - ix;   // weight of i0   (ix_ne - ix)
  w1 = ix - fl;            // weight of i0+1
}

// The window of a pixel: level 0 touches entries floor(x) - 5 .. floor(x) + 6 and level 1 (pairs of them)
// 2 floor(x/2) - 10 .. 2 floor(x/2) + 13, so the 24 entries from 2 floor(x/2) - 10 hold every tap of both levels.
constexpr int GEO_WIN = 24;
