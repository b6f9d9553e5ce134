// K10 backward: the gradients of IGEV's geometry lookup with the noise filter (geo_lookup.hip; the reference
// differentiates Combined_Geo_Encoding_Volume.__call__, KITTI15/core/geometry_ddim.py:33-69, once per GRU iteration of the
// train loop, igev_stereo_ddim.py:441-443) with respect to the geometry volume and to the all-pairs correlation.
//
// The lookup is linear in both, so the backward reads neither the volume nor the forward's output: only grad_out, the
// sample positions (disp, coords) and the noise.  For flat pixel n with noise row r = noisy_flat[n*D .. n*D + D),
// R[m] = (r[2m] + r[2m+1]) / 2, level-0 taps (i_t, a_t, b_t) = sample_pos(d + t - 4, D) and level-1 taps
// (j_t, a'_t, b'_t) = sample_pos(d/2 + t - 4, D/2):
//   dgeo[c,k]  = sum_t g0[c,t] (a_t r[k] [i_t = k] + b_t r[k] [i_t + 1 = k])
//              + sum_t g1[c,t] (a'_t [j_t = k>>1] + b'_t [j_t + 1 = k>>1]) R[k>>1] / 2        (k < 2 (D/2))
//   dcorr0[k]  = the same without noise at cx - d + t - 4 over W2 and cx/2 - d/2 + t - 4 over W2/2: corr1 is only the
//                avg_pool of corr0 (geometry_ddim.py:28-30), so its gradient folds into dcorr0 with the factor 1/2.
// Every cell of dgeo and every row of dcorr0 belongs to exactly one pixel: no atomics, no memset, every element written
// exactly once (zero outside the pixel's 24-entry window), the same bits on every launch and for every batch split.
//
// dgeo (w fastest): a lane owns a pixel, builds the 24 coefficients of a channel in its LDS column (the forward's gwin
// layout) and the wave then walks the planes k = 0 .. D-1 of its 64 pixels together -- one 256-byte segment per store.
// dcorr0 (W2 contiguous floats per pixel): the owner lane leaves its 24 coefficients in LDS and the wave writes its 64
// rows one after the other, the lanes spread over x2.
#include "geo_sample.h"

namespace {

template <int R>
__global__ __launch_bounds__(256) void geo_lookup_dgeo_kernel(const float* __restrict__ grad_out,
                                                              const float* __restrict__ disp,
                                                              const float* __restrict__ noisy, float* __restrict__ dgeo,
                                                              int C, int D, int h, int w, size_t npix) {
  constexpr int T = 2 * R + 1;
  static_assert(R == 4, "window sized for radius 4");
  __shared__ float win[GEO_WIN * 256];                  // first the noise window, then the coefficients of a channel
  const int tid = threadIdx.x;
  const size_t n0 = (size_t)blockIdx.x * blockDim.x + tid;
  const bool live = n0 < npix;
  const size_t n = live ? n0 : npix - 1;                // (a lane past the end shadows the last pixel and stores nothing)
  const size_t hw = (size_t)h * w;
  const size_t b = n / hw, p = n - b * hw;
  const float d = disp[n];
  const float* nrow = noisy + n * D;                    // raw-reshape row (quirk)
  const int D1 = D / 2;
  const int dlo = 2 * (int)floorf(d * 0.5f) - 10;
  float* cw = win + tid;                                // entry k at cw[k * 256]: a column only this lane touches
  if ((D & 3) == 0 && ((reinterpret_cast<uintptr_t>(noisy) & 15u) == 0)) {   // (uniform; the forward's two ways to the same values)
    const int base = dlo & ~3;
#pragma unroll
    for (int k = 0; k < GEO_WIN; ++k) cw[k * 256] = 0.f;
    float4 nq[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const int kk = base + 4 * q;
      nq[q] = (unsigned)kk < (unsigned)D ? *reinterpret_cast<const float4*>(nrow + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) {
      const float e4[4] = {nq[q].x, nq[q].y, nq[q].z, nq[q].w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int slot = base + 4 * q + e - dlo;          // (base - dlo is 0 or -2)
        if ((unsigned)slot < (unsigned)GEO_WIN) cw[slot * 256] = e4[e];
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < GEO_WIN; ++k) cw[k * 256] = (unsigned)(dlo + k) < (unsigned)D ? nrow[dlo + k] : 0.f;
  }
  // per tap: the window slots and weight x noise (entries outside [0, D) carry zero noise: the forward's zero padding)
  int s0[T], s1[T];
  float an0[T], bn0[T], an1[T], bn1[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    int i0;
    float a, bb;
    sample_pos(d + (float)(t - R), D, i0, a, bb);
    int s = i0 - dlo;                                   // entries s, s + 1 (5 .. 18 by construction)
    s = s < 0 ? 0 : (s > GEO_WIN - 2 ? GEO_WIN - 2 : s);              // (never taken: keeps every access in the column)
    s0[t] = s;
    an0[t] = a * cw[s * 256];
    bn0[t] = bb * cw[(s + 1) * 256];
    sample_pos(d / 2.0f + (float)(t - R), D1, i0, a, bb);
    s = 2 * i0 - dlo;                                   // entries s .. s + 3 (0 .. 23)
    s = s < 0 ? 0 : (s > GEO_WIN - 4 ? GEO_WIN - 4 : s);
    s1[t] = s;
    const float n10 = (unsigned)i0 < (unsigned)D1 ? (cw[s * 256] + cw[(s + 1) * 256]) * 0.5f : 0.f;      // (an odd D: one entry past the pairs)
    const float n11 = (unsigned)(i0 + 1) < (unsigned)D1 ? (cw[(s + 2) * 256] + cw[(s + 3) * 256]) * 0.5f : 0.f;
    an1[t] = 0.5f * (a * n10);
    bn1[t] = 0.5f * (bb * n11);
  }
  const int half = C * T + T;
  const float* go = grad_out + b * (size_t)(2 * half) * hw + p;       // + channel * hw
  for (int c = blockIdx.y; c < C; c += gridDim.y) {
    float g0[T], g1[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      g0[t] = go[(size_t)(c * T + t) * hw];
      g1[t] = go[(size_t)(half + c * T + t) * hw];
    }
#pragma unroll
    for (int k = 0; k < GEO_WIN; ++k) cw[k * 256] = 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) {                       // (slots of different taps coincide: read-modify-write, in tap order)
      cw[s0[t] * 256] += g0[t] * an0[t];
      cw[(s0[t] + 1) * 256] += g0[t] * bn0[t];
      const float u0 = g1[t] * an1[t], u1 = g1[t] * bn1[t];
      cw[s1[t] * 256] += u0;
      cw[(s1[t] + 1) * 256] += u0;
      cw[(s1[t] + 2) * 256] += u1;
      cw[(s1[t] + 3) * 256] += u1;
    }
    float* o = dgeo + ((b * C + c) * D) * hw + p;       // + k * hw
#pragma unroll 4
    for (int k = 0; k < D; ++k) {
      const unsigned slot = (unsigned)k - (unsigned)dlo;
      const float v = cw[(slot < (unsigned)GEO_WIN ? slot : 0u) * 256];
      if (live) o[(size_t)k * hw] = slot < (unsigned)GEO_WIN ? v : 0.f;
    }
  }
}

constexpr int GEO_CS = GEO_WIN + 1;     // row stride of a pixel's correlation coefficients (odd: rows fall on different banks)

template <int R>
__global__ __launch_bounds__(256) void geo_lookup_dcorr_kernel(const float* __restrict__ grad_out,
                                                               const float* __restrict__ disp,
                                                               const float* __restrict__ coords,
                                                               float* __restrict__ dcorr0, int C, int h, int w, int W2,
                                                               size_t npix) {
  constexpr int T = 2 * R + 1;
  static_assert(R == 4, "window sized for radius 4");
  __shared__ float ccw[256 * GEO_CS];
  __shared__ int clo_s[256];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const size_t n0 = (size_t)blockIdx.x * blockDim.x + tid;
  const size_t n = n0 < npix ? n0 : npix - 1;
  const size_t hw = (size_t)h * w;
  const size_t b = n / hw, p = n - b * hw;
  const float d = disp[n], cx = coords[n];
  const int W2b = W2 / 2;
  const int clo = 2 * (int)floorf(cx / 2.0f - d / 2.0f) - 10;
  float* col = ccw + tid * GEO_CS;
#pragma unroll
  for (int k = 0; k < GEO_WIN; ++k) col[k] = 0.f;
  const int half = C * T + T;
  const float* go = grad_out + b * (size_t)(2 * half) * hw + p;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    int i0;
    float w0, w1;
    sample_pos(cx - d + (float)(t - R), W2, i0, w0, w1);
    int s = i0 - clo;
    s = s < 0 ? 0 : (s > GEO_WIN - 2 ? GEO_WIN - 2 : s);              // (never taken, as above)
    const float gc0 = go[(size_t)(C * T + t) * hw];
    col[s] += gc0 * w0;
    col[s + 1] += gc0 * w1;
    sample_pos(cx / 2.0f - d / 2.0f + (float)(t - R), W2b, i0, w0, w1);
    s = 2 * i0 - clo;
    s = s < 0 ? 0 : (s > GEO_WIN - 4 ? GEO_WIN - 4 : s);
    const float gc1 = 0.5f * go[(size_t)(half + C * T + t) * hw];
    if ((unsigned)i0 < (unsigned)W2b) {                 // (an odd W2: the last entry has no pooled partner)
      col[s] += gc1 * w0;
      col[s + 1] += gc1 * w0;
    }
    if ((unsigned)(i0 + 1) < (unsigned)W2b) {
      col[s + 2] += gc1 * w1;
      col[s + 3] += gc1 * w1;
    }
  }
  clo_s[tid] = clo;
  __syncthreads();
  // the wave's 64 rows, one per step; entries outside [0, W2) of a window are simply never stored
  const size_t nw0 = (size_t)blockIdx.x * blockDim.x + wave * 64;
  for (int q = 0; q < 64; ++q) {
    const size_t nq = nw0 + q;
    if (nq >= npix) break;                              // (uniform)
    const unsigned cq = (unsigned)clo_s[wave * 64 + q];
    const float* colq = ccw + (wave * 64 + q) * GEO_CS;
    float* row = dcorr0 + nq * W2;
    for (int x2 = lane; x2 < W2; x2 += 64) {
      const unsigned slot = (unsigned)x2 - cq;
      const float v = colq[slot < (unsigned)GEO_WIN ? slot : 0u];
      row[x2] = slot < (unsigned)GEO_WIN ? v : 0.f;
    }
  }
}

}  // namespace

extern "C" int dv_geo_filter_lookup_bwd_f32(const float* grad_out, const float* disp, const float* coords,
                                            const float* noisy, float* dgeo, float* dcorr0, int B, int C, int D, int h,
                                            int w, int W2, int radius, dv_stream_t stream) {
  DV_REQUIRE_PTR(grad_out);
  DV_REQUIRE_PTR(disp);
  DV_REQUIRE_PTR(coords);
  DV_REQUIRE_PTR(noisy);
  DV_REQUIRE(dgeo != nullptr || dcorr0 != nullptr, DV_ERR_NULL);
  DV_REQUIRE(B > 0 && C > 0 && D > 3 && h > 0 && w > 0 && W2 > 3, DV_ERR_SHAPE);
  DV_REQUIRE(radius == 4, DV_ERR_UNSUPPORTED);   // as the forward
  const size_t npix = (size_t)B * h * w;
  const unsigned nblk = (unsigned)((npix + 255) / 256);
  if (dgeo) {
    // channels spread over grid.y until the launch has ~1024 blocks (every cell has one writer either way)
    unsigned cy = (1024u + nblk - 1) / nblk;
    cy = cy < 1u ? 1u : (cy > (unsigned)C ? (unsigned)C : cy);
    hipLaunchKernelGGL((geo_lookup_dgeo_kernel<4>), dim3(nblk, cy), dim3(256), 0, (hipStream_t)stream, grad_out, disp,
                       noisy, dgeo, C, D, h, w, npix);
    const int e = dv_launch_status();
    if (e != DV_OK) return e;
  }
  if (dcorr0) {
    hipLaunchKernelGGL((geo_lookup_dcorr_kernel<4>), dim3(nblk), dim3(256), 0, (hipStream_t)stream, grad_out, disp,
                       coords, dcorr0, C, h, w, W2, npix);
    return dv_launch_status();
  }
  return DV_OK;
}
