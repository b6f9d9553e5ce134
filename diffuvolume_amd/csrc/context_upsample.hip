// IGEV's convex upsampling of the quarter-resolution disparity (KITTI15/core/igev_stereo_ddim.py:209-217
// `upsample_disp`, core/submodule.py:241-253 `context_upsample`):
//   p      = softmax over the 9 taps of the superpixel logits [B,9,4h,4w]          (F.softmax(spx_pred, 1))
//   out[Y,X] = sum_k p_k[Y,X] * scale * disp[(Y>>2) + ky - 1, (X>>2) + kx - 1]      (unfold 3x3 pad 1, nearest x4)
// with tap k = 3*ky + kx (F.unfold's channel order) and zeros outside the image.  The reference materialises the
// unfolded [B,9,h,w] tensor, its nearest-neighbour x4 copy [B,9,4h,4w], the softmax and the product; here each
// thread owns 4 consecutive X of one output row (they share one low-resolution cell): 9 x 16-byte logit loads, one
// 3x3 neighbourhood of the disparity, one 16-byte store.  HBM-bound: 40 B/output pixel.
#include "dv_common.h"

namespace {

template <bool SOFTMAX>
__global__ __launch_bounds__(256) void context_upsample_kernel(const float* __restrict__ disp,
                                                               const float* __restrict__ w9,
                                                               float* __restrict__ out, float scale, int h, int w,
                                                               size_t cells) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;      // one (b, Y, x) cell = 4 output pixels
  if (i >= cells) return;
  const int x = (int)(i % w);
  const int Y = (int)((i / w) % (4 * h));
  const size_t b = i / ((size_t)w * 4 * h);
  const int y = Y >> 2;
  const float* dp = disp + b * (size_t)h * w;
  float nb[9];
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y + ky - 1, xx = x + kx - 1;
      nb[ky * 3 + kx] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? dp[(size_t)yy * w + xx] * scale : 0.f;
    }
  const size_t plane = (size_t)16 * h * w;
  const size_t o = (size_t)Y * 4 * w + 4 * x;
  const float* lp = w9 + b * 9 * plane + o;
  float4 l[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) l[k] = *reinterpret_cast<const float4*>(lp + k * plane);
  float r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = j == 0 ? l[k].x : j == 1 ? l[k].y : j == 2 ? l[k].z : l[k].w;
    if (SOFTMAX) {
      float m = v[0];
#pragma unroll
      for (int k = 1; k < 9; ++k) m = fmaxf(m, v[k]);
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        v[k] = expf(v[k] - m);
        s += v[k];
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = v[k] / s;
    }
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) acc += nb[k] * v[k];
    r[j] = acc;
  }
  *reinterpret_cast<float4*>(out + b * plane + o) = make_float4(r[0], r[1], r[2], r[3]);
}


// ---- backward (training: the reference differentiates upsample_disp at every GRU iteration, igev_stereo_ddim.py:441-457)
// With nb_k the scaled neighbourhood of the forward and p the recomputed softmax (never saved):
//   d logit_k[Y,X] = p_k (g nb_k - sum_j p_j g nb_j)            (no softmax: d weight_k = g nb_k)
//   d disp[y,x]    = scale * sum_k s_k[y - ky + 1, x - kx + 1],  s_k[cell] = sum over the cell's 16 pixels of g p_k
// Pass 1: a block is 4 waves x 64 cells of one cell row; wave r owns output row 4y + r, a lane 4 consecutive X (the
// forward's mapping: 9 + 1 16-byte loads, 9 16-byte stores).  The four row partials of s_k meet in LDS and are added in
// row order into the [B,9,h,w] intermediate.  Pass 2 gathers the nine neighbouring cells of that intermediate in tap
// order.  No scatter, no atomics: the same bits on every launch.  HBM: 40 B read + 36 B written per output pixel, plus
// 2 x 36 B per CELL for the intermediate (4.5 B per pixel).
constexpr int CB_CELLS = 64;

template <bool SOFTMAX, bool WANT_DW, bool WANT_DD>
__global__ __launch_bounds__(256) void context_upsample_bwd_kernel(const float* __restrict__ disp,
                                                                   const float* __restrict__ w9,
                                                                   const float* __restrict__ g, float* __restrict__ dw9,
                                                                   float* __restrict__ cell_sums, float scale, int h,
                                                                   int w) {
  __shared__ float part[4][9][CB_CELLS];
  const int lane = threadIdx.x & 63, r = threadIdx.x >> 6;
  const int x = blockIdx.x * CB_CELLS + lane, y = blockIdx.y;
  const size_t b = blockIdx.z;
  const bool live = x < w;
  float s9[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) s9[k] = 0.f;
  if (live) {
    const float* dp = disp + b * (size_t)h * w;
    float nb[9];
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int yy = y + ky - 1, xx = x + kx - 1;
        nb[ky * 3 + kx] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? dp[(size_t)yy * w + xx] * scale : 0.f;
      }
    const size_t plane = (size_t)16 * h * w;
    const size_t o = (size_t)(4 * y + r) * 4 * w + 4 * x;
    const float* lp = w9 + b * 9 * plane + o;
    float4 l[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) l[k] = *reinterpret_cast<const float4*>(lp + k * plane);
    const float4 g4 = *reinterpret_cast<const float4*>(g + b * plane + o);
    float d[9][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float v[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) v[k] = j == 0 ? l[k].x : j == 1 ? l[k].y : j == 2 ? l[k].z : l[k].w;
      const float gj = j == 0 ? g4.x : j == 1 ? g4.y : j == 2 ? g4.z : g4.w;
      if (SOFTMAX) {                                     // the forward's expression: the forward's bits
        float m = v[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) m = fmaxf(m, v[k]);
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          v[k] = expf(v[k] - m);
          s += v[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = v[k] / s;
      }
      if (WANT_DD) {
#pragma unroll
        for (int k = 0; k < 9; ++k) s9[k] += gj * v[k];
      }
      if (WANT_DW) {
        float gn[9], dot = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          gn[k] = gj * nb[k];
          dot += v[k] * gn[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) d[k][j] = SOFTMAX ? v[k] * (gn[k] - dot) : gn[k];
      }
    }
    if (WANT_DW) {
      float* op = dw9 + b * 9 * plane + o;
#pragma unroll
      for (int k = 0; k < 9; ++k)
        *reinterpret_cast<float4*>(op + k * plane) = make_float4(d[k][0], d[k][1], d[k][2], d[k][3]);
    }
  }
  if (WANT_DD) {
#pragma unroll
    for (int k = 0; k < 9; ++k) part[r][k][lane] = s9[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 9 * CB_CELLS; e += 256) {
      const int k = e / CB_CELLS, c = e % CB_CELLS, xc = blockIdx.x * CB_CELLS + c;
      if (xc < w)
        cell_sums[((b * 9 + k) * h + y) * (size_t)w + xc] = ((part[0][k][c] + part[1][k][c]) + part[2][k][c]) + part[3][k][c];
    }
  }
}

// d_disp[b,y,x] = scale * sum_k s_k[b, y - ky + 1, x - kx + 1], taps in k order, zero outside the image
__global__ __launch_bounds__(256) void context_upsample_ddisp_kernel(const float* __restrict__ cell_sums,
                                                                     float* __restrict__ ddisp, float scale, int h, int w,
                                                                     size_t cells) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  const int x = (int)(i % w), y = (int)((i / w) % h);
  const size_t b = i / ((size_t)w * h);
  float acc = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y - ky + 1, xx = x - kx + 1;
      if (yy >= 0 && yy < h && xx >= 0 && xx < w) acc += cell_sums[((b * 9 + ky * 3 + kx) * h + yy) * (size_t)w + xx];
    }
  ddisp[i] = acc * scale;
}

template <bool SOFTMAX>
void launch_bwd(const float* disp, const float* w9, const float* g, float* dw9, float* sums, float scale, int B, int h,
                int w, bool want_dd, hipStream_t s) {
  const dim3 grid((unsigned)((w + CB_CELLS - 1) / CB_CELLS), (unsigned)h, (unsigned)B);
  if (dw9 != nullptr && want_dd)
    hipLaunchKernelGGL((context_upsample_bwd_kernel<SOFTMAX, true, true>), grid, dim3(256), 0, s, disp, w9, g, dw9, sums,
                       scale, h, w);
  else if (dw9 != nullptr)
    hipLaunchKernelGGL((context_upsample_bwd_kernel<SOFTMAX, true, false>), grid, dim3(256), 0, s, disp, w9, g, dw9, sums,
                       scale, h, w);
  else
    hipLaunchKernelGGL((context_upsample_bwd_kernel<SOFTMAX, false, true>), grid, dim3(256), 0, s, disp, w9, g, dw9, sums,
                       scale, h, w);
}

}  // namespace

extern "C" int dv_context_upsample_f32(const float* disp_low, const float* weights, float* out, int B, int h, int w,
                                       float scale, int apply_softmax, dv_stream_t stream) {
  DV_REQUIRE_PTR(disp_low);
  DV_REQUIRE_PTR(weights);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(B > 0 && h > 0 && w > 0, DV_ERR_SHAPE);
  DV_REQUIRE(dv_aligned16(weights) && dv_aligned16(out), DV_ERR_ALIGN);      // rows are 4*w floats: always 16-B multiples
  const size_t cells = (size_t)B * 4 * h * w;
  const unsigned nblk = (unsigned)((cells + 255) / 256);
  if (apply_softmax)
    hipLaunchKernelGGL((context_upsample_kernel<true>), dim3(nblk), dim3(256), 0, (hipStream_t)stream, disp_low,
                       weights, out, scale, h, w, cells);
  else
    hipLaunchKernelGGL((context_upsample_kernel<false>), dim3(nblk), dim3(256), 0, (hipStream_t)stream, disp_low,
                       weights, out, scale, h, w, cells);
  return dv_launch_status();
}

extern "C" int dv_context_upsample_bwd_f32(const float* disp_low, const float* weights, const float* grad_out,
                                           float* d_weights, float* d_disp, float* cell_sums, int B, int h, int w,
                                           float scale, int apply_softmax, dv_stream_t stream) {
  DV_REQUIRE_PTR(disp_low);
  DV_REQUIRE_PTR(weights);
  DV_REQUIRE_PTR(grad_out);
  DV_REQUIRE(d_weights != nullptr || d_disp != nullptr, DV_ERR_NULL);
  if (d_disp != nullptr) DV_REQUIRE_PTR(cell_sums);
  DV_REQUIRE(B > 0 && h > 0 && w > 0 && B <= 65535 && h <= 65535, DV_ERR_SHAPE);
  DV_REQUIRE(dv_aligned16(weights) && dv_aligned16(grad_out) && (d_weights == nullptr || dv_aligned16(d_weights)),
             DV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  if (apply_softmax)
    launch_bwd<true>(disp_low, weights, grad_out, d_weights, cell_sums, scale, B, h, w, d_disp != nullptr, s);
  else
    launch_bwd<false>(disp_low, weights, grad_out, d_weights, cell_sums, scale, B, h, w, d_disp != nullptr, s);
  int rc = dv_launch_status();
  if (rc != DV_OK || d_disp == nullptr) return rc;
  const size_t cells = (size_t)B * h * w;
  hipLaunchKernelGGL(context_upsample_ddisp_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, cell_sums,
                     d_disp, scale, h, w, cells);
  return dv_launch_status();
}
