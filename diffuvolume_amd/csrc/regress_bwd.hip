// Backward of K7 (regress.hip): gradient of trilinear x4 upsample -> softmax over disparity -> soft-argmax with respect
// to the quarter-resolution cost.  Replaces what autograd runs in training for F.interpolate(trilinear) + F.softmax(dim=1)
// + disparity_regression (SceneFlow/models/acv_ddim.py:457-480, KITTI12/models/pwcnet_ddim.py:682-710): it keeps a
// [B,192,H,W] softmax per head until backward and adds the upsampling gradient with atomics.
//
// Per fine pixel (Y, X), with c[d] the in-plane interpolated costs, v_k = l0 c[i0(k)] + l1 c[i1(k)], p = softmax(v):
//   dv_k = g p_k (k - disp)          dc[d] = sum_k (l0 [i0(k) = d] + l1 [i1(k) = d]) dv_k
// and dcost[b,d,y,x] = sum over the fine pixels whose bilinear taps include (y, x) of wy wx dc[d].
// The softmax is recomputed from the cost (same shift as the forward, regress_tail.h); disp is the forward's output.
// With e_k = exp(v_k - m), s = sum e_k:  dc[d] = (g / s) * sum_k (...) e_k (k - disp): the sums over k are finite whenever
// the cost is, so g == 0 gives dc == 0 exactly however peaked p is; NaN / Inf in g or cost propagate through the products.
//
// No atomics: a block owns a tile of quarter-resolution pixels with all D slices and writes each of their dcost elements
// once; it walks the tile's fine footprint (every fine pixel with a tap in the tile) in chunks of one pixel per thread,
// each thread computes dc[D] in registers, the chunk's columns go through LDS, and the tile's threads add the taps they
// own in ascending (Y, X).  Fine pixels on a tile border are evaluated by each tile they touch (x1.3 at 4 x 16 tiles).
#include "dv_common.h"
#include "regress_tail.h"
#include "../../include/diffuvolume_hip_train.h"

namespace {

constexpr int BT_TY = 4, BT_TX = 16;    // tile of quarter-resolution pixels
constexpr int BT_NT = 256;              // threads = fine pixels per chunk = (slice groups) x TY x TX
constexpr int BT_SG = BT_NT / (BT_TY * BT_TX);   // 4 groups of D / 4 slices: one gather thread per (group, y, x)

template <int D, bool ALIGN>
__global__ __launch_bounds__(BT_NT) void regress_bwd_fused_kernel(const float* __restrict__ cost,
                                                                  const float* __restrict__ disp,
                                                                  const float* __restrict__ grad,
                                                                  float* __restrict__ dcost, int h, int w,
                                                                  int tiles_y, int tiles_x, unsigned cost_bytes) {
  constexpr int K = 4 * D, DG = D / BT_SG;
  static_assert(D % BT_SG == 0, "slices split evenly over the gather groups");
  __shared__ float col[D][BT_NT];                 // dc of the chunk's fine pixels, [slice][pixel]: 48 KiB at D = 48
  __shared__ int rng[2 * (BT_TY + BT_TX)];        // fine tap ranges of the tile's rows and columns
  const int H = 4 * h, W = 4 * w;
  const int tid = threadIdx.x;
  const int tx_t = blockIdx.x % tiles_x;
  const int ty_t = (blockIdx.x / tiles_x) % tiles_y;
  const int b = blockIdx.x / (tiles_x * tiles_y);
  const int cy0 = ty_t * BT_TY, cx0 = tx_t * BT_TX;
  const int nty = min(BT_TY, h - cy0), ntx = min(BT_TX, w - cx0);     // ragged last tiles

  // the footprint comes from lin_src itself (tail_tap_range): clamping and align_corners change its width
  if (tid < BT_TY + BT_TX) {
    const bool row = tid < BT_TY;
    const int j = row ? tid : tid - BT_TY;
    int lo = 0, hi = -1;
    if (row ? j < nty : j < ntx) {
      if (row) tail_tap_range<ALIGN>(cy0 + j, h, H, lo, hi);
      else tail_tap_range<ALIGN>(cx0 + j, w, W, lo, hi);
    }
    rng[2 * tid] = lo;
    rng[2 * tid + 1] = hi;
  }
  __syncthreads();
  const int Y0 = rng[0], Y1 = rng[2 * (nty - 1) + 1];
  const int X0 = rng[2 * BT_TY], X1 = rng[2 * (BT_TY + ntx - 1) + 1];
  const int FX = X1 - X0 + 1, NF = (Y1 - Y0 + 1) * FX;

  // this thread as a gatherer: slices [sg * DG, sg * DG + DG) of tile pixel (gty, gtx)
  const int sg = tid / (BT_TY * BT_TX), gty = (tid / BT_TX) % BT_TY, gtx = tid % BT_TX;
  const bool gather = gty < nty && gtx < ntx;
  const int gy = cy0 + gty, gx = cx0 + gtx;
  const int ylo = rng[2 * gty], yhi = rng[2 * gty + 1];
  const int xlo = rng[2 * (BT_TY + gtx)], xhi = rng[2 * (BT_TY + gtx) + 1];
  float acc[DG];
#pragma unroll
  for (int i = 0; i < DG; ++i) acc[i] = 0.f;

  const size_t plane = (size_t)h * w;
  const int plane_bytes = __builtin_amdgcn_readfirstlane((int)(plane * sizeof(float)));
  // buffer loads with 32-bit offsets, as the forward: the host guarantees the cost tensor is below 2^31 bytes
  const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(cost), 0, (int)cost_bytes, 0x00020000);
  const unsigned ob = (unsigned)b * D * (unsigned)plane;

  for (int base = 0; base < NF; base += BT_NT) {
    // ---- one fine pixel per thread: dc[D] --------------------------------------------------------------------------
    const int f = base + tid;
    const bool live = f < NF;
    const int ff = live ? f : 0;                     // a dead lane recomputes pixel 0 of the footprint; nobody reads it
    const int fy = ff / FX;
    const int Y = Y0 + fy, X = X0 + (ff - fy * FX);
    int y0, y1, x0, x1;
    float hy0, hy1, wx0, wx1;
    lin_src<ALIGN>(Y, h, H, y0, y1, hy0, hy1);
    lin_src<ALIGN>(X, w, W, x0, x1, wx0, wx1);
    const int o00 = (int)((ob + y0 * w + x0) * 4u), o01 = (int)((ob + y0 * w + x1) * 4u);
    const int o10 = (int)((ob + y1 * w + x0) * 4u), o11 = (int)((ob + y1 * w + x1) * 4u);
    float c[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int so = d * plane_bytes;
      const float v00 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o00, so, 0));
      const float v01 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o01, so, 0));
      const float v10 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o10, so, 0));
      const float v11 = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, o11, so, 0));
      c[d] = hy0 * (wx0 * v00 + wx1 * v01) + hy1 * (wx0 * v10 + wx1 * v11);      // the forward's expression
    }
    const size_t pix = ((size_t)b * H + Y) * W + X;
    const float g = grad[pix], dsp = disp[pix];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (tail_shift_bin<ALIGN>(k, K)) {
        int i0, i1;
        float l0, l1;
        lin_src<ALIGN>(k, D, K, i0, i1, l0, l1);     // k is a compile-time constant after unrolling
        m = fmaxf(m, l0 * c[i0] + l1 * c[i1]);
      }
    }
    float dc[D];
#pragma unroll
    for (int d = 0; d < D; ++d) dc[d] = 0.f;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      int i0, i1;
      float l0, l1;
      lin_src<ALIGN>(k, D, K, i0, i1, l0, l1);
      const float e = dv_exp_le0(l0 * c[i0] + l1 * c[i1] - m);
      s += e;
      const float t = e * ((float)k - dsp);
      dc[i0] += l0 * t;
      dc[i1] += l1 * t;
    }
    const float scale = g * (1.f / s);               // g == 0: every dc is exactly (signed) zero
#pragma unroll
    for (int d = 0; d < D; ++d) col[d][tid] = dc[d] * scale;
    __syncthreads();

    // ---- the tile's threads add the taps of this chunk that they own, rows then columns ascending --------------------
    if (gather) {
      const int last = min(base + BT_NT, NF) - 1;
      const int r0 = max(ylo - Y0, base / FX), r1 = min(yhi - Y0, last / FX);
      for (int r = r0; r <= r1; ++r) {
        const float wy = tail_tap_weight<ALIGN>(Y0 + r, gy, h, H);
        for (int xx = xlo; xx <= xhi; ++xx) {
          const int idx = r * FX + (xx - X0) - base;
          if (idx < 0 || idx > last - base) continue;              // this tap belongs to another chunk
          const float wgt = wy * tail_tap_weight<ALIGN>(xx, gx, w, W);
#pragma unroll
          for (int i = 0; i < DG; ++i) acc[i] += wgt * col[sg * DG + i][idx];
        }
      }
    }
    __syncthreads();
  }
  if (gather) {
#pragma unroll
    for (int i = 0; i < DG; ++i) dcost[(((size_t)b * D + sg * DG + i) * h + gy) * w + gx] = acc[i];
  }
}

// ---- any D, any size: two passes through a [B,D,4h,4w] workspace ------------------------------------------------------
// Pass 1: one thread per fine pixel, its D interpolated costs and its D gradients in LDS (one column each per thread).
template <bool ALIGN>
__global__ void regress_bwd_columns_generic(const float* __restrict__ cost, const float* __restrict__ disp,
                                            const float* __restrict__ grad, float* __restrict__ ws, int D, int h,
                                            int w, size_t total) {
  extern __shared__ float cs[];  // [2][D][blockDim.x]
  const int H = 4 * h, W = 4 * w, K = 4 * D;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;        // no barrier below
  const int X = (int)(i % W);
  const int Y = (int)((i / W) % H);
  const size_t b = i / ((size_t)W * H);
  int y0, y1, x0, x1;
  float hy0, hy1, wx0, wx1;
  lin_src<ALIGN>(Y, h, H, y0, y1, hy0, hy1);
  lin_src<ALIGN>(X, w, W, x0, x1, wx0, wx1);
  const size_t plane = (size_t)h * w;
  const float* cb = cost + b * D * plane;
  const int st = blockDim.x;
  float* c = cs + threadIdx.x;
  float* dc = cs + (size_t)D * st + threadIdx.x;
  for (int d = 0; d < D; ++d) {
    const float* p = cb + (size_t)d * plane;
    c[d * st] = hy0 * (wx0 * p[(size_t)y0 * w + x0] + wx1 * p[(size_t)y0 * w + x1]) +
                hy1 * (wx0 * p[(size_t)y1 * w + x0] + wx1 * p[(size_t)y1 * w + x1]);
    dc[d * st] = 0.f;
  }
  auto vk = [&](int k, int& i0, int& i1, float& l0, float& l1) {
    lin_src<ALIGN>(k, D, K, i0, i1, l0, l1);
    return l0 * c[i0 * st] + l1 * c[i1 * st];
  };
  int i0, i1;
  float l0, l1;
  float m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmaxf(m, vk(k, i0, i1, l0, l1));
  const float dsp = disp[i];
  float s = 0.f;
  for (int k = 0; k < K; ++k) {
    const float e = expf(vk(k, i0, i1, l0, l1) - m);
    s += e;
    const float t = e * ((float)k - dsp);
    dc[i0 * st] += l0 * t;
    dc[i1 * st] += l1 * t;
  }
  const float scale = grad[i] * (1.f / s);
  const size_t fine = (size_t)H * W;
  float* o = ws + b * D * fine + (size_t)Y * W + X;
  for (int d = 0; d < D; ++d) o[(size_t)d * fine] = dc[d * st] * scale;
}

// Pass 2: one thread per dcost element adds its taps, rows then columns ascending.
template <bool ALIGN>
__global__ void regress_bwd_gather_generic(const float* __restrict__ ws, float* __restrict__ dcost, int h, int w,
                                           size_t total) {
  const int H = 4 * h, W = 4 * w;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int x = (int)(i % w);
  const int y = (int)((i / w) % h);
  const size_t bd = i / ((size_t)w * h);
  int ylo, yhi, xlo, xhi;
  tail_tap_range<ALIGN>(y, h, H, ylo, yhi);
  tail_tap_range<ALIGN>(x, w, W, xlo, xhi);
  const float* src = ws + bd * (size_t)H * W;
  float acc = 0.f;
  for (int Y = ylo; Y <= yhi; ++Y) {
    const float wy = tail_tap_weight<ALIGN>(Y, y, h, H);
    for (int X = xlo; X <= xhi; ++X) acc += wy * tail_tap_weight<ALIGN>(X, x, w, W) * src[(size_t)Y * W + X];
  }
  dcost[i] = acc;
}

inline bool fused_applies(int B, int D, int h, int w) {
  return D == 48 && (size_t)B * D * h * w * sizeof(float) < 0x80000000ull;    // the forward's predicate (launch_tail)
}

constexpr int GEN_THREADS = 64;

}  // namespace

extern "C" size_t dv_upsample_softmax_regress_bwd_workspace_floats(int B, int D, int h, int w) {
  if (B <= 0 || D <= 0 || h <= 0 || w <= 0 || fused_applies(B, D, h, w)) return 0;
  return (size_t)B * D * 16 * h * w;
}

extern "C" int dv_upsample_softmax_regress_bwd_f32(const float* cost, const float* disp, const float* grad_disp,
                                                   float* dcost, float* workspace, int B, int D, int h, int w,
                                                   int align_corners, dv_stream_t stream) {
  DV_REQUIRE_PTR(cost);
  DV_REQUIRE_PTR(disp);
  DV_REQUIRE_PTR(grad_disp);
  DV_REQUIRE_PTR(dcost);
  DV_REQUIRE(B > 0 && D > 0 && h > 0 && w > 0, DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (fused_applies(B, D, h, w)) {
    const int tiles_y = (h + BT_TY - 1) / BT_TY, tiles_x = (w + BT_TX - 1) / BT_TX;
    const size_t blocks = (size_t)B * tiles_y * tiles_x;
    DV_REQUIRE(blocks <= 0x7fffffffull, DV_ERR_UNSUPPORTED);
    const unsigned cost_bytes = (unsigned)((size_t)B * D * h * w * sizeof(float));
    if (align_corners)
      hipLaunchKernelGGL((regress_bwd_fused_kernel<48, true>), dim3((unsigned)blocks), dim3(BT_NT), 0, s, cost, disp,
                         grad_disp, dcost, h, w, tiles_y, tiles_x, cost_bytes);
    else
      hipLaunchKernelGGL((regress_bwd_fused_kernel<48, false>), dim3((unsigned)blocks), dim3(BT_NT), 0, s, cost, disp,
                         grad_disp, dcost, h, w, tiles_y, tiles_x, cost_bytes);
    return dv_launch_status();
  }
  DV_REQUIRE_PTR(workspace);
  const size_t lds = (size_t)2 * D * GEN_THREADS * sizeof(float);
  DV_REQUIRE(lds <= 64 * 1024, DV_ERR_UNSUPPORTED);
  const size_t fine = (size_t)B * 16 * h * w, coarse = (size_t)B * D * h * w;
  const size_t blocks1 = (fine + GEN_THREADS - 1) / GEN_THREADS, blocks2 = (coarse + 255) / 256;
  DV_REQUIRE(blocks1 <= 0x7fffffffull && blocks2 <= 0x7fffffffull, DV_ERR_UNSUPPORTED);
  if (align_corners) {
    hipLaunchKernelGGL((regress_bwd_columns_generic<true>), dim3((unsigned)blocks1), dim3(GEN_THREADS), lds, s, cost,
                       disp, grad_disp, workspace, D, h, w, fine);
    hipLaunchKernelGGL((regress_bwd_gather_generic<true>), dim3((unsigned)blocks2), dim3(256), 0, s, workspace, dcost,
                       h, w, coarse);
  } else {
    hipLaunchKernelGGL((regress_bwd_columns_generic<false>), dim3((unsigned)blocks1), dim3(GEN_THREADS), lds, s, cost,
                       disp, grad_disp, workspace, D, h, w, fine);
    hipLaunchKernelGGL((regress_bwd_gather_generic<false>), dim3((unsigned)blocks2), dim3(256), 0, s, workspace, dcost,
                       h, w, coarse);
  }
  return dv_launch_status();
}
