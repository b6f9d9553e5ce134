// The differentiable part of the refinement network's input (KITTI12/models/pwcnet_ddim.py:719-725), for training:
//   F    = warp(right, disp)                        (warp_taps.h: the taps and the 0.999 validity of the eval kernel)
//   diff = left - F                                  [B,C,H,W]
//   corr = build_corrleation_volume(left, F, 24, 1)  [B,49,H,W]   (negative shifts: the reference's wrap-around pairing)
// Forward: refine_inputs.hip's kernel without the channels that need no gradient path of their own (left, dispupsample,
// disp): the same staging, the same order of accumulation over the channels and the same acc * (1/C), so diff and corr are
// channels [0,C) and [3C+1,3C+50) of dv_refine_inputs_f32 bit for bit.
//
// Backward, without atomics, every element written once in a fixed order, F recomputed:
//   pass 1 (block = 128 columns of one row, channels in chunks of 16 through LDS):
//     threads 0..127   dL[c,x]  = g_diff + (1/C) (sum_i g_corr[i+24,x] F[c,x-i] + wrap)              -- F staged as in the forward
//     threads 128..255 dF[c,x'] = -g_diff + (1/C) (sum_i g_corr[i+24,x'+i] L[c,x'+i] + wrap)         -- L staged with its halo
//                      ddisp    = -m W/(W-1) sum_c dF (horizontal differences of R at the taps, weighted by the two rows)
//                      workspace[c,x'] = m dF[c,x']
//   pass 2 (thread = one source pixel (ys, xs), all channels in registers): the transpose of the bilinear gather.  The
//     vertical tap depends on y only (y0 is y-1 or y), so source row ys is fed by rows ys-1, ys, ys+1 at most; for each of
//     them the block stages x0(x) and the two horizontal weights of 256 columns at a time in LDS (computed once for all
//     channels) and every thread scans them in ascending x for the columns whose x0 is xs or xs-1.  The order is y
//     ascending, then x ascending, whatever the disparity: exact for any fan-in, the same bits on every launch.
#include "dv_common.h"
#include "warp_taps.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int TX = 128, MD = 24, NSH = 2 * MD + 1, CMAX = 32;
constexpr int SW = TX + 2 * MD;       // the eval kernel's staged columns per channel
constexpr int CCH = 16;               // channels per LDS chunk of the backward
constexpr int SB = TX + MD;           // staged columns per channel of the backward (tile + one halo)
constexpr int CG = 4;                 // channels whose global loads pass 1 issues together
constexpr int TS = 256;               // columns per scan tile of pass 2
constexpr int LK = 8;                 // matches a thread of pass 2 notes before they are worked off
constexpr int NO_COLUMN = 0x40000000; // x0 of a staged slot right of the image: no source column is that far

struct FwdArgs {
  const float* left;    // [B,C,H,W]
  const float* right;   // [B,C,H,W]
  const float* disp;    // [B,H,W]
  float* diff;          // [B,C,H,W]
  float* corr;          // [B,49,H,W]
  int B, C, H, W;
};

__global__ __launch_bounds__(256) void warp_corr_kernel(FwdArgs a) {
  __shared__ float frw_s[CMAX][SW];      // warped right features, columns x0-MD .. x0+TX+MD-1
  __shared__ float wrap_s[CMAX][MD];     // columns W-MD .. W-1 of the same row (first tile only)
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TX, y = blockIdx.y, b = blockIdx.z;
  const int W = a.W, H = a.H, C = a.C;
  const size_t plane = (size_t)H * W;
  const float* lb = a.left + (size_t)b * C * plane;
  const float* rb = a.right + (size_t)b * C * plane;
  const float* db = a.disp + (size_t)b * plane + (size_t)y * W;

  // ---- stage the warped row segment: thread = column, loop over channels (as refine_inputs_kernel) ----
  for (int col = tid; col < SW + MD; col += 256) {
    const bool wrap = col >= SW;
    if (wrap && x0 != 0) break;
    const int x = wrap ? W - MD + (col - SW) : x0 - MD + col;
    if ((unsigned)x < (unsigned)W) {
      const Taps t = make_taps((float)x, (float)y, db[x], W, H);
      for (int c = 0; c < C; ++c) {
        const float v = warp_one(rb + (size_t)c * plane, t, W, H);
        if (wrap) wrap_s[c][col - SW] = v; else frw_s[c][col] = v;
      }
    } else {
      for (int c = 0; c < C; ++c)
        if (wrap) wrap_s[c][col - SW] = 0.f; else frw_s[c][col] = 0.f;
    }
  }
  __syncthreads();

  // ---- outputs: two threads per pixel; half 0: left - frw and shifts -24..0; half 1: shifts 1..24 ----
  const int px = tid & (TX - 1), half = tid >> 7;
  const int x = x0 + px;
  if (x >= W) return;
  const size_t row = (size_t)y * W + x;
  float lv[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) lv[c] = c < C ? lb[(size_t)c * plane + row] : 0.f;
  const float inv_c = 1.f / (float)C;
  if (half == 0) {
    float* ob = a.diff + (size_t)b * C * plane + row;
#pragma unroll
    for (int c = 0; c < CMAX; ++c)
      if (c < C) ob[(size_t)c * plane] = lv[c] - frw_s[c][MD + px];
  }
  float* cvb = a.corr + (size_t)b * NSH * plane + row;
  const int s_lo = half == 0 ? -MD : 1, s_hi = half == 0 ? 0 : MD;
  for (int i = s_lo; i <= s_hi; ++i) {
    float acc = 0.f;
    if (i >= 0) {
      if (x >= i) {                                    // ref[x] * tgt[x - i]
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
          if (c < C) acc += lv[c] * frw_s[c][MD + px - i];
      }
    } else if (x < -i) {                               // first |i| columns against the LAST |i| columns (as written)
#pragma unroll
      for (int c = 0; c < CMAX; ++c)
        if (c < C) acc += lv[c] * wrap_s[c][MD + i + x];
    }
    cvb[(size_t)(i + MD) * plane] = acc * inv_c;
  }
}

struct BwdArgs {
  const float* left;    // [B,C,H,W]
  const float* right;   // [B,C,H,W]
  const float* disp;    // [B,H,W]
  const float* g_diff;  // [B,C,H,W]
  const float* g_corr;  // [B,49,H,W]
  float* dleft;         // [B,C,H,W] or NULL
  float* ddisp;         // [B,H,W] or NULL
  float* dfm;           // [B,C,H,W] m * dF for pass 2, or NULL
  int B, C, H, W;
};

// pass 1: dleft, ddisp and the masked gradient of the warped map
__global__ __launch_bounds__(256, 4) void warp_corr_bwd_kernel(BwdArgs a) {
  __shared__ float f_s[CCH][SB];         // F, columns x0-MD .. x0+TX-1                (for dleft)
  __shared__ float fw_s[CCH][MD];        // F, columns W-MD .. W-1                      (first tile only)
  __shared__ float l_s[CCH][SB];         // left, columns x0 .. x0+TX+MD-1              (for dF)
  __shared__ float lw_s[CCH][MD];        // left, columns 0 .. MD-1                     (tiles that reach the last MD columns)
  __shared__ float gw_s[MD][MD];         // g_corr[MD-k, j], k = 1..MD, j < MD: the wrap-around shifts (those two kinds of tile)
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TX, y = blockIdx.y, b = blockIdx.z;
  const int W = a.W, H = a.H, C = a.C;
  const size_t plane = (size_t)H * W;
  const size_t rowo = (size_t)y * W;
  const float* lb = a.left + (size_t)b * C * plane + rowo;
  const float* rb = a.right + (size_t)b * C * plane;
  const float* db = a.disp + (size_t)b * plane + rowo;
  const float* gdb = a.g_diff + (size_t)b * C * plane + rowo;
  const float* gcb = a.g_corr + (size_t)b * NSH * plane + rowo;
  const bool want_l = a.dleft != nullptr, want_f = a.dfm != nullptr || a.ddisp != nullptr;
  const bool first = x0 == 0, last = x0 + TX > W - MD;      // block-uniform: which wrap segments this tile needs

  const int px = tid & (TX - 1), half = tid >> 7;
  const int x = x0 + px;
  const bool live = x < W;
  const float inv_c = 1.f / (float)C;

  // The wrap-around terms touch the first MD columns of a row (dleft) and the last MD (dF), both through g_corr[MD-k, j]
  // with j < MD: staged once per block (kept in registers they cost every thread 24 VGPRs; read from memory where they
  // are used, a dependent load per term, they made pass 1 0.2 ms slower at [4,32,256,512]).  The barriers of the first
  // chunk order the staging before its use.
  if (first || last)
    for (int e = tid; e < MD * MD; e += 256) gw_s[e / MD][e % MD] = gcb[(size_t)(MD - 1 - e / MD) * plane + e % MD];

  // per-thread coefficients: the gradients of corr that meet this pixel through the shifts 0..MD
  float gc[MD + 1];                     // half 0: g_corr[i+MD, x];  half 1: the diagonal g_corr[i+MD, x+i]
  Taps t{};
  float wy0 = 0.f, wy1 = 0.f, dsum = 0.f;
#pragma unroll
  for (int i = 0; i <= MD; ++i) gc[i] = 0.f;
  if (live && half == 0 && want_l) {
#pragma unroll
    for (int i = 0; i <= MD; ++i)
      if (i <= x) gc[i] = gcb[(size_t)(i + MD) * plane + x];          // shift i > x has no partner: it stays 0
  }
  if (live && half == 1 && want_f) {
#pragma unroll
    for (int i = 0; i <= MD; ++i)
      if (x + i < W) gc[i] = gcb[(size_t)(i + MD) * plane + x + i];
    t = make_taps((float)x, (float)y, db[x], W, H);
    warp_row_weights((float)y, H, wy0, wy1);
  }

  for (int c0 = 0; c0 < C; c0 += CCH) {
    const int cn = min(CCH, C - c0);
    __syncthreads();                                       // the previous chunk has been read
    if (want_l) {                                          // F: thread = column, loop over the chunk's channels
      for (int col = tid; col < SB + MD; col += 256) {
        const bool wrap = col >= SB;
        if (wrap && !first) break;
        const int xc = wrap ? W - MD + (col - SB) : x0 - MD + col;
        if ((unsigned)xc < (unsigned)W) {
          const Taps tc = make_taps((float)xc, (float)y, db[xc], W, H);
          for (int c = 0; c < cn; ++c) {
            const float v = warp_one(rb + (size_t)(c0 + c) * plane, tc, W, H);
            if (wrap) fw_s[c][col - SB] = v; else f_s[c][col] = v;
          }
        } else {
          for (int c = 0; c < cn; ++c)
            if (wrap) fw_s[c][col - SB] = 0.f; else f_s[c][col] = 0.f;
        }
      }
    }
    if (want_f) {                                          // left: coalesced along the row
      for (int e = tid; e < cn * SB; e += 256) {
        const int c = e / SB, col = e - c * SB;
        const int xc = x0 + col;
        l_s[c][col] = xc < W ? lb[(size_t)(c0 + c) * plane + xc] : 0.f;
      }
      if (last)
        for (int e = tid; e < cn * MD; e += 256) {
          const int c = e / MD, col = e - c * MD;
          lw_s[c][col] = lb[(size_t)(c0 + c) * plane + col];          // W >= MD
        }
    }
    __syncthreads();
    if (!live) continue;

    // Channels go in groups of CG: the group's global loads are issued together, ahead of the LDS sums that do not need
    // them (one channel at a time, every channel waited for its own loads: the loop was a chain of memory round trips).
    // A channel index past the chunk is clamped for the loads and its result is dropped.
    if (half == 0) {
      if (!want_l) continue;
      float* __restrict__ ob = a.dleft + (size_t)b * C * plane + rowo + x;
      for (int c = 0; c < cn; c += CG) {
        float g[CG];
#pragma unroll
        for (int u = 0; u < CG; ++u) g[u] = gdb[(size_t)(c0 + min(c + u, cn - 1)) * plane + x];
#pragma unroll
        for (int u = 0; u < CG; ++u) {
          const int cc = min(c + u, cn - 1);
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i <= MD; ++i) acc += gc[i] * f_s[cc][MD + px - i];         // F is 0 left of the image
          if (x < MD) {                                 // the first MD columns only
#pragma unroll
            for (int k = 1; k <= MD; ++k)
              if (x < k) acc += gw_s[k - 1][x] * fw_s[cc][MD - k + x];                 // column W - k + x
          }
          if (c + u < cn) ob[(size_t)(c0 + c + u) * plane] = g[u] + acc * inv_c;
        }
      }
    } else {
      if (!want_f) continue;
      // the four sources of this pixel: addresses clamped, out-of-range taps count as 0
      const bool xl = (unsigned)t.x0 < (unsigned)W, xr = (unsigned)(t.x0 + 1) < (unsigned)W;
      const bool yt = (unsigned)t.y0 < (unsigned)H, yb = (unsigned)(t.y0 + 1) < (unsigned)H;
      const int xa = min(max(t.x0, 0), W - 1), xb = min(max(t.x0 + 1, 0), W - 1);
      const int ya = min(max(t.y0, 0), H - 1), yc = min(max(t.y0 + 1, 0), H - 1);
      const size_t o00 = (size_t)ya * W + xa, o01 = (size_t)ya * W + xb, o10 = (size_t)yc * W + xa, o11 = (size_t)yc * W + xb;
      const bool want_d = a.ddisp != nullptr;
      for (int c = 0; c < cn; c += CG) {
        float g[CG], r00[CG], r01[CG], r10[CG], r11[CG];
#pragma unroll
        for (int u = 0; u < CG; ++u) {
          const size_t ch = (size_t)(c0 + min(c + u, cn - 1)) * plane;
          g[u] = gdb[ch + x];
          if (want_d) {
            const float* __restrict__ rp = rb + ch;
            r00[u] = rp[o00]; r01[u] = rp[o01]; r10[u] = rp[o10]; r11[u] = rp[o11];
          }
        }
#pragma unroll
        for (int u = 0; u < CG; ++u) {
          const int cc = min(c + u, cn - 1);
          float acc = 0.f;
#pragma unroll
          for (int i = 0; i <= MD; ++i) acc += gc[i] * l_s[cc][px + i];               // left is 0 right of the image
          if (x >= W - MD) {                            // the last MD columns only
#pragma unroll
            for (int k = 1; k <= MD; ++k)
              if (x >= W - k) acc += gw_s[k - 1][x - (W - k)] * lw_s[cc][x - (W - k)];
          }
          const float df = acc * inv_c - g[u];
          if (c + u < cn) {
            if (a.dfm) a.dfm[((size_t)b * C + c0 + c + u) * plane + rowo + x] = df * t.valid;
            if (want_d) {
              const float n = xl && yt ? r00[u] : 0.f, e = xr && yt ? r01[u] : 0.f;
              const float sw = xl && yb ? r10[u] : 0.f, se = xr && yb ? r11[u] : 0.f;
              dsum += df * ((e - n) * wy0 + (se - sw) * wy1);
            }
          }
        }
      }
    }
  }
  if (live && half == 1 && a.ddisp) {
    const float scale = (float)W / (float)(W > 1 ? W - 1 : 1);      // d ix / d disp = -W / (W - 1)
    a.ddisp[(size_t)b * plane + rowo + x] = -t.valid * scale * dsum;
  }
}

// pass 2: dright[c, ys, xs] = sum over the output pixels whose taps land on (ys, xs) of weight * (m dF).
// A thread scans the staged x0 of a tile in ascending x and notes its own matches in its column of an LDS list; the lists
// are then worked off with every lane on a match of its own (its 32 channel loads in flight together).  Adding while
// scanning instead ran every match alone -- at one scan position at most two lanes of a wave match -- and cost 2.5 ms of a
// 3.0 ms backward at [4,32,256,512].  A list is flushed as soon as any lane of the wave could overflow it, so any fan-in is
// exact, and a thread still adds its columns in ascending x.  Tiles none of whose taps reach the block's columns are
// skipped (block-uniform, by __syncthreads_or).
__global__ __launch_bounds__(256) void warp_scatter_rows_kernel(const float* __restrict__ disp, const float* __restrict__ dfm,
                                                                float* __restrict__ dright, int C, int H, int W) {
  __shared__ __attribute__((aligned(16))) int x0_s[TS];
  __shared__ float wa_s[TS], wb_s[TS];   // weight onto source column x0 / x0 + 1 of THIS source row
  __shared__ int list_s[LK][TS];         // per thread: (column within the tile) * 2 + (x0 + 1 == xs)
  const int tid = threadIdx.x;
  const int bx0 = blockIdx.x * TS;
  const int xs = bx0 + tid, ys = blockIdx.y, b = blockIdx.z;
  const size_t plane = (size_t)H * W;
  const bool live = xs < W;
  float acc[CMAX];
#pragma unroll
  for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
  for (int y = max(ys - 1, 0); y <= min(ys + 1, H - 1); ++y) {
    const int y0 = make_taps(0.f, (float)y, 0.f, W, H).y0;         // depends on y only: block-uniform
    const bool top = y0 == ys, bottom = y0 + 1 == ys;
    if (!top && !bottom) continue;
    const float* db = disp + (size_t)b * plane + (size_t)y * W;
    const float* fb = dfm + (size_t)b * C * plane + (size_t)y * W;
    for (int t0 = 0; t0 < W; t0 += TS) {
      __syncthreads();                                             // the previous tile has been scanned
      int reaches = 0;
      if (t0 + tid < W) {
        const Taps t = make_taps((float)(t0 + tid), (float)y, db[t0 + tid], W, H);
        x0_s[tid] = t.x0;
        wa_s[tid] = top ? t.nw : t.sw;
        wb_s[tid] = top ? t.ne : t.se;
        reaches = (unsigned)t.x0 - (unsigned)(bx0 - 1) <= (unsigned)TS;      // x0 or x0 + 1 is one of the block's columns
      } else {
        x0_s[tid] = NO_COLUMN;
      }
      if (!__syncthreads_or(reaches)) continue;
      const float* pt = fb + t0;
      int cnt = 0;
      auto flush = [&]() {
        for (int m = 0; m < LK; ++m) {
          if (!__any(m < cnt)) break;
          if (m < cnt) {
            const int e = list_s[m][tid], j = e >> 1;
            const float w = (e & 1) ? wb_s[j] : wa_s[j];
            // all CMAX loads are issued, without a branch on C between them (channels past C re-read the last one and
            // are never written): guarded one by one, every load waited for the one before it
            const float* p = pt + j;
            float v[CMAX];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) v[c] = p[(size_t)min(c, C - 1) * plane];
#pragma unroll
            for (int c = 0; c < CMAX; ++c) acc[c] += w * v[c];
          }
        }
        cnt = 0;
      };
      for (int j0 = 0; j0 < TS; j0 += 4) {
        const int4 v = *reinterpret_cast<const int4*>(&x0_s[j0]);
        const int x0v[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const unsigned dx = (unsigned)xs - (unsigned)x0v[u];
          if (live && dx <= 1u) {
            list_s[cnt][tid] = ((j0 + u) << 1) | (int)dx;
            ++cnt;
          }
        }
        if (__any(cnt > LK - 4)) flush();                          // four more matches might not fit
      }
      if (__any(cnt > 0)) flush();
    }
  }
  if (!live) return;
  float* ob = dright + (size_t)b * C * plane + (size_t)ys * W + xs;
#pragma unroll
  for (int c = 0; c < CMAX; ++c)
    if (c < C) ob[(size_t)c * plane] = acc[c];
}

}  // namespace

extern "C" int dv_warp_corr_f32(const float* left, const float* right, const float* disp, float* diff, float* corr, int B,
                                int C, int H, int W, int maxshift, dv_stream_t stream) {
  DV_REQUIRE_PTR(left);
  DV_REQUIRE_PTR(right);
  DV_REQUIRE_PTR(disp);
  DV_REQUIRE_PTR(diff);
  DV_REQUIRE_PTR(corr);
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE(C <= CMAX && maxshift == MD && W >= MD, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(B <= 65535 && H <= 65535, DV_ERR_SHAPE);
  FwdArgs a{left, right, disp, diff, corr, B, C, H, W};
  hipLaunchKernelGGL(warp_corr_kernel, dim3((unsigned)((W + TX - 1) / TX), (unsigned)H, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, a);
  return dv_launch_status();
}

extern "C" size_t dv_warp_corr_bwd_workspace_floats(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)B * C * H * W;                           // m * dF, one feature map
}

extern "C" int dv_warp_corr_bwd_f32(const float* left, const float* right, const float* disp, const float* g_diff,
                                    const float* g_corr, float* dleft, float* dright, float* ddisp, float* workspace, int B,
                                    int C, int H, int W, int maxshift, dv_stream_t stream) {
  DV_REQUIRE_PTR(left);
  DV_REQUIRE_PTR(right);
  DV_REQUIRE_PTR(disp);
  DV_REQUIRE_PTR(g_diff);
  DV_REQUIRE_PTR(g_corr);
  DV_REQUIRE(dleft || dright || ddisp, DV_ERR_NULL);
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE(C <= CMAX && maxshift == MD && W >= MD, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(B <= 65535 && H <= 65535, DV_ERR_SHAPE);
  if (dright) DV_REQUIRE_PTR(workspace);
  BwdArgs a{left, right, disp, g_diff, g_corr, dleft, ddisp, dright ? workspace : nullptr, B, C, H, W};
  hipLaunchKernelGGL(warp_corr_bwd_kernel, dim3((unsigned)((W + TX - 1) / TX), (unsigned)H, (unsigned)B), dim3(256), 0,
                     (hipStream_t)stream, a);
  if (dright) {
    const int e = dv_launch_status();
    if (e != DV_OK) return e;
    hipLaunchKernelGGL(warp_scatter_rows_kernel, dim3((unsigned)((W + TS - 1) / TS), (unsigned)H, (unsigned)B), dim3(256),
                       0, (hipStream_t)stream, disp, workspace, dright, C, H, W);
  }
  return dv_launch_status();
}
