// Backward of nn.ConvTranspose3d((4,4,4), stride 2, padding 1, bias=False): the IGEV hourglass's conv3_up / conv2_up /
// conv1_up (KITTI15/core/igev_stereo_ddim.py:44-51, BasicConv deconv core/submodule.py:9-35), 48 -> 32, 32 -> 16, 16 -> 8.
// w [Ci][Co][4][4][4], x [B,Ci,D,H,W], g = d loss / d out [B,Co,2D,2H,2W], t in [0,4)^3, g zero outside the volume:
//   dx[b,ci,i]  = sum_{co,t} g[b,co,2i-1+t] * w[ci,co,t]        (a stride-2 4x4x4 pad-1 convolution Co -> Ci)
//   dw[ci,co,t] = sum_{b,i}  x[b,ci,i]      * g[b,co,2i-1+t]
// Both are implicit GEMMs on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32; no atomics anywhere, so the
// bits do not depend on the launch.
//
// INPUT GRADIENT (M = positions of x, N = Ci, K = Co*64).  A block owns a 2 x 8 x 8 brick of x positions of one batch
// item and up to 48 input channels (NT 16-wide N tiles); its 4 waves own two M tiles each (one M tile = 2 rows x 8
// columns).  Per K chunk of 4 output channels the g halo [4][6][18][2 x 10] is staged in LDS with its rows phase-split
// (even g columns, then odd ones), so the 8 columns 2q-1+tx of an MFMA step are adjacent dwords; one MFMA step takes
// the 4 channels of the chunk at one tap.  Weights come packed as [tap][Co4][Cip] (zeros in the padding) and are read
// from global memory (L1/L2 resident: at most 64 x 32 x 48 floats), one read per N tile reused by both M tiles.
// Every dx element is ONE fma chain over its Co*64 products (padding taps / channels enter as exact zeros).
// LDS bank map (ds_read_b32, conflicts inside a 32-lane half): lane l reads channel l >> 4 at M row l & 15; the channel
// stride is 16 mod 32, two halo rows are 8 mod 32, the 8 columns adjacent: 32 different banks.
// Vector path (W % 4 == 0, 16-byte aligned g and dx): float2 halo loads, float4 stores; scalar path otherwise.
//
// WEIGHT GRADIENT (M = Ci, N = Co, K = B*D*H*W), the structure of conv3d_wgrad.hip: bricks of 2 x 4 x 8 x positions,
// the x tile [ci][64] and the g halo [co][2][10][2 x 9] (phase-split rows) in LDS, the K dimension split over blocks
// into the caller's workspace, a second kernel adding the splits in split order.  64 taps x one 16 x 16 accumulator
// tile would be 256 accumulator registers per lane, so the z tap is a grid dimension: a block holds the 16 (ty, tx)
// accumulators (64 registers) of ONE tz across its whole brick range and stages only the g rows 2z-1+tz of that tz
// (x is staged four times over, g twice).  A block is MW x NW x KW waves: MW x NW (16 ci, 16 co) tiles, picked by the
// launcher from the channel counts (MW in {1,2,3}, NW in {1,2}), and for narrow layers KW = 4 / (MW NW) waves per tile
// that deal the brick's 8 (z, y) rows among themselves, so that 4 waves share the staging (48 -> 32: 3 x 2 x 1,
// 32 -> 16: 2 x 1 x 2, 16 -> 8: 1 x 1 x 4 with the upper 8 columns of the N tile zeros).  After its last brick K wave
// k = 1 .. KW-1 hands its accumulators to K wave 0 through LDS, in that order.  Summation order of one dw element:
// per K wave one fma chain over its rows (64 / KW positions per brick) of the split's bricks, the KW chains added in
// wave order, then the splits added in split order.  LDS bank map as in conv3d_wgrad.hip: per-channel strides 2 mod 32,
// the positions of one step adjacent.
//
// Registers and spills (hipcc -O3 -fno-slp-vectorize, gfx950, .vgpr_count / .vgpr_spill_count of the code object):
//   deconv3d_k4_dgrad_kernel<NT = 1 | 2 | 3>   98 | 105 | 110 VGPR, 0 spilled (vector and scalar path alike), 34 560 B LDS
//   deconv3d_k4_wgrad_kernel<MW, NW, KW>       100 - 104 VGPR (KW = 1), 196 (KW = 2), 144 (KW = 4), 64 of them the 16
//                                              accumulator tiles; 0 spilled; 28 928 B (1 x 1 x 4) ... 62 080 B (3 x 2 x 1) LDS
#include "wgrad_splitk.h"

namespace {

bool valid_shape(int B, int Ci, int D, int H, int W, int Co) {
  return B > 0 && Ci > 0 && D > 0 && H > 0 && W > 0 && Co > 0;
}

// ------------------------------------------------------------------------------------------------ input gradient
constexpr int DG_TZ = 2, DG_TY = 8, DG_TX = 8, DG_THREADS = 256, DG_KC = 4, DG_NT_MAX = 3;
constexpr int DG_EZ = 2 * DG_TZ + 2, DG_EY = 2 * DG_TY + 2;      // g rows 2i-1 .. 2i+2 of the brick
constexpr int DG_EXH = DG_TX + 2, DG_ROW = 2 * DG_EXH;           // g columns 2*ox0-2 .. 2*ox0+2*TX+1, per phase
constexpr int DG_GS = DG_EZ * DG_EY * DG_ROW;                    // per-channel stride of the halo
static_assert(DG_GS % 32 == 16 && (2 * DG_ROW) % 32 == 8, "bank map of the A operand");
static_assert(DG_TZ * DG_TY == 2 * 2 * (DG_THREADS / 64) && DG_TX == 8, "two M tiles of 2 rows x 8 columns per wave");

struct DgGeo {
  int nt, groups, cop, cip;
};

DgGeo dg_geo(int Ci, int Co) {
  DgGeo q;
  const int nm = (Ci + 15) / 16;
  q.nt = nm < DG_NT_MAX ? nm : DG_NT_MAX;
  q.groups = (nm + q.nt - 1) / q.nt;
  q.cop = (Co + DG_KC - 1) / DG_KC * DG_KC;
  q.cip = q.groups * q.nt * 16;
  return q;
}

// wp[t][co][ci] = w[ci][co][t], zeros past Co / Ci
__global__ __launch_bounds__(256) void dgrad_pack_kernel(const float* __restrict__ w, float* __restrict__ wp, int Ci,
                                                         int Co, int cop, int cip) {
  const long long n = 64ll * cop * cip;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    const int ci = (int)(e % cip), co = (int)((e / cip) % cop), t = (int)(e / ((long long)cip * cop));
    wp[e] = (ci < Ci && co < Co) ? w[((size_t)ci * Co + co) * 64 + t] : 0.f;
  }
}

struct DgArgs {
  const float* g;    // [B, Co, 2D, 2H, 2W]
  const float* wp;   // [64, cop, cip]
  float* dx;         // [B, Ci, D, H, W]
  int B, Ci, D, H, W, Co, cop, cip;
  int nbz, nby, nbx;
};

template <int NT, bool VEC>
__global__ __launch_bounds__(DG_THREADS, 2) void deconv3d_k4_dgrad_kernel(DgArgs a) {
  __shared__ float gs[DG_KC * DG_GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  unsigned r = blockIdx.x;
  const int bx = (int)(r % a.nbx); r /= a.nbx;
  const int by = (int)(r % a.nby); r /= a.nby;
  const int bz = (int)(r % a.nbz); r /= a.nbz;
  const int b = (int)r;
  const int oz0 = bz * DG_TZ, oy0 = by * DG_TY, ox0 = bx * DG_TX;
  const int gz0 = 2 * oz0 - 1, gy0 = 2 * oy0 - 1, gx0 = 2 * ox0 - 2;
  const int Dg = 2 * a.D, Hg = 2 * a.H, Wg = 2 * a.W;
  const size_t gplane = (size_t)Dg * Hg * Wg;
  const int pz = wave >> 1, ybase = (wave & 1) * 4;
  const int n0 = blockIdx.y * NT * 16;

  f32x4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  const float* ard = gs + lk * DG_GS + (2 * pz * DG_EY + 2 * (ybase + (li >> 3))) * DG_ROW + (li & 7);
  const float* brd = a.wp + (size_t)lk * a.cip + n0 + li;

  for (int c0 = 0; c0 < a.cop; c0 += DG_KC) {
    __syncthreads();                                      // the previous chunk's reads are done
    if (VEC) {
      for (int idx = tid; idx < DG_KC * DG_EZ * DG_EY * DG_EXH; idx += DG_THREADS) {
        const int j = idx % DG_EXH;
        const int rest = idx / DG_EXH;
        const int ey = rest % DG_EY, ez = (rest / DG_EY) % DG_EZ, c = rest / (DG_EY * DG_EZ);
        const int co = c0 + c, gz = gz0 + ez, gy = gy0 + ey, gx = gx0 + 2 * j;
        float2 v = make_float2(0.f, 0.f);
        if (co < a.Co && gz >= 0 && gz < Dg && gy >= 0 && gy < Hg && gx >= 0 && gx < Wg)   // gx even, Wg even: a pair
          v = *reinterpret_cast<const float2*>(a.g + ((size_t)b * a.Co + co) * gplane + ((size_t)gz * Hg + gy) * Wg + gx);
        float* o = gs + c * DG_GS + (ez * DG_EY + ey) * DG_ROW + j;
        o[0] = v.x;
        o[DG_EXH] = v.y;
      }
    } else {
      for (int idx = tid; idx < DG_KC * DG_EZ * DG_EY * DG_ROW; idx += DG_THREADS) {
        const int e = idx % DG_ROW;
        const int rest = idx / DG_ROW;
        const int ey = rest % DG_EY, ez = (rest / DG_EY) % DG_EZ, c = rest / (DG_EY * DG_EZ);
        const int co = c0 + c, gz = gz0 + ez, gy = gy0 + ey, gx = gx0 + e;
        float v = 0.f;
        if (co < a.Co && gz >= 0 && gz < Dg && gy >= 0 && gy < Hg && gx >= 0 && gx < Wg)
          v = a.g[((size_t)b * a.Co + co) * gplane + ((size_t)gz * Hg + gy) * Wg + gx];
        gs[c * DG_GS + (ez * DG_EY + ey) * DG_ROW + (e & 1) * DG_EXH + (e >> 1)] = v;
      }
    }
    __syncthreads();

    const float* bc = brd + (size_t)c0 * a.cip;
#pragma unroll 1
    for (int tz = 0; tz < 4; ++tz) {
#pragma unroll
      for (int ty = 0; ty < 4; ++ty)
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) {
          // g column 2q-1+tx = halo column 2q+1+tx: phase (1+tx) & 1, index q + ((1+tx) >> 1)
          const int off = (tz * DG_EY + ty) * DG_ROW + ((1 + tx) & 1) * DG_EXH + ((1 + tx) >> 1);
          const float a0 = ard[off], a1 = ard[off + 4 * DG_ROW];
          const float* bt = bc + (size_t)((tz * 4 + ty) * 4 + tx) * a.cop * a.cip;
#pragma unroll
          for (int n = 0; n < NT; ++n) {
            const float bv = bt[n * 16];
            acc[0][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bv, acc[0][n], 0, 0, 0);
            acc[1][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bv, acc[1][n], 0, 0, 0);
          }
        }
    }
  }

  // D layout: col = lane & 15 (ci), row = 4 * (lane >> 4) + r (position: tile row (lane >> 4) >> 1, columns 4 * (lk & 1) + r)
  const int iz = oz0 + pz, ix = ox0 + 4 * (lk & 1);
  if (iz >= a.D || ix >= a.W) return;
  const size_t xplane = (size_t)a.D * a.H * a.W;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int iy = oy0 + ybase + 2 * m + (lk >> 1);
    if (iy >= a.H) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int ci = n0 + n * 16 + li;
      if (ci >= a.Ci) continue;
      float* o = a.dx + ((size_t)b * a.Ci + ci) * xplane + ((size_t)iz * a.H + iy) * a.W + ix;
      if (VEC) {
        *reinterpret_cast<float4*>(o) = make_float4(acc[m][n][0], acc[m][n][1], acc[m][n][2], acc[m][n][3]);
      } else {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          if (ix + rr < a.W) o[rr] = acc[m][n][rr];
      }
    }
  }
}

template <int NT>
int launch_dgrad(const DgArgs& a, dim3 grid, bool vec, hipStream_t s) {
  if (vec)
    hipLaunchKernelGGL((deconv3d_k4_dgrad_kernel<NT, true>), grid, dim3(DG_THREADS), 0, s, a);
  else
    hipLaunchKernelGGL((deconv3d_k4_dgrad_kernel<NT, false>), grid, dim3(DG_THREADS), 0, s, a);
  return dv_launch_status();
}

// ------------------------------------------------------------------------------------------------ weight gradient
constexpr int WG_TZ = 2, WG_TY = 4, WG_TX = 8, WG_P = WG_TZ * WG_TY * WG_TX;
constexpr int WG_EY = 2 * (WG_TY - 1) + 4, WG_EXH = WG_TX + 1, WG_ROW = 2 * WG_EXH;
constexpr int WG_TARGET_WAVES = 2048;                    // two waves per SIMD on 256 CUs, whatever the block size
constexpr int WG_XS = dv_pad_2mod32(WG_P);                          // per-channel stride of the x tile
constexpr int WG_HS = dv_pad_2mod32(WG_TZ * WG_EY * WG_ROW);        // per-channel stride of the g halo (one tz)
static_assert(WG_TX % 4 == 0, "an MFMA step takes 4 positions along W");

struct WgArgs {
  const float* x;     // [B, Ci, D, H, W]
  const float* g;     // [B, Co, 2D, 2H, 2W]
  float* ws;          // [splits, Ci, Co, 64]
  int B, Ci, D, H, W, Co;
  int nbz, nby, nbx;
  long long nbricks;
  int splits;
};

template <int MW, int NW, int KW>
__global__ __launch_bounds__(64 * MW * NW * KW) void deconv3d_k4_wgrad_kernel(WgArgs a) {
  constexpr int THREADS = 64 * MW * NW * KW, MC = 16 * MW, NC = 16 * NW;
  __shared__ float smem[MC * WG_XS + NC * WG_HS];
  static_assert(KW == 1 || MW * NW * 16 * 256 <= MC * WG_XS + NC * WG_HS, "the K waves' accumulators pass through the tiles");
  static_assert((WG_TZ * WG_TY) % KW == 0, "brick rows per K wave");
  float* xs = smem;
  float* hs = smem + MC * WG_XS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cw = wave % (MW * NW), kw = wave / (MW * NW);      // channel tile of the wave, and its share of the brick's rows
  const int mw = cw % MW, nw = cw / MW;
  const int li = lane & 15, lk = lane >> 4;
  const int tz = blockIdx.x & 3;
  const int ci0 = (blockIdx.x >> 2) * MC, co0 = blockIdx.y * NC, split = blockIdx.z;
  const int Dg = 2 * a.D, Hg = 2 * a.H, Wg = 2 * a.W;

  f32x4 acc[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const size_t xplane = (size_t)a.D * a.H * a.W, gplane = (size_t)Dg * Hg * Wg;
  const float* xrd = xs + (mw * 16 + li) * WG_XS;
  const float* hrd = hs + (nw * 16 + li) * WG_HS;

  for (long long br = b0; br < b1; ++br) {
    int b, bz, by, bx;
    dv_brick_decode3(br, a.nbz, a.nby, a.nbx, b, bz, by, bx);
    const int oz0 = bz * WG_TZ, oy0 = by * WG_TY, ox0 = bx * WG_TX;

    __syncthreads();                                      // the previous brick's reads are done
    // x tile: [MC ci][TZ][TY][TX]
    for (int idx = tid; idx < MC * WG_P; idx += THREADS) {
      const int c = idx / WG_P, p = idx % WG_P;
      const int px = p % WG_TX, py = (p / WG_TX) % WG_TY, pz = p / (WG_TX * WG_TY);
      const int ci = ci0 + c, iz = oz0 + pz, iy = oy0 + py, ix = ox0 + px;
      float v = 0.f;
      if (ci < a.Ci && iz < a.D && iy < a.H && ix < a.W)
        v = a.x[((size_t)b * a.Ci + ci) * xplane + ((size_t)iz * a.H + iy) * a.W + ix];
      xs[c * WG_XS + p] = v;
    }
    // g halo of this tz: [NC co][TZ][EY][EX], rows phase-split
    for (int idx = tid; idx < NC * WG_TZ * WG_EY * WG_ROW; idx += THREADS) {
      const int ex = idx % WG_ROW;
      const int rest = idx / WG_ROW;
      const int ey = rest % WG_EY, pz = (rest / WG_EY) % WG_TZ, c = rest / (WG_EY * WG_TZ);
      const int co = co0 + c, gz = 2 * (oz0 + pz) - 1 + tz, gy = 2 * oy0 - 1 + ey, gx = 2 * ox0 - 1 + ex;
      float v = 0.f;
      if (co < a.Co && gz >= 0 && gz < Dg && gy >= 0 && gy < Hg && gx >= 0 && gx < Wg)
        v = a.g[((size_t)b * a.Co + co) * gplane + ((size_t)gz * Hg + gy) * Wg + gx];
      hs[c * WG_HS + (pz * WG_EY + ey) * WG_ROW + (ex & 1) * WG_EXH + (ex >> 1)] = v;
    }
    __syncthreads();

#pragma unroll 1
    for (int row = kw; row < WG_TZ * WG_TY; row += KW) {  // the brick's (z, y) rows, dealt to the K waves
      const int pz = row / WG_TY, py = row % WG_TY;
#pragma unroll
      for (int sx = 0; sx < WG_TX / 4; ++sx) {
        const int q = sx * 4 + lk;                        // x column inside the brick
        const float av = xrd[row * WG_TX + q];
#pragma unroll
        for (int ty = 0; ty < 4; ++ty)
#pragma unroll
          for (int tx = 0; tx < 4; ++tx) {
            // g column 2q-1+tx = halo column 2q+tx: phase tx & 1, index q + (tx >> 1)
            const float bv = hrd[(pz * WG_EY + 2 * py + ty) * WG_ROW + (tx & 1) * WG_EXH + q + (tx >> 1)];
            acc[ty * 4 + tx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[ty * 4 + tx], 0, 0, 0);
          }
      }
    }
  }

  // K waves 1 .. KW-1 hand their accumulators to K wave 0 through LDS, one after the other: a fixed order
  if (KW > 1) {
    float* pass = smem + cw * 16 * 256 + lane;
#pragma unroll 1
    for (int k = 1; k < KW; ++k) {
      __syncthreads();                                    // the tiles (k = 1) or the previous pass have been read
      if (kw == k) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) pass[(t * 4 + rr) * 64] = acc[t][rr];
      }
      __syncthreads();
      if (kw == 0) {
#pragma unroll
        for (int t = 0; t < 16; ++t)
#pragma unroll
          for (int rr = 0; rr < 4; ++rr) acc[t][rr] += pass[(t * 4 + rr) * 64];
      }
    }
    if (kw != 0) return;
  }

  // D layout: col = lane & 15 (co), row = 4 * (lane >> 4) + r (ci)
  const int co = co0 + nw * 16 + li;
  if (co >= a.Co) return;
  float* out = a.ws + (size_t)split * a.Ci * a.Co * 64;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int ci = ci0 + mw * 16 + 4 * lk + rr;
    if (ci >= a.Ci) continue;
    float* o = out + ((size_t)ci * a.Co + co) * 64 + tz * 16;
#pragma unroll
    for (int t = 0; t < 16; ++t) o[t] = acc[t][rr];
  }
}

struct WgPlan {
  int mw, nw, kw, mtiles, ntiles, nbz, nby, nbx, splits;
  long long nbricks;
};

WgPlan wg_plan(int B, int Ci, int D, int H, int W, int Co) {
  WgPlan p;
  const int nm = (Ci + 15) / 16, nn = (Co + 15) / 16;
  p.mw = nm % 3 == 0 ? 3 : (nm >= 2 ? 2 : 1);
  p.nw = nn >= 2 ? 2 : 1;
  p.kw = p.mw * p.nw >= 4 ? 1 : 4 / (p.mw * p.nw);        // narrow channel tiles: the block's other waves split the brick
  p.mtiles = (nm + p.mw - 1) / p.mw;
  p.ntiles = (nn + p.nw - 1) / p.nw;
  p.nbz = (D + WG_TZ - 1) / WG_TZ;
  p.nby = (H + WG_TY - 1) / WG_TY;
  p.nbx = (W + WG_TX - 1) / WG_TX;
  p.nbricks = (long long)B * p.nbz * p.nby * p.nbx;
  // split K so that the grid's waves fill the device twice over, within the workspace bound
  const long long mn = 4ll * p.mtiles * p.ntiles * p.mw * p.nw * p.kw;
  p.splits = dv_wgrad_splits((WG_TARGET_WAVES + mn - 1) / mn, (long long)Ci * Co * 64, p.nbricks, 1, false);
  return p;
}

template <int MW, int NW>
void launch_wgrad_kernel(const WgArgs& a, dim3 grid, hipStream_t s) {
  constexpr int KW = MW * NW >= 4 ? 1 : 4 / (MW * NW);
  hipLaunchKernelGGL((deconv3d_k4_wgrad_kernel<MW, NW, KW>), grid, dim3(64 * MW * NW * KW), 0, s, a);
}

}  // namespace

extern "C" size_t dv_deconv3d_k4s2_dgrad_packed_floats(int Ci, int Co) {
  if (Ci <= 0 || Co <= 0) return 0;
  const DgGeo q = dg_geo(Ci, Co);
  return (size_t)64 * q.cop * q.cip;
}

extern "C" int dv_deconv3d_k4s2_dgrad_pack_weights_f32(const float* w, float* wpacked, int Ci, int Co,
                                                       dv_stream_t stream) {
  DV_REQUIRE_PTR(w);
  DV_REQUIRE_PTR(wpacked);
  DV_REQUIRE(Ci > 0 && Co > 0, DV_ERR_SHAPE);
  const DgGeo q = dg_geo(Ci, Co);
  const long long n = 64ll * q.cop * q.cip;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(dgrad_pack_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, (hipStream_t)stream, w,
                     wpacked, Ci, Co, q.cop, q.cip);
  return dv_launch_status();
}

extern "C" int dv_deconv3d_k4s2_dgrad_f32(const float* g, const float* wpacked, float* dx, int B, int Ci, int D, int H,
                                          int W, int Co, dv_stream_t stream) {
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(wpacked);
  DV_REQUIRE_PTR(dx);
  DV_REQUIRE(valid_shape(B, Ci, D, H, W, Co), DV_ERR_SHAPE);
  const DgGeo q = dg_geo(Ci, Co);
  DgArgs a;
  a.g = g; a.wp = wpacked; a.dx = dx;
  a.B = B; a.Ci = Ci; a.D = D; a.H = H; a.W = W; a.Co = Co; a.cop = q.cop; a.cip = q.cip;
  a.nbz = (D + DG_TZ - 1) / DG_TZ; a.nby = (H + DG_TY - 1) / DG_TY; a.nbx = (W + DG_TX - 1) / DG_TX;
  const long long bricks = (long long)B * a.nbz * a.nby * a.nbx;
  DV_REQUIRE(bricks <= 0x7fffffffll && q.groups <= 65535, DV_ERR_SHAPE);
  const bool vec = W % 4 == 0 && dv_aligned16(g) && dv_aligned16(dx);
  const dim3 grid((unsigned)bricks, (unsigned)q.groups);
  hipStream_t s = (hipStream_t)stream;
  if (q.nt == 1) return launch_dgrad<1>(a, grid, vec, s);
  if (q.nt == 2) return launch_dgrad<2>(a, grid, vec, s);
  return launch_dgrad<3>(a, grid, vec, s);
}

extern "C" size_t dv_deconv3d_k4s2_wgrad_workspace_floats(int B, int Ci, int D, int H, int W, int Co) {
  if (!valid_shape(B, Ci, D, H, W, Co)) return 0;
  return (size_t)wg_plan(B, Ci, D, H, W, Co).splits * Ci * Co * 64;
}

extern "C" int dv_deconv3d_k4s2_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Ci,
                                          int D, int H, int W, int Co, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(valid_shape(B, Ci, D, H, W, Co), DV_ERR_SHAPE);
  const WgPlan p = wg_plan(B, Ci, D, H, W, Co);
  DV_REQUIRE(4ll * p.mtiles <= 0x7fffffffll && p.ntiles <= 65535 && p.splits <= 65535, DV_ERR_SHAPE);
  WgArgs a;
  a.x = x; a.g = g; a.ws = workspace;
  a.B = B; a.Ci = Ci; a.D = D; a.H = H; a.W = W; a.Co = Co;
  a.nbz = p.nbz; a.nby = p.nby; a.nbx = p.nbx; a.nbricks = p.nbricks; a.splits = p.splits;
  const dim3 grid((unsigned)(4 * p.mtiles), (unsigned)p.ntiles, (unsigned)p.splits);
  hipStream_t s = (hipStream_t)stream;
  if (p.mw == 3 && p.nw == 2) launch_wgrad_kernel<3, 2>(a, grid, s);
  else if (p.mw == 3) launch_wgrad_kernel<3, 1>(a, grid, s);
  else if (p.mw == 2 && p.nw == 2) launch_wgrad_kernel<2, 2>(a, grid, s);
  else if (p.mw == 2) launch_wgrad_kernel<2, 1>(a, grid, s);
  else if (p.nw == 2) launch_wgrad_kernel<1, 2>(a, grid, s);
  else launch_wgrad_kernel<1, 1>(a, grid, s);
  return dv_splitk_finish(workspace, dw, (long long)Ci * Co * 64, p.splits, s, false);
}
