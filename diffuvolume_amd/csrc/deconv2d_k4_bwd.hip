// Weight gradient of nn.ConvTranspose2d(4, stride 2, padding 1): IGEV's `spx_2_gru.conv1` (32 -> 32, BasicConv deconv,
// KITTI15/core/submodule.py:9-35, :36-76) and `spx_gru` (64 -> 9, igev_stereo_ddim.py:110-112), which the reference's train
// loop differentiates at every GRU iteration (`upsample_disp`, igev_stereo_ddim.py:203-211, :441-457).
// w [Ci][Co][4][4], x [B,Ci,H,W], g = d loss / d out [B,Co,2H,2W], zero outside the image:
//   dw[ci,co,ky,kx] = sum_{b,i,j} x[b,ci,i,j] * g[b,co,2i-1+ky,2j-1+kx]
// (The input gradient needs no kernel of its own: it is a 3x3 convolution of the pixel-unshuffled g with the flipped parity
// weights of Deconv2dK4S2Plan, on the forward kernels.)
//
// An implicit GEMM on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32 with M = the 16 taps of ONE output channel,
// N = 16 input channels, K = input pixels: every row of every M tile is a real tap, whatever Co is (a (co, ci) tiling of
// `spx_gru` would idle 7 of 16 rows, the 3x3 parity form of the forward 20 of 36 taps).  The A operand of a step is the
// stride-2 gather itself: lane (tap = 4 ty + tx, pixel q) reads g halo element (2 py + ty, 2 q + tx) from LDS.
//   * a wave owns one output channel and NT (1..4) N tiles: NT MFMAs per 1 + NT LDS reads;
//   * a block is 1..4 waves (one output channel each: the launcher takes 3 for Co = 9 or 3, else up to 4) that share the
//     x tile [NT*16 ci][4 x 16 pixels] and stage their own channel's g halo [10][34];
//   * the staging is double-buffered through registers with fixed per-thread shares (element tid + it * threads of the
//     tile, compile-time trip counts): the global loads of brick n+1 are all issued before the MFMAs of brick n and
//     stored to LDS after them;
//   * the K dimension (bricks of 4 x 16 input pixels, all batch items in one sequence) is split over blocks; each split
//     writes its partial [Ci][Co][16] into the caller's workspace, a second kernel adds the splits: four quarters of
//     the split range in split order each, then the quarters in order.
// Summation order of one dw element: one fma chain over the pixels of the split's bricks, then the splits as above.
// No atomics: the bits depend on the shape only.  Pixels of a brick outside the image are staged as x = 0 (and g = 0).
// LDS bank map (ds_read_b32, conflicts inside a 32-lane half): A -- the halo row stride is 8 mod 32, the columns
// tx + 2 q of a half span 6 dwords, equal addresses broadcast: conflict-free; B -- lane reads channel l & 15 at pixel
// l >> 4, channel stride 2 mod 32: conflict-free.
// Registers (hipcc -O3 -fno-slp-vectorize, gfx950): <NT 2, 4 waves> (32 -> 32) 84 VGPR, 14.8 KB LDS; <NT 4, 3 waves>
// (64 -> 9) 149 VGPR, 21.7 KB LDS; no instantiation spills (<4, 1> takes all 256).
#include "wgrad_splitk.h"

namespace {

constexpr int D2_TY = 4, D2_TX = 16, D2_P = D2_TY * D2_TX;       // brick of input pixels
constexpr int D2_EY = 2 * D2_TY + 2, D2_EX = 2 * D2_TX + 2;      // g rows 2*oy0-1 .. 2*oy0+2*TY, columns alike
constexpr int D2_ROW = 40;                                       // halo row stride
constexpr int D2_HS = D2_EY * D2_ROW;                            // per-channel stride of the halo
constexpr int D2_XS = D2_P + 2;                                  // per-channel stride of the x tile
constexpr int D2_MAX_CO = 4, D2_MAX_NT = 4;
constexpr int D2_TARGET_BLOCKS = 1024;                           // four blocks per CU on 256 CUs
static_assert(D2_ROW >= D2_EX && D2_ROW % 32 == 8 && D2_XS % 32 == 2, "bank maps");
static_assert(D2_TX % 4 == 0, "an MFMA step takes 4 pixels along W");

struct D2Args {
  const float* x;     // [B, Ci, H, W]
  const float* g;     // [B, Co, 2H, 2W]
  float* ws;          // [splits, Ci, Co, 16]
  int B, Ci, H, W, Co;
  int nby, nbx, splits;
  long long nbricks;
};

// The calling thread's share of a brick: x tile [NT*16 ci][TY x TX] and the g halos [COB co][EY][EX], element idx =
// tid + it * THREADS of each.  Loaded into registers one brick ahead (the loads of brick n+1 are issued before the
// MFMAs of brick n and stored to LDS after them), all loads of a brick in flight together.
template <int NT, int COB>
struct D2Regs {
  static constexpr int THREADS = 64 * COB;
  static constexpr int NXE = NT * 16 * D2_P, NGE = COB * D2_EY * D2_EX;
  static constexpr int NX = (NXE + THREADS - 1) / THREADS, NG = (NGE + THREADS - 1) / THREADS;
  float x[NX];
  float g[NG];
};

template <int NT, int COB>
__device__ __forceinline__ void d2_load(const D2Args& a, long long br, int co0, int ci0, int tid, D2Regs<NT, COB>& r) {
  using R = D2Regs<NT, COB>;
  int b, by, bx;
  dv_brick_decode2(br, a.nby, a.nbx, b, by, bx);
  const int oy0 = by * D2_TY, ox0 = bx * D2_TX;
  const int Hg = 2 * a.H, Wg = 2 * a.W;
  const size_t xplane = (size_t)a.H * a.W, gplane = (size_t)Hg * Wg;
#pragma unroll
  for (int it = 0; it < R::NX; ++it) {
    const int idx = tid + it * R::THREADS;
    const int c = idx / D2_P, p = idx % D2_P;
    const int ci = ci0 + c, iy = oy0 + p / D2_TX, ix = ox0 + p % D2_TX;
    float v = 0.f;
    if (idx < R::NXE && ci < a.Ci && iy < a.H && ix < a.W) v = a.x[((size_t)b * a.Ci + ci) * xplane + (size_t)iy * a.W + ix];
    r.x[it] = v;
  }
#pragma unroll
  for (int it = 0; it < R::NG; ++it) {
    const int idx = tid + it * R::THREADS;
    const int ex = idx % D2_EX, ey = (idx / D2_EX) % D2_EY, c = idx / (D2_EX * D2_EY);
    const int co = co0 + c, gy = 2 * oy0 - 1 + ey, gx = 2 * ox0 - 1 + ex;
    float v = 0.f;
    if (idx < R::NGE && co < a.Co && gy >= 0 && gy < Hg && gx >= 0 && gx < Wg)
      v = a.g[((size_t)b * a.Co + co) * gplane + (size_t)gy * Wg + gx];
    r.g[it] = v;
  }
}

template <int NT, int COB>
__device__ __forceinline__ void d2_store(float* xs, float* hs, int tid, const D2Regs<NT, COB>& r) {
  using R = D2Regs<NT, COB>;
#pragma unroll
  for (int it = 0; it < R::NX; ++it) {
    const int idx = tid + it * R::THREADS;
    if (idx < R::NXE) xs[(idx / D2_P) * D2_XS + idx % D2_P] = r.x[it];
  }
#pragma unroll
  for (int it = 0; it < R::NG; ++it) {
    const int idx = tid + it * R::THREADS;
    if (idx < R::NGE) hs[(idx / (D2_EX * D2_EY)) * D2_HS + ((idx / D2_EX) % D2_EY) * D2_ROW + idx % D2_EX] = r.g[it];
  }
}

template <int NT, int COB>
__global__ __launch_bounds__(64 * COB) void deconv2d_k4_wgrad_kernel(D2Args a) {
  __shared__ float xs[NT * 16 * D2_XS];
  __shared__ float hs[COB * D2_HS];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int co0 = blockIdx.x * COB, ci0 = blockIdx.y * NT * 16, split = blockIdx.z;

  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const float* ard = hs + wave * D2_HS + (li >> 2) * D2_ROW + (li & 3) + 2 * lk;     // tap (ty, tx) = (li >> 2, li & 3)
  const float* brd = xs + li * D2_XS + lk;

  D2Regs<NT, COB> regs;
  if (b0 < b1) d2_load<NT, COB>(a, b0, co0, ci0, tid, regs);
  for (long long br = b0; br < b1; ++br) {
    __syncthreads();                                      // the previous brick's reads are done
    d2_store<NT, COB>(xs, hs, tid, regs);
    __syncthreads();
    if (br + 1 < b1) d2_load<NT, COB>(a, br + 1, co0, ci0, tid, regs);      // in flight during the MFMAs below

#pragma unroll
    for (int py = 0; py < D2_TY; ++py) {
#pragma unroll
      for (int sx = 0; sx < D2_TX / 4; ++sx) {
        // pixel (py, q = 4 sx + lk): g element (2 py + ty, 2 q + tx) of the halo
        const float av = ard[2 * py * D2_ROW + 8 * sx];
#pragma unroll
        for (int n = 0; n < NT; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, brd[n * 16 * D2_XS + py * D2_TX + 4 * sx], acc[n], 0, 0, 0);
      }
    }
  }

  // D layout: col = lane & 15 (ci), row = 4 * (lane >> 4) + r (tap: ty = lane >> 4, tx = r)
  const int co = co0 + wave;
  if (co >= a.Co) return;
  float* out = a.ws + (size_t)split * a.Ci * a.Co * 16;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int ci = ci0 + n * 16 + li;
    if (ci >= a.Ci) continue;
    float* o = out + ((size_t)ci * a.Co + co) * 16 + 4 * lk;
    *reinterpret_cast<float4*>(o) = make_float4(acc[n][0], acc[n][1], acc[n][2], acc[n][3]);
  }
}

struct D2Plan {
  int cob, nt, coblocks, cigroups, nby, nbx, splits;
  long long nbricks;
};

bool d2_valid(int B, int Ci, int H, int W, int Co) {
  return B > 0 && Ci > 0 && H > 0 && W > 0 && Co > 0 && (long long)H * W < (1ll << 28) &&
         (long long)Ci * Co * 16 <= DV_WGRAD_MAX_WS_FLOATS;
}

D2Plan d2_plan(int B, int Ci, int H, int W, int Co) {
  D2Plan p;
  // output channels per block: the count in 4, 3 that wastes the fewest waves (9 -> 3 x 3, 32 -> 8 x 4), small layers whole
  p.cob = Co < D2_MAX_CO ? Co : ((Co + 2) / 3 * 3 < (Co + 3) / 4 * 4 ? 3 : 4);
  const int ntiles = (Ci + 15) / 16;
  p.nt = ntiles < D2_MAX_NT ? ntiles : D2_MAX_NT;
  p.coblocks = (Co + p.cob - 1) / p.cob;
  p.cigroups = (ntiles + p.nt - 1) / p.nt;
  p.nby = (H + D2_TY - 1) / D2_TY;
  p.nbx = (W + D2_TX - 1) / D2_TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  const long long mn = (long long)p.coblocks * p.cigroups;
  // at least two bricks per split
  p.splits = dv_wgrad_splits((D2_TARGET_BLOCKS + mn - 1) / mn, (long long)Ci * Co * 16, p.nbricks, 2, true);
  return p;
}

template <int NT>
void d2_launch_nt(int cob, dim3 grid, hipStream_t s, const D2Args& a) {
  switch (cob) {
    case 1: hipLaunchKernelGGL((deconv2d_k4_wgrad_kernel<NT, 1>), grid, dim3(64), 0, s, a); break;
    case 2: hipLaunchKernelGGL((deconv2d_k4_wgrad_kernel<NT, 2>), grid, dim3(128), 0, s, a); break;
    case 3: hipLaunchKernelGGL((deconv2d_k4_wgrad_kernel<NT, 3>), grid, dim3(192), 0, s, a); break;
    default: hipLaunchKernelGGL((deconv2d_k4_wgrad_kernel<NT, 4>), grid, dim3(256), 0, s, a); break;
  }
}

void d2_launch(int nt, int cob, dim3 grid, hipStream_t s, const D2Args& a) {
  switch (nt) {
    case 1: d2_launch_nt<1>(cob, grid, s, a); break;
    case 2: d2_launch_nt<2>(cob, grid, s, a); break;
    case 3: d2_launch_nt<3>(cob, grid, s, a); break;
    default: d2_launch_nt<4>(cob, grid, s, a); break;
  }
}

}  // namespace

extern "C" size_t dv_deconv2d_k4s2_wgrad_workspace_floats(int B, int Ci, int H, int W, int Co) {
  if (!d2_valid(B, Ci, H, W, Co)) return 0;
  return (size_t)d2_plan(B, Ci, H, W, Co).splits * Ci * Co * 16;
}

extern "C" int dv_deconv2d_k4s2_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Ci,
                                          int H, int W, int Co, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(d2_valid(B, Ci, H, W, Co), DV_ERR_SHAPE);
  DV_REQUIRE(dv_aligned16(workspace), DV_ERR_ALIGN);
  const D2Plan p = d2_plan(B, Ci, H, W, Co);
  DV_REQUIRE(p.cigroups <= 65535, DV_ERR_SHAPE);
  D2Args a;
  a.x = x; a.g = g; a.ws = workspace;
  a.B = B; a.Ci = Ci; a.H = H; a.W = W; a.Co = Co;
  a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  const dim3 grid((unsigned)p.coblocks, (unsigned)p.cigroups, (unsigned)p.splits);
  hipStream_t s = (hipStream_t)stream;
  d2_launch(p.nt, p.cob, grid, s, a);
  return dv_splitk_finish(workspace, dw, (long long)Ci * Co * 16, p.splits, s, true);
}
