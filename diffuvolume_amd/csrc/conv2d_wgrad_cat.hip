// Weight gradient of the dilation-1 convolutions of IGEV's recurrent update block over a VIRTUAL channel concatenation
// (training: the backward of ConvGRU's convz / convr / convq, KITTI15/core/update.py:26-40, of BasicMotionEncoder,
// update.py:74-94, of DispHead.conv1, update.py:15-24, and of mask_feat_4, update.py:115-117):
//   dW[co, ci, ky, kx] = sum_{b, y, x} g[b, co, y, x] * X[b, ci, y + ky - p, x + kx - p],  X = cat(inputs, dim=1),
//   k in {1, 3}, p = (k-1)/2, stride 1, X zero outside the image; `inputs` as in dv_conv2d_cat_f32 (1..4 tensors).
// An implicit GEMM M = Cout, N = Cin*k^2, K = B*H*W on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
//
// Against csrc/conv2d_wgrad.hip (built for refinenet3's dilated layers, kept as it is):
//   * the block tile is 64 co x 64 ci: each of the four waves owns 32 x 32 (2 x 2 MFMA tiles x k^2 taps = 144 accumulator
//     registers for k = 3); a g fragment feeds 2 * k^2 MFMAs and an x fragment two;
//   * dilation 1 lets all three tap rows share ONE halo tile of x, (TY+2) x (TX+2) per channel, instead of three bands
//     (136 floats per channel and brick instead of 480);
//   * the staging is double-buffered through registers: the global loads of brick n+1 are issued before the MFMAs of
//     brick n and stored to LDS after them, so their latency is covered by the same block's arithmetic (one LDS buffer of
//     58 KB).  144 accumulators + 50 staging registers + the fragments of an unrolled brick do not fit 256 registers
//     (the compiler spilled 220-280 of them under __launch_bounds__(256, 2)), so a block has a CU to itself: one wave
//     per SIMD with the full 512-register file, 36 independent MFMAs per step keep the pipe busy without a second wave;
//   * every thread's share of a brick is fixed (compile-time LDS offsets, no division in the staging loop): per iteration
//     a 32-lane half-wave loads one image row of 32 floats (one 128-byte line when the plane allows it).
// The K dimension (bricks of TY x TX = 2 x 32 output positions, all batch items in one sequence) is split over blocks;
// each split writes its partial [Cout][Cin][k^2] into the caller's workspace, a second kernel sums the splits in split
// order.  No atomics: the bits depend on the shape only.  (The split plan counts the bricks of the whole batch, so a
// batch and its halves are NOT summed in the same order.)
// Non-finite values: the positions of a brick outside the image are staged as g = 0 (and x = 0) and multiplied like any
// other, so a NaN OR an Inf in x next to the bottom / right edge of a plane that is no multiple of the brick meets a
// 0 of g: 0 * Inf = NaN in dw where the exact sum has no such product (csrc/conv2d_wgrad.hip has the same property).
// It stays in the rows of dw that belong to that input channel.
//
// Also here, for the same training route: the weight gradient of the 7x7 single-input-channel convd1.  (The ConvGRU gate
// arithmetic of the route is in csrc/gru_gates.hip.)
//
// LDS bank map (ds_read_b32, conflicts inside a 32-lane half): lane l reads channel l & 15 at output position l >> 4;
// per-channel strides are 2 mod 32 and the two positions of a half are adjacent dwords: conflict-free for every tap.
#include "wgrad_splitk.h"

namespace {

constexpr int WC_CO = 64, WC_CI = 64, WC_THREADS = 256;
constexpr int WC_TY = 2, WC_TX = 32;                     // output brick
constexpr int WC_TARGET_BLOCKS = 256;                    // one block per CU on 256 CUs, one round

template <int KS_>
struct WcGeo {
  static constexpr int KS = KS_, KT = KS * KS, HALO = (KS - 1) / 2;
  static constexpr int HR = WC_TY + KS - 1, HC = WC_TX + KS - 1;        // halo tile of x per channel
  static constexpr int XS = dv_pad_2mod32(HR * HC);                     // per-channel stride of the x tile
  static constexpr int GS = dv_pad_2mod32(WC_TY * WC_TX);               // per-channel stride of the g tile
  static constexpr int NX = WC_CI * HR / 8;                             // interior loads per thread (8 rows per pass)
  static constexpr int NE = KS == 1 ? 0 : 2;                            // halo-column loads per thread
  static constexpr int NG = WC_CO * WC_TY / 8;                          // g loads per thread
  static_assert(8 % HR == 0, "a pass of 8 rows holds whole channels");
  static_assert(KS == 1 || WC_CI * HR == WC_THREADS, "one halo row per thread");
  static_assert((WC_CI * XS + WC_CO * GS) * 4 <= 64 * 1024, "static LDS");
};

template <class G>
struct WcRegs {
  float x[G::NX];
  float e[G::NE == 0 ? 1 : G::NE];
  float g[G::NG];
};

// the calling thread's share of brick `br`, from global memory into registers (zeros outside the image / the channels)
template <class G>
__device__ __forceinline__ void wc_load(const DvCatArgs& a, long long br, int co0, int ci0, int tid, WcRegs<G>& r) {
  int b, by, bx;
  dv_brick_decode2(br, a.nby, a.nbx, b, by, bx);
  const int oy0 = by * WC_TY, ox0 = bx * WC_TX;
  const size_t plane = (size_t)a.H * a.W;
  const int col = tid & 31, rw = tid >> 5;               // 8 rows of 32 columns per pass
  {
    const int hr = rw % G::HR, cb = __builtin_amdgcn_readfirstlane(rw / G::HR);
    const int iy = oy0 + hr - G::HALO, ix = ox0 + col;
    const bool in = iy >= 0 && iy < a.H && ix < a.W;
    const unsigned off = (unsigned)((in ? iy : 0) * a.W + (in ? ix : 0));     // (H*W < 2^30: checked by the entry)
#pragma unroll
    for (int j = 0; j < G::NX; ++j) {
      const int ci = ci0 + cb + j * (8 / G::HR);
      float v = 0.f;
      if (in && ci < a.Cin) v = dv_cat_plane(a, ci, b, plane)[off];
      r.x[j] = v;
    }
  }
  if constexpr (G::NE != 0) {                            // columns ox0 - 1 and ox0 + TX of halo row `tid`
    const int hr = tid % G::HR, c = tid / G::HR;
    const int iy = oy0 + hr - G::HALO, ci = ci0 + c;
    const bool rin = iy >= 0 && iy < a.H && ci < a.Cin;
    const float* p = dv_cat_plane(a, rin ? ci : 0, b, plane) + (size_t)(rin ? iy : 0) * a.W;
    r.e[0] = (rin && ox0 >= 1) ? p[ox0 - 1] : 0.f;
    r.e[G::NE - 1] = (rin && ox0 + WC_TX < a.W) ? p[ox0 + WC_TX] : 0.f;
  }
  {
    const int py = rw % WC_TY, cb = __builtin_amdgcn_readfirstlane(rw / WC_TY);
    const int oy = oy0 + py, ox = ox0 + col;
    const bool in = oy < a.H && ox < a.W;
    const unsigned off = (unsigned)((in ? oy : 0) * a.W + (in ? ox : 0));
#pragma unroll
    for (int j = 0; j < G::NG; ++j) {
      const int co = co0 + cb + j * (8 / WC_TY);
      float v = 0.f;
      if (in && co < a.Cout) v = (a.g + ((size_t)b * a.Cout + co) * plane)[off];
      r.g[j] = v;
    }
  }
}

template <class G>
__device__ __forceinline__ void wc_store(float* xs, float* gs, int tid, const WcRegs<G>& r) {
  const int col = tid & 31, rw = tid >> 5;
  {
    float* p = xs + (rw / G::HR) * G::XS + (rw % G::HR) * G::HC + G::HALO + col;
#pragma unroll
    for (int j = 0; j < G::NX; ++j) p[j * (8 / G::HR) * G::XS] = r.x[j];
  }
  if constexpr (G::NE != 0) {
    float* p = xs + (tid / G::HR) * G::XS + (tid % G::HR) * G::HC;
    p[0] = r.e[0];
    p[G::HC - 1] = r.e[G::NE - 1];
  }
  {
    float* p = gs + (rw / WC_TY) * G::GS + (rw % WC_TY) * WC_TX + col;
#pragma unroll
    for (int j = 0; j < G::NG; ++j) p[j * (8 / WC_TY) * G::GS] = r.g[j];
  }
}

template <class G>
__global__ __launch_bounds__(WC_THREADS, 1) void conv2d_wgrad_cat_kernel(DvCatArgs a) {
  __shared__ float xs[WC_CI * G::XS];
  __shared__ float gs[WC_CO * G::GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * WC_CO, ci0 = blockIdx.y * WC_CI, split = blockIdx.z;
  const int cow = wave & 1, ciw = wave >> 1;             // the wave's 32 co x 32 ci quarter
  const int li = lane & 15, lk = lane >> 4;

  f32x4 acc[4][G::KT];                                   // [2 co tiles x 2 ci tiles][taps]
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int t = 0; t < G::KT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const float* xrd = xs + (ciw * 32 + li) * G::XS + lk;
  const float* grd = gs + (cow * 32 + li) * G::GS + lk;

  WcRegs<G> regs;
  if (b0 < b1) wc_load<G>(a, b0, co0, ci0, tid, regs);
  for (long long br = b0; br < b1; ++br) {
    __syncthreads();                                     // the previous brick's reads are done
    wc_store<G>(xs, gs, tid, regs);
    __syncthreads();
    if (br + 1 < b1) wc_load<G>(a, br + 1, co0, ci0, tid, regs);     // in flight during the MFMAs below

#pragma unroll
    for (int py = 0; py < WC_TY; ++py) {
#pragma unroll
      for (int sx = 0; sx < WC_TX / 4; ++sx) {
        const int p = py * WC_TX + sx * 4;               // (+ lk: folded into grd / xrd)
        const float a0 = grd[p], a1 = grd[16 * G::GS + p];
#pragma unroll
        for (int ky = 0; ky < G::KS; ++ky) {
#pragma unroll
          for (int kx = 0; kx < G::KS; ++kx) {
            const int o = (py + ky) * G::HC + sx * 4 + kx;
            const float x0 = xrd[o], x1 = xrd[16 * G::XS + o];
            const int t = ky * G::KS + kx;
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, x0, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, x1, acc[1][t], 0, 0, 0);
            acc[2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, x0, acc[2][t], 0, 0, 0);
            acc[3][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, x1, acc[3][t], 0, 0, 0);
          }
        }
      }
    }
  }

#pragma unroll
  for (int m = 0; m < 4; ++m)
    dv_wgrad_store_tile<G::KT>(a.ws, split, acc[m], co0 + cow * 32 + (m >> 1) * 16, ci0 + ciw * 32 + (m & 1) * 16, a.Cout,
                               a.Cin, li, lk);
}

struct WcPlan {
  int nby, nbx, splits;
  long long nbricks;
};

WcPlan wc_plan(int B, int Cin, int H, int W, int Cout, int k) {
  WcPlan p;
  p.nby = (H + WC_TY - 1) / WC_TY;
  p.nbx = (W + WC_TX - 1) / WC_TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  // split K so that the grid fills the device once (a block has a CU to itself: a second, partial round would cost a
  // whole one), within the workspace bound, at least two bricks per split
  const long long mn = (long long)((Cout + WC_CO - 1) / WC_CO) * ((Cin + WC_CI - 1) / WC_CI);
  p.splits = dv_wgrad_splits(WC_TARGET_BLOCKS / mn, (long long)Cout * Cin * k * k, p.nbricks, 2, false);
  return p;
}

bool wc_valid(long long cin, int B, int H, int W, int Cout, int k) {
  return (k == 1 || k == 3) && cin > 0 && B > 0 && H > 0 && W > 0 && Cout > 0 && (long long)H * W < (1ll << 30) &&
         (long long)Cout * cin * k * k <= DV_WGRAD_MAX_WS_FLOATS;
}

template <class G>
int wc_launch(const DvCatArgs& a, float* dw, hipStream_t s) {
  dim3 grid((unsigned)((a.Cout + WC_CO - 1) / WC_CO), (unsigned)((a.Cin + WC_CI - 1) / WC_CI), (unsigned)a.splits);
  hipLaunchKernelGGL(conv2d_wgrad_cat_kernel<G>, grid, dim3(WC_THREADS), 0, s, a);
  return dv_splitk_finish(a.ws, dw, (long long)a.Cout * a.Cin * G::KT, a.splits, s, false);
}

// ---- weight gradient of a single-input-channel k x k convolution (BasicMotionEncoder.convd1, 7x7, update.py:78) -----
// dw[co, ky, kx] = sum_{b,y,x} g[b,co,y,x] * x[b,0,y+ky-p,x+kx-p].  One block per (co, ky): every thread adds its
// positions (a fixed stride) into k accumulators, then a fixed-order tree over the block.  No atomics.
template <int K>
__global__ __launch_bounds__(256) void conv2d_1in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                               float* __restrict__ dw, int B, int H, int W, int Cout) {
  __shared__ float red[K][256];
  const int co = blockIdx.x, ky = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)H * W, total = (size_t)B * plane;
  float acc[K];
#pragma unroll
  for (int kx = 0; kx < K; ++kx) acc[kx] = 0.f;
  for (size_t i = tid; i < total; i += 256) {
    const int b = (int)(i / plane), p = (int)(i % plane), y = p / W, xx = p % W;
    const int iy = y + ky - K / 2;
    if (iy < 0 || iy >= H) continue;
    const float gv = g[((size_t)b * Cout + co) * plane + p];
    const float* row = x + (size_t)b * plane + (size_t)iy * W;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = xx + kx - K / 2;
      if (ix >= 0 && ix < W) acc[kx] = fmaf(gv, row[ix], acc[kx]);
    }
  }
#pragma unroll
  for (int kx = 0; kx < K; ++kx) red[kx][tid] = acc[kx];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int kx = 0; kx < K; ++kx) red[kx][tid] += red[kx][tid + s];
    __syncthreads();
  }
  if (tid < K) dw[((size_t)co * K + ky) * K + tid] = red[tid][0];
}

}  // namespace

extern "C" size_t dv_conv2d_wgrad_cat_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout,
                                                       int k) {
  const long long cin = dv_cat_cin(channels, n_inputs);
  if (!wc_valid(cin, B, H, W, Cout, k)) return 0;
  const WcPlan p = wc_plan(B, (int)cin, H, W, Cout, k);
  return (size_t)p.splits * Cout * cin * k * k;
}

extern "C" int dv_conv2d_wgrad_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* g,
                                       float* dw, float* workspace, int B, int H, int W, int Cout, int k,
                                       dv_stream_t stream) {
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(inputs);
  DV_REQUIRE_PTR(channels);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(n_inputs >= 1 && n_inputs <= DV_CAT_MAX_INPUTS, DV_ERR_SHAPE);
  const long long cin = dv_cat_cin(channels, n_inputs);
  DV_REQUIRE(wc_valid(cin, B, H, W, Cout, k), DV_ERR_SHAPE);
  for (int i = 0; i < n_inputs; ++i) DV_REQUIRE_PTR(inputs[i]);
  const WcPlan p = wc_plan(B, (int)cin, H, W, Cout, k);
  DvCatArgs a;
  dv_cat_fill(a, inputs, channels, n_inputs, (int)cin);
  a.g = g; a.ws = workspace;
  a.B = B; a.H = H; a.W = W; a.Cout = Cout;
  a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  hipStream_t s = (hipStream_t)stream;
  return k == 1 ? wc_launch<WcGeo<1>>(a, dw, s) : wc_launch<WcGeo<3>>(a, dw, s);
}

extern "C" int dv_conv2d_1in_wgrad_f32(const float* x, const float* g, float* dw, int B, int H, int W, int Cout, int k,
                                       dv_stream_t stream) {
  DV_REQUIRE(k == 7, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE(B > 0 && H > 0 && W > 0 && Cout > 0 && Cout <= 65535 && (long long)H * W < (1ll << 30), DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(conv2d_1in_wgrad_kernel<7>, dim3((unsigned)Cout, 7), dim3(256), 0, s, x, g, dw, B, H, W, Cout);
  return dv_launch_status();
}
