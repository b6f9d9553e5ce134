// Weight gradient of the 3-D aggregation convolutions (training: the backward of convbn_3d, SceneFlow/models/
// submodule.py:94-97, and of the hourglass ConvTranspose3d layers through the exchange of x and g):
//   dW[co, ci, t] = sum_{b, o} g[b, co, o] * x[b, ci, s*o + t - p],   cubic k in {1, 3}, p = (k-1)/2, s in {1, 2}.
// An implicit GEMM M = Cout, N = Cin*k^3, K = B*Do*Ho*Wo on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
//
// A block owns 32 output channels x 32 input channels x all k^3 taps and walks a contiguous range of output bricks
// (TZ x TY x TX output positions of one batch item): per brick it stages the g tile [32 co][brick] and the x tile with
// its halo [32 ci][EZ][EY][EX] in LDS (zeros outside the volume = the convolution's padding, and for channels past
// Cout / Cin), then each wave -- one (16 co, 16 ci) quarter of the block's tile -- runs k^3 accumulators over the brick:
// one MFMA step takes 4 consecutive output positions along W, its A operand (g) is read once and reused by every tap.
// The K dimension is split over blocks; every split writes its partial [Cout][Cin][k^3] into the caller's workspace and a
// second kernel sums the splits in split order.  No atomics: the bits do not depend on the launch.
//
// LDS bank map (ds_read_b32: bank = dword % 32, conflicts inside a 32-lane half): lane l reads channel l & 15 at output
// position k = l >> 4 (two positions per half), so per-channel strides are 2 mod 32 and the two positions are adjacent
// dwords: conflict-free.  For stride 2 the x rows are stored phase-split (even columns, then odd columns), so the
// positions 2o + tx of one MFMA step are adjacent there too.
#include "wgrad_splitk.h"

namespace {

constexpr int WG_CO = 32, WG_CI = 32, WG_THREADS = 256;
constexpr int WG_TARGET_BLOCKS = 512;                    // two blocks per CU on 256 CUs

template <int KS_, int S_, int TZ_, int TY_, int TX_>
struct WgGeo {
  static constexpr int KS = KS_, S = S_, TZ = TZ_, TY = TY_, TX = TX_;
  static constexpr int KT = KS * KS * KS;
  static constexpr int P = TZ * TY * TX;
  static constexpr int EZ = S * (TZ - 1) + KS, EY = S * (TY - 1) + KS, EX = S * (TX - 1) + KS;
  static constexpr int EXH = (EX + S - 1) / S;           // columns per phase
  static constexpr int ROW = S * EXH;                    // floats per staged (z, y) row
  static constexpr int XS = dv_pad_2mod32(EZ * EY * ROW);   // per-channel stride of the x tile
  static constexpr int GS = dv_pad_2mod32(P);               // per-channel stride of the g tile
  static_assert(TX % 4 == 0, "an MFMA step takes 4 positions along W");
  static_assert((WG_CI * XS + WG_CO * GS) * 4 <= 80 * 1024, "two blocks per CU");
};

// k = 3, stride 1: 2 x 4 x 16 output bricks (x tile 4 x 6 x 18)
using GeoK3S1 = WgGeo<3, 1, 2, 4, 16>;
// k = 3, stride 2: 2 x 2 x 8 output bricks (x tile 5 x 5 x 17, phase-split rows of 2 x 9)
using GeoK3S2 = WgGeo<3, 2, 2, 2, 8>;
// k = 1: 2 x 4 x 16
using GeoK1 = WgGeo<1, 1, 2, 4, 16>;

struct WgArgs {
  const float* x;     // [B, Cin, D, H, W]
  const float* g;     // [B, Cout, Do, Ho, Wo]
  float* ws;          // [splits, Cout, Cin, KT]
  int B, Cin, D, H, W, Cout, Do, Ho, Wo;
  int nbz, nby, nbx;
  long long nbricks;
  int splits;
};

template <class G>
__global__ __launch_bounds__(WG_THREADS, 2) void conv3d_wgrad_kernel(WgArgs a) {
  __shared__ float xs[WG_CI * G::XS];
  __shared__ float gs[WG_CO * G::GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * WG_CO, ci0 = blockIdx.y * WG_CI, split = blockIdx.z;
  const int coh = wave & 1, cih = wave >> 1;
  const int li = lane & 15, lk = lane >> 4;
  constexpr int PAD = (G::KS - 1) / 2;

  f32x4 acc[G::KT];
#pragma unroll
  for (int t = 0; t < G::KT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const size_t xplane = (size_t)a.D * a.H * a.W, gplane = (size_t)a.Do * a.Ho * a.Wo;
  const float* xrd = xs + (cih * 16 + li) * G::XS;
  const float* grd = gs + (coh * 16 + li) * G::GS;

  for (long long br = b0; br < b1; ++br) {
    int b, bz, by, bx;
    dv_brick_decode3(br, a.nbz, a.nby, a.nbx, b, bz, by, bx);
    const int oz0 = bz * G::TZ, oy0 = by * G::TY, ox0 = bx * G::TX;
    const int iz0 = oz0 * G::S - PAD, iy0 = oy0 * G::S - PAD, ix0 = ox0 * G::S - PAD;

    __syncthreads();                                      // the previous brick's reads are done
    // g tile: [32 co][TZ][TY][TX]
    for (int idx = tid; idx < WG_CO * G::P; idx += WG_THREADS) {
      const int c = idx / G::P, p = idx % G::P;
      const int px = p % G::TX, py = (p / G::TX) % G::TY, pz = p / (G::TX * G::TY);
      const int co = co0 + c, oz = oz0 + pz, oy = oy0 + py, ox = ox0 + px;
      float v = 0.f;
      if (co < a.Cout && oz < a.Do && oy < a.Ho && ox < a.Wo)
        v = a.g[((size_t)b * a.Cout + co) * gplane + ((size_t)oz * a.Ho + oy) * a.Wo + ox];
      gs[c * G::GS + p] = v;
    }
    // x tile with halo: [32 ci][EZ][EY][EX], rows phase-split for stride 2
    for (int idx = tid; idx < WG_CI * G::EZ * G::EY * G::EX; idx += WG_THREADS) {
      const int ex = idx % G::EX;
      const int rest = idx / G::EX;
      const int ey = rest % G::EY, ez = (rest / G::EY) % G::EZ, c = rest / (G::EY * G::EZ);
      const int ci = ci0 + c, iz = iz0 + ez, iy = iy0 + ey, ix = ix0 + ex;
      float v = 0.f;
      if (ci < a.Cin && iz >= 0 && iz < a.D && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = a.x[((size_t)b * a.Cin + ci) * xplane + ((size_t)iz * a.H + iy) * a.W + ix];
      const int col = G::S == 1 ? ex : (ex & 1) * G::EXH + (ex >> 1);
      xs[c * G::XS + (ez * G::EY + ey) * G::ROW + col] = v;
    }
    __syncthreads();

#pragma unroll 1
    for (int pz = 0; pz < G::TZ; ++pz) {
#pragma unroll 1
      for (int py = 0; py < G::TY; ++py) {
#pragma unroll
        for (int sx = 0; sx < G::TX / 4; ++sx) {
          const float av = grd[(pz * G::TY + py) * G::TX + sx * 4 + lk];
          const int q = sx * 4 + lk;                      // output column inside the brick
#pragma unroll
          for (int tz = 0; tz < G::KS; ++tz)
#pragma unroll
            for (int ty = 0; ty < G::KS; ++ty)
#pragma unroll
              for (int tx = 0; tx < G::KS; ++tx) {
                const int row = (G::S * pz + tz) * G::EY + (G::S * py + ty);
                // column S*q + tx of the halo row; phase-split: phase tx & 1, index q + (tx >> 1)
                const int col = G::S == 1 ? q + tx : (tx & 1) * G::EXH + q + (tx >> 1);
                const float bv = xrd[row * G::ROW + col];
                const int t = (tz * G::KS + ty) * G::KS + tx;
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t], 0, 0, 0);
              }
        }
      }
    }
  }

  dv_wgrad_store_tile<G::KT>(a.ws, split, acc, co0 + coh * 16, ci0 + cih * 16, a.Cout, a.Cin, li, lk);
}

struct WgPlan {
  int Do, Ho, Wo, nbz, nby, nbx, splits;
  long long nbricks;
};

template <class G>
WgPlan plan_of(int B, int Cin, int D, int H, int W, int Cout) {
  WgPlan p;
  const int pad = (G::KS - 1) / 2;
  p.Do = (D + 2 * pad - G::KS) / G::S + 1;
  p.Ho = (H + 2 * pad - G::KS) / G::S + 1;
  p.Wo = (W + 2 * pad - G::KS) / G::S + 1;
  p.nbz = (p.Do + G::TZ - 1) / G::TZ;
  p.nby = (p.Ho + G::TY - 1) / G::TY;
  p.nbx = (p.Wo + G::TX - 1) / G::TX;
  p.nbricks = (long long)B * p.nbz * p.nby * p.nbx;
  // split K so that the grid fills the device twice over, within the workspace bound
  const long long mn = (long long)((Cout + WG_CO - 1) / WG_CO) * ((Cin + WG_CI - 1) / WG_CI);
  p.splits = dv_wgrad_splits((WG_TARGET_BLOCKS + mn - 1) / mn, (long long)Cout * Cin * G::KT, p.nbricks, 1, false);
  return p;
}

bool valid_shape(int B, int Cin, int D, int H, int W, int Cout) {
  return B > 0 && Cin > 0 && D > 0 && H > 0 && W > 0 && Cout > 0;
}

template <class G>
int launch_wgrad(const float* x, const float* g, float* dw, float* ws, int B, int Cin, int D, int H, int W, int Cout,
                 hipStream_t s) {
  const WgPlan p = plan_of<G>(B, Cin, D, H, W, Cout);
  WgArgs a;
  a.x = x; a.g = g; a.ws = ws;
  a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout; a.Do = p.Do; a.Ho = p.Ho; a.Wo = p.Wo;
  a.nbz = p.nbz; a.nby = p.nby; a.nbx = p.nbx; a.nbricks = p.nbricks; a.splits = p.splits;
  dim3 grid((unsigned)((Cout + WG_CO - 1) / WG_CO), (unsigned)((Cin + WG_CI - 1) / WG_CI), (unsigned)p.splits);
  hipLaunchKernelGGL(conv3d_wgrad_kernel<G>, grid, dim3(WG_THREADS), 0, s, a);
  return dv_splitk_finish(ws, dw, (long long)Cout * Cin * G::KT, p.splits, s, false);
}

}  // namespace

extern "C" size_t dv_conv3d_wgrad_workspace_floats(int B, int Cin, int D, int H, int W, int Cout, int k, int stride) {
  if (!valid_shape(B, Cin, D, H, W, Cout)) return 0;
  WgPlan p;
  if (k == 3 && stride == 1) p = plan_of<GeoK3S1>(B, Cin, D, H, W, Cout);
  else if (k == 3 && stride == 2) p = plan_of<GeoK3S2>(B, Cin, D, H, W, Cout);
  else if (k == 1 && stride == 1) p = plan_of<GeoK1>(B, Cin, D, H, W, Cout);
  else return 0;
  return (size_t)p.splits * Cout * Cin * k * k * k;
}

extern "C" int dv_conv3d_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D,
                                   int H, int W, int Cout, int k, int stride, dv_stream_t stream) {
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(stride == 1 || stride == 2, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(!(k == 1 && stride != 1), DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(valid_shape(B, Cin, D, H, W, Cout), DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (k == 3 && stride == 1) return launch_wgrad<GeoK3S1>(x, g, dw, workspace, B, Cin, D, H, W, Cout, s);
  if (k == 3) return launch_wgrad<GeoK3S2>(x, g, dw, workspace, B, Cin, D, H, W, Cout, s);
  return launch_wgrad<GeoK1>(x, g, dw, workspace, B, Cin, D, H, W, Cout, s);
}
