// Weight gradient of the dilated 2-D convolutions of the KITTI12 refinement network (training: the backward of
// `convbn` / BasicBlock / conv8 inside refinenet_version3, KITTI12/models/pwcnet_ddim.py:251-306, submodule.py:21-24,
// :192-215):
//   dW[co, ci, ky, kx] = sum_{b, y, x} g[b, co, y, x] * x[b, ci, y + (ky-1)*d, x + (kx-1)*d],
//   k in {1, 3}, stride 1, padding = dilation d (1..16); x is zero outside the image.
// An implicit GEMM M = Cout, N = Cin*k^2, K = B*H*W on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
//
// A block owns 32 output channels x 32 input channels x all k^2 taps and walks a contiguous range of output bricks
// (TY x TX positions of one batch item).  Per brick it stages in LDS the g tile [32 co][TY][TX] and, per tap row ky, one
// band of x: rows y0 + (ky-1)d .. y0 + (ky-1)d + TY-1 and columns x0 - d .. x0 + TX-1 + d, so the dilation is gathered
// while staging (option (a) of the design note in DESIGN.md: rows of whole cache lines, no de-interleave pass).  Zeros
// are stored outside the image (the padding) and for channels past Cout / Cin.  Each wave -- one (16 co, 16 ci) quarter
// of the block's tile -- then runs k^2 accumulators over the brick: one MFMA step takes 4 consecutive output positions
// along W, its A operand (g) is read once and reused by every tap, the tap (ky, kx) reads band ky at column offset kx*d.
// The K dimension is split over blocks; every split writes its partial [Cout][Cin][k^2] into the caller's workspace
// and a second kernel sums the splits in split order.  No atomics: the bits do not depend on the launch.
//
// LDS bank map (ds_read_b32: bank = dword % 32, conflicts inside a 32-lane half): lane l reads channel l & 15 at output
// position l >> 4 (two positions per half); per-channel strides are 2 mod 32 and the two positions are adjacent dwords
// (the tap offset kx*d is the same for every lane): conflict-free for every dilation.
#include "wgrad_splitk.h"

namespace {

constexpr int WG_CO = 32, WG_CI = 32, WG_THREADS = 256;
constexpr int WG_TARGET_BLOCKS = 512;                    // two blocks per CU on 256 CUs
constexpr int WG_MAX_DILATION = 16;

// KS: kernel size; TY x TX: output brick; DMAX: largest dilation the x bands have room for
template <int KS_, int TY_, int TX_, int DMAX_>
struct WgGeo {
  static constexpr int KS = KS_, TY = TY_, TX = TX_, DMAX = DMAX_;
  static constexpr int KT = KS * KS;
  static constexpr int P = TY * TX;
  static constexpr int ROW = TX + (KS - 1) * DMAX;        // floats per staged band row
  static constexpr int XS = dv_pad_2mod32(KS * TY * ROW);    // per-channel stride of the x bands
  static constexpr int GS = dv_pad_2mod32(P);                // per-channel stride of the g tile
  static_assert(TX % 4 == 0, "an MFMA step takes 4 positions along W");
  static_assert((WG_CI * XS + WG_CO * GS) * 4 <= 80 * 1024, "two blocks per CU");
};

// k = 3, dilation 1..4: 4 x 32 output bricks (three bands of 4 x 40)
using GeoK3D4 = WgGeo<3, 4, 32, 4>;
// k = 3, dilation 5..16: 2 x 32 output bricks (three bands of 2 x 64)
using GeoK3D16 = WgGeo<3, 2, 32, WG_MAX_DILATION>;
// k = 1: 4 x 32
using GeoK1 = WgGeo<1, 4, 32, 0>;

struct WgArgs {
  const float* x;     // [B, Cin, H, W]
  const float* g;     // [B, Cout, H, W]
  float* ws;          // [splits, Cout, Cin, KT]
  int B, Cin, H, W, Cout, d;
  int nby, nbx;
  long long nbricks;
  int splits;
};

template <class G>
__global__ __launch_bounds__(WG_THREADS, 2) void conv2d_wgrad_kernel(WgArgs a) {
  __shared__ float xs[WG_CI * G::XS];
  __shared__ float gs[WG_CO * G::GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * WG_CO, ci0 = blockIdx.y * WG_CI, split = blockIdx.z;
  const int coh = wave & 1, cih = wave >> 1;
  const int li = lane & 15, lk = lane >> 4;
  const int d = G::KS == 1 ? 0 : a.d;                    // tap spacing (k = 1 has one tap at offset 0)
  const int ex_n = G::TX + (G::KS - 1) * d;              // staged columns of a band row

  f32x4 acc[G::KT];
#pragma unroll
  for (int t = 0; t < G::KT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const size_t plane = (size_t)a.H * a.W;
  const float* xrd = xs + (cih * 16 + li) * G::XS;
  const float* grd = gs + (coh * 16 + li) * G::GS;

  for (long long br = b0; br < b1; ++br) {
    int b, by, bx;
    dv_brick_decode2(br, a.nby, a.nbx, b, by, bx);
    const int oy0 = by * G::TY, ox0 = bx * G::TX;

    __syncthreads();                                      // the previous brick's reads are done
    // g tile: [32 co][TY][TX]
    for (int idx = tid; idx < WG_CO * G::P; idx += WG_THREADS) {
      const int c = idx / G::P, p = idx % G::P;
      const int co = co0 + c, oy = oy0 + p / G::TX, ox = ox0 + p % G::TX;
      float v = 0.f;
      if (co < a.Cout && oy < a.H && ox < a.W) v = a.g[((size_t)b * a.Cout + co) * plane + (size_t)oy * a.W + ox];
      gs[c * G::GS + p] = v;
    }
    // x bands: [32 ci][KS][TY][ex_n] (row stride ROW), band ky starts at row oy0 + (ky-1)d, column ox0 - d
    const int nrow = WG_CI * G::KS * G::TY;
    for (int idx = tid; idx < nrow * ex_n; idx += WG_THREADS) {
      const int ex = idx % ex_n, rw = idx / ex_n;
      const int py = rw % G::TY, ky = (rw / G::TY) % G::KS, c = rw / (G::TY * G::KS);
      const int ci = ci0 + c, iy = oy0 + py + (ky - (G::KS - 1) / 2) * d, ix = ox0 + ex - ((G::KS - 1) / 2) * d;
      float v = 0.f;
      if (ci < a.Cin && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
        v = a.x[((size_t)b * a.Cin + ci) * plane + (size_t)iy * a.W + ix];
      xs[c * G::XS + (ky * G::TY + py) * G::ROW + ex] = v;
    }
    __syncthreads();

#pragma unroll 1
    for (int py = 0; py < G::TY; ++py) {
#pragma unroll
      for (int sx = 0; sx < G::TX / 4; ++sx) {
        const int q = sx * 4 + lk;                        // output column inside the brick
        const float av = grd[py * G::TX + q];
#pragma unroll
        for (int ky = 0; ky < G::KS; ++ky) {
          const float* row = xrd + (ky * G::TY + py) * G::ROW + q;
#pragma unroll
          for (int kx = 0; kx < G::KS; ++kx) {
            const float bv = row[kx * d];
            acc[ky * G::KS + kx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[ky * G::KS + kx], 0, 0, 0);
          }
        }
      }
    }
  }

  dv_wgrad_store_tile<G::KT>(a.ws, split, acc, co0 + coh * 16, ci0 + cih * 16, a.Cout, a.Cin, li, lk);
}

struct WgPlan {
  int nby, nbx, splits;
  long long nbricks;
};

template <class G>
WgPlan plan_of(int B, int Cin, int H, int W, int Cout) {
  WgPlan p;
  p.nby = (H + G::TY - 1) / G::TY;
  p.nbx = (W + G::TX - 1) / G::TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  // split K so that the grid fills the device twice over, within the workspace bound
  const long long mn = (long long)((Cout + WG_CO - 1) / WG_CO) * ((Cin + WG_CI - 1) / WG_CI);
  p.splits = dv_wgrad_splits((WG_TARGET_BLOCKS + mn - 1) / mn, (long long)Cout * Cin * G::KT, p.nbricks, 1, false);
  return p;
}

bool valid_shape(int B, int Cin, int H, int W, int Cout) {
  return B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0;
}

bool valid_conv(int k, int dilation) {
  return (k == 1 || k == 3) && dilation >= 1 && dilation <= WG_MAX_DILATION;
}

template <class G>
int launch_wgrad(const float* x, const float* g, float* dw, float* ws, int B, int Cin, int H, int W, int Cout, int d,
                 hipStream_t s) {
  const WgPlan p = plan_of<G>(B, Cin, H, W, Cout);
  WgArgs a;
  a.x = x; a.g = g; a.ws = ws;
  a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.d = d;
  a.nby = p.nby; a.nbx = p.nbx; a.nbricks = p.nbricks; a.splits = p.splits;
  dim3 grid((unsigned)((Cout + WG_CO - 1) / WG_CO), (unsigned)((Cin + WG_CI - 1) / WG_CI), (unsigned)p.splits);
  hipLaunchKernelGGL(conv2d_wgrad_kernel<G>, grid, dim3(WG_THREADS), 0, s, a);
  return dv_splitk_finish(ws, dw, (long long)Cout * Cin * G::KT, p.splits, s, false);
}

}  // namespace

extern "C" size_t dv_conv2d_wgrad_workspace_floats(int B, int Cin, int H, int W, int Cout, int k, int dilation) {
  if (!valid_shape(B, Cin, H, W, Cout) || !valid_conv(k, dilation)) return 0;
  WgPlan p;
  if (k == 1) p = plan_of<GeoK1>(B, Cin, H, W, Cout);
  else if (dilation <= GeoK3D4::DMAX) p = plan_of<GeoK3D4>(B, Cin, H, W, Cout);
  else p = plan_of<GeoK3D16>(B, Cin, H, W, Cout);
  return (size_t)p.splits * Cout * Cin * k * k;
}

extern "C" int dv_conv2d_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int H,
                                   int W, int Cout, int k, int dilation, dv_stream_t stream) {
  DV_REQUIRE(valid_conv(k, dilation), DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(valid_shape(B, Cin, H, W, Cout), DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (k == 1) return launch_wgrad<GeoK1>(x, g, dw, workspace, B, Cin, H, W, Cout, 1, s);
  if (dilation <= GeoK3D4::DMAX) return launch_wgrad<GeoK3D4>(x, g, dw, workspace, B, Cin, H, W, Cout, dilation, s);
  return launch_wgrad<GeoK3D16>(x, g, dw, workspace, B, Cin, H, W, Cout, dilation, s);
}
