// Weight gradient of the 3x3x3 stride-1 aggregation convolutions in mixed-precision training, written once for the two
// 16-bit element types of csrc/mp_elem.h (train precisions "f16" and "bf16"):
//   dW[co, ci, tz, ty, tx] = sum_{b, z, y, x} r(g[b, co, z, y, x]) * r(X[b, ci, z + tz - 1, y + ty - 1, x + tx - 1]),
//   X zero outside the volume, r = T::round: r16 at MpF16 (round to nearest even fp16, subnormals kept, beyond 65504:
//   Inf), rb16 at MpBf16 (round to nearest even bfloat16 by the hardware conversion while the operand is staged; NaN
//   stays NaN; a finite float32 above about 3.3895e38 rounds to Inf; operands below 2^-126 may be flushed to zero).
// Both operands are float32 tensors, rounded while they are staged; the products (exact in fp32 unless they leave the
// fp32 exponent range) accumulate in fp32 on T::mfma (v_mfma_f32_16x16x32_f16 / _bf16); dW is written as UNROUNDED
// float32.  This header holds the kernel, the staging, the plan and the launch helper; csrc/conv3d_wgrad_f16.hip and
// csrc/conv3d_wgrad_bf16.hip each hold one instantiation and its extern "C" entries.  The scheme is
// csrc/conv3d_wgrad.hip's through
// wgrad_splitk.h (a block owns 32 co x 32 ci x 27 taps and walks a contiguous range of output bricks, each wave one
// 16 x 16 quarter with 27 accumulators; every split writes its partial into the caller's workspace and a second launch
// sums the splits in split order: no atomics, the bits depend on the shape only); the LDS image and the operand
// fragments are csrc/conv2d_wgrad_cat_f16.hip's.  "Half" below is one 16-bit element of either type.
//
// GEMM view: M = 16 output channels, N = 16 input channels of one tap, K = the 32 output positions of one (z, y) row of
// a brick of 2 x 2 x 32 positions.  Lane (li = lane & 15, lk = lane >> 4) supplies the 8 positions 8 lk .. 8 lk + 7 of
// channel li.  LDS: channel-major 16-bit, the positions of a row contiguous.  g: 4 rows of 32 halves per channel, the A
// fragment ONE aligned ds_read_b128, reused by the 27 taps.  x: ONE haloed copy, 4 x 4 rows of 40 halves per channel with
// interior column 0 at half 8 (16-byte aligned), the left halo at half 7 and the right halo at half 40; the B fragment of
// tap tx = 1 is the aligned b128, tx = 0 and tx = 2 are that b128 shifted by one half, built in registers from it and the
// dword before / after it.  Bank map: per-channel strides of 2 * odd 16-byte slots (656 halves = 82 slots for x, 144 = 18
// for g) keep the b128 reads conflict-free; the two b32 reads are 4-way conflicted (as in the 2-D kernel).
// Staging: a 32-lane half-wave loads one row of 32 floats (one channel per pass: 16 rows per channel make the
// (channel, row) of a pass shifts and masks); even lanes take their right neighbour's value through a DPP quad permute
// and store two halves as one dword.  Two blocks per CU overlap one block's staging with the other's MFMAs.
//
// Non-finite values: the positions of a brick outside the volume are staged as g = 0 (and x = 0) and multiplied like any
// other, so an Inf of x next to the far edge of a volume that is no multiple of the brick meets a 0 of g: NaN in the
// rows of dW of that input channel where the exact sum has none.  An Inf of g stays in the rows of its output channel.
#pragma once
#include "mp_elem.h"
#include "wgrad_splitk.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int HG_CO = 32, HG_CI = 32, HG_THREADS = 256;
constexpr int HG_TZ = 2, HG_TY = 2, HG_TX = 32;          // output brick: TZ * TY MFMA K steps of 32 positions
constexpr int HG_EZ = HG_TZ + 2, HG_EY = HG_TY + 2;      // x rows with halo
constexpr int HG_HR = HG_EZ * HG_EY;                     // 16 staged x rows per channel
constexpr int HG_GR = HG_TZ * HG_TY;                     // 4 staged g rows per channel
constexpr int HG_RS = 40;                                // halves per staged x row: [.. 7 = left halo | 8..39 | 40 = right halo]
constexpr int HG_X0 = 8;                                 // half of interior column 0 in its row
constexpr int HG_XS = HG_HR * HG_RS + 16;                // 656: the last row's right halo lies inside the stride
constexpr int HG_GS = HG_GR * HG_TX + 16;                // 144
constexpr int HG_KT = 27;
constexpr int HG_TARGET_BLOCKS = 512;                    // two blocks per CU on 256 CUs
static_assert(HG_HR == 16 && HG_GR == 4 && HG_EY == 4, "the staging maps (channel, row) with shifts");
static_assert((HG_XS / 8) % 4 == 2 && (HG_GS / 8) % 4 == 2 && HG_XS % 8 == 0 && HG_GS % 8 == 0, "strides of 2 * odd slots");
static_assert((HG_CI * HG_XS + 8 + HG_CO * HG_GS) * 2 <= 64 * 1024, "static LDS, two blocks per CU");

struct HgArgs {
  const float* x;     // [B, Cin, D, H, W]
  const float* g;     // [B, Cout, D, H, W]
  float* ws;          // [splits, Cout, Cin, 27]
  int B, Cin, D, H, W, Cout;
  int nbz, nby, nbx, splits;
  long long nbricks;
};

// own | right neighbour << 16 (meaningful in even lanes): the neighbour through a DPP quad permute [1, 0, 3, 2]
template <class T>
__device__ __forceinline__ unsigned hg_pair(float v) {
  const unsigned own = mp_bits<T>(v);                              // round to nearest even; beyond the range: Inf
  const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, false);
  return own | (other << 16);
}

__device__ __forceinline__ unsigned hg_align(unsigned lo, unsigned hi) { return (lo >> 16) | (hi << 16); }

// brick `br` from global memory into the LDS images (zeros outside the volume / the channels)
template <class T>
__device__ __forceinline__ void hg_stage(const HgArgs& a, long long br, int co0, int ci0, int tid, typename T::elem* xs,
                                         typename T::elem* gs) {
  int b, bz, by, bx;
  dv_brick_decode3(br, a.nbz, a.nby, a.nbx, b, bz, by, bx);
  const int oz0 = bz * HG_TZ, oy0 = by * HG_TY, ox0 = bx * HG_TX;
  const size_t vol = (size_t)a.D * a.H * a.W;
  const int col = tid & 31, rw = tid >> 5;
  const int ix = ox0 + col;
  const float* xb = a.x + (size_t)b * a.Cin * vol;
  const float* gb = a.g + (size_t)b * a.Cout * vol;

  // x interior: pass p covers row (p & 1) * 8 + rw of channel p >> 1; the two offsets serve every channel
  bool xin[2];
  unsigned xoff[2];                                      // (D*H*W < 2^30: checked by the entry)
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int r = h * 8 + rw, iz = oz0 - 1 + (r >> 2), iy = oy0 - 1 + (r & 3);
    xin[h] = iz >= 0 && iz < a.D && iy >= 0 && iy < a.H && ix < a.W;
    xoff[h] = xin[h] ? (unsigned)((iz * a.H + iy) * a.W + ix) : 0u;
  }
  constexpr int BATCH = 8;                               // channels whose loads are in flight together
#pragma unroll 1
  for (int cb = 0; cb < HG_CI; cb += BATCH) {
    float v[BATCH][2];
#pragma unroll
    for (int c = 0; c < BATCH; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ci = ci0 + cb + c;
        v[c][h] = (xin[h] && ci < a.Cin) ? xb[(size_t)ci * vol + xoff[h]] : 0.f;
      }
#pragma unroll
    for (int c = 0; c < BATCH; ++c)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const unsigned pr = hg_pair<T>(v[c][h]);            // (every lane: the permute reads the odd lanes)
        if ((col & 1) == 0)
          *reinterpret_cast<unsigned*>(xs + (cb + c) * HG_XS + (h * 8 + rw) * HG_RS + HG_X0 + col) = pr;
      }
  }
  // x halo columns: item i = channel row i >> 1, side i & 1 (column ox0 - 1 / ox0 + TX)
  {
    constexpr int NE = HG_CI * HG_HR * 2 / HG_THREADS;
    float e[NE];
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int i = tid + j * HG_THREADS, row = i >> 1, c = row >> 4, r = row & 15;
      const int iz = oz0 - 1 + (r >> 2), iy = oy0 - 1 + (r & 3), hx = (i & 1) ? ox0 + HG_TX : ox0 - 1, ci = ci0 + c;
      const bool in = iz >= 0 && iz < a.D && iy >= 0 && iy < a.H && hx >= 0 && hx < a.W && ci < a.Cin;
      e[j] = in ? xb[(size_t)ci * vol + (unsigned)((iz * a.H + iy) * a.W + hx)] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const int i = tid + j * HG_THREADS, row = i >> 1, c = row >> 4, r = row & 15;
      xs[c * HG_XS + r * HG_RS + ((i & 1) ? HG_X0 + HG_TX : HG_X0 - 1)] = T::round(e[j]);
    }
  }
  // g: pass p covers row rw & 3 of channel 2 p + (rw >> 2)
  {
    const int r = rw & 3, oz = oz0 + (r >> 1), oy = oy0 + (r & 1);
    const bool in = oz < a.D && oy < a.H && ix < a.W;
    const unsigned off = in ? (unsigned)((oz * a.H + oy) * a.W + ix) : 0u;
    constexpr int NG = HG_CO * HG_GR / 8;
    float v[NG];
#pragma unroll
    for (int p = 0; p < NG; ++p) {
      const int co = co0 + 2 * p + (rw >> 2);
      v[p] = (in && co < a.Cout) ? gb[(size_t)co * vol + off] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < NG; ++p) {
      const unsigned pr = hg_pair<T>(v[p]);
      if ((col & 1) == 0) *reinterpret_cast<unsigned*>(gs + (2 * p + (rw >> 2)) * HG_GS + r * HG_TX + col) = pr;
    }
  }
}

template <class T>
__global__ __launch_bounds__(HG_THREADS, 2) void conv3d_wgrad_mp_kernel(HgArgs a) {
  typedef typename T::elem elem;
  typedef typename T::v8 h8;
  __shared__ __attribute__((aligned(16))) elem xs[HG_CI * HG_XS + 8];
  __shared__ __attribute__((aligned(16))) elem gs[HG_CO * HG_GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * HG_CO, ci0 = blockIdx.y * HG_CI, split = blockIdx.z;
  const int coh = wave & 1, cih = wave >> 1;             // the wave's 16 co x 16 ci quarter
  const int li = lane & 15, lk = lane >> 4;

  f32x4 acc[HG_KT];
#pragma unroll
  for (int t = 0; t < HG_KT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const elem* xrd = xs + (cih * 16 + li) * HG_XS + 8 * lk;
  const elem* grd = gs + (coh * 16 + li) * HG_GS + 8 * lk;

  for (long long br = b0; br < b1; ++br) {
    __syncthreads();                                     // the previous brick's reads are done
    hg_stage<T>(a, br, co0, ci0, tid, xs, gs);
    __syncthreads();

#pragma unroll 1                                         // (unrolled, the compiler hoists 36 fragments' reads and spills)
    for (int pr = 0; pr < HG_GR; ++pr) {
      const int pz = pr >> 1, py = pr & 1;
      const h8 av = *reinterpret_cast<const h8*>(grd + pr * HG_TX);
#pragma unroll
      for (int tz = 0; tz < 3; ++tz)
#pragma unroll
        for (int ty = 0; ty < 3; ++ty) {
          const elem* p = xrd + ((pz + tz) * HG_EY + (py + ty)) * HG_RS;
          const u32x4 d = *reinterpret_cast<const u32x4*>(p + HG_X0);
          const unsigned before = *reinterpret_cast<const unsigned*>(p + HG_X0 - 2);
          const unsigned after = *reinterpret_cast<const unsigned*>(p + HG_X0 + 8);
          const unsigned s1 = hg_align(d[0], d[1]), s2 = hg_align(d[1], d[2]), s3 = hg_align(d[2], d[3]);
          const h8 x0 = __builtin_bit_cast(h8, (u32x4{hg_align(before, d[0]), s1, s2, s3}));
          const h8 x1 = __builtin_bit_cast(h8, d);
          const h8 x2 = __builtin_bit_cast(h8, (u32x4{s1, s2, s3, hg_align(d[3], after)}));
          const int t = (tz * 3 + ty) * 3;
          acc[t] = T::mfma(av, x0, acc[t]);
          acc[t + 1] = T::mfma(av, x1, acc[t + 1]);
          acc[t + 2] = T::mfma(av, x2, acc[t + 2]);
        }
    }
  }

  dv_wgrad_store_tile<HG_KT>(a.ws, split, acc, co0 + coh * 16, ci0 + cih * 16, a.Cout, a.Cin, li, lk);
}

struct HgPlan {
  int nbz, nby, nbx, splits;
  long long nbricks;
};

HgPlan hg_plan(int B, int Cin, int D, int H, int W, int Cout) {
  HgPlan p;
  p.nbz = (D + HG_TZ - 1) / HG_TZ;
  p.nby = (H + HG_TY - 1) / HG_TY;
  p.nbx = (W + HG_TX - 1) / HG_TX;
  p.nbricks = (long long)B * p.nbz * p.nby * p.nbx;
  // split K so that the grid fills the device twice over, within the workspace bound
  const long long mn = (long long)((Cout + HG_CO - 1) / HG_CO) * ((Cin + HG_CI - 1) / HG_CI);
  p.splits = dv_wgrad_splits((HG_TARGET_BLOCKS + mn - 1) / mn, (long long)Cout * Cin * HG_KT, p.nbricks, 1, false);
  return p;
}

bool hg_valid(int B, int Cin, int D, int H, int W, int Cout) {
  return B > 0 && Cin > 0 && D > 0 && H > 0 && W > 0 && Cout > 0 && (long long)D * H * W < (1ll << 30) &&
         (long long)Cout * Cin * HG_KT <= DV_WGRAD_MAX_WS_FLOATS && (Cout + HG_CO - 1) / HG_CO <= 65535 &&
         (Cin + HG_CI - 1) / HG_CI <= 65535;
}

// the two entries of a table: the size (the plan does not depend on the element type) and the checks and the launch
inline size_t conv3d_wgrad_mp_workspace_floats(int B, int Cin, int D, int H, int W, int Cout) {
  if (!hg_valid(B, Cin, D, H, W, Cout)) return 0;
  return (size_t)hg_plan(B, Cin, D, H, W, Cout).splits * Cout * Cin * HG_KT;
}

template <class T>
int conv3d_wgrad_mp_launch(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D, int H, int W,
                           int Cout, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(hg_valid(B, Cin, D, H, W, Cout), DV_ERR_SHAPE);
  const HgPlan p = hg_plan(B, Cin, D, H, W, Cout);
  HgArgs a;
  a.x = x; a.g = g; a.ws = workspace;
  a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout;
  a.nbz = p.nbz; a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  hipStream_t s = (hipStream_t)stream;
  dim3 grid((unsigned)((Cout + HG_CO - 1) / HG_CO), (unsigned)((Cin + HG_CI - 1) / HG_CI), (unsigned)p.splits);
  hipLaunchKernelGGL(conv3d_wgrad_mp_kernel<T>, grid, dim3(HG_THREADS), 0, s, a);
  return dv_splitk_finish(workspace, dw, (long long)Cout * Cin * HG_KT, p.splits, s, false);
}

}  // namespace
