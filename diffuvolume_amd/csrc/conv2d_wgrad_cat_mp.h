// Weight gradient of the convolutions of IGEV's recurrent update block in 16-bit mixed-precision training
// (KITTI15/core/update.py:26-142 run inside autocast, train_stereo.py:146-173), over the VIRTUAL channel concatenation of
// dv_conv2d_wgrad_cat_f32 and with its argument list, written once for the two element types of csrc/mp_elem.h (train
// precisions "f16" and "bf16"):
//   dW[co, ci, ky, kx] = sum_{b, y, x} r(g[b, co, y, x]) * r(X[b, ci, y + ky - p, x + kx - p]),  X = cat(inputs, dim=1),
//   k in {1, 3}, p = (k-1)/2, stride 1, X zero outside the image, r = T::round: r16 at MpF16 (round to nearest even
//   fp16, subnormals kept, beyond 65504: Inf), rb16 at MpBf16 (round to nearest even bfloat16 by the hardware conversion;
//   NaN stays NaN; a finite float32 above about 3.3895e38 rounds to Inf; operands below 2^-126 may be flushed to zero).
// Both operands are float32 tensors, rounded while they are staged (what autocast's casts do to the operands of the
// reference's convolution backward); products (exact in fp32 unless they leave the fp32 exponent range) accumulate in
// fp32 on T::mfma (v_mfma_f32_16x16x32_f16 / _bf16); dW is written as UNROUNDED float32.  (The reference's autocast rounds
// dW to 16 bits before casting it back to the float32 parameter; keeping the fp32 sum is a deliberate difference that can
// only lose less.)  At fp16 a g or x beyond the fp16 range becomes Inf and Inf / NaN appears in dW: the signal
// torch.amp.GradScaler skips a step on.  At bf16 the range is float32's: no scaler, no skipped step.
// This header holds the kernel, the staging, the plan, the checks and the launch; csrc/conv2d_wgrad_cat_f16.hip and
// csrc/conv2d_wgrad_cat_bf16.hip each hold one instantiation's extern "C" entries.  "Half" below is one 16-bit element of
// either type.
//
// GEMM view: M = 16 output channels, N = 16 input channels of one tap, K = 32 consecutive output positions of one image
// row.  A block owns 64 co x 64 ci x k^2 taps, each of the four waves 32 x 32 (2 x 2 MFMA tiles x k^2 taps = 144
// accumulator registers for k = 3), one block per CU as in the fp32 kernel; per brick of 4 rows x 32 columns a wave issues
// 4 * 36 MFMAs.
//
// LDS image: channel-major 16-bit, the positions of a row contiguous, so that the A fragment (8 consecutive positions of one
// output channel) is ONE aligned ds_read_b128.  The x tile keeps ONE haloed copy, (4 + k - 1) rows of 40 halves per
// channel with the interior column 0 at half 8 of its row (16-byte aligned), the left halo at half 7 and the right halo at
// half 40.  The B fragment of tap kx is the 8 halves from half 7 + kx of the lane's 8-column group: kx = 1 is the aligned
// b128 itself; kx = 0 and kx = 2 are that b128 shifted by one half, built in registers from it and the dword before / after
// it (one ds_read_b32 each, 4 v_alignbit per tap).  So the three kx taps of a row cost one b128 + two b32 reads instead of
// three unaligned 16-byte reads (which the LDS does not do) or three shifted copies (three times the stores).  Bank map:
// a 16-lane group of ds_read_b128 holds 8 channels of position group lk and the OTHER 8 channels of group lk + 1 (one
// 16-byte slot further), so a per-channel stride of 2 * odd slots puts the former on the even and the latter on the odd
// slots: 240 halves (30 slots; k = 1: 176) for x, 144 (18) for g, conflict-free (an odd number of slots, the usual
// padding, always leaves one 2-way slot).  The two ds_read_b32 are 4-way conflicted (the strides are whole 16-byte slots,
// so 16 channels x 2 groups fall on 8 banks) -- see DESIGN.md for what that costs and the alternatives.
// Staging: as in the fp32 kernel every thread's share of a brick is fixed and double-buffered through registers (global
// loads of brick n+1 issued before the MFMAs of brick n).  A 32-lane half-wave loads one image row of 32 floats; even lanes
// take their right neighbour's value through a DPP quad permute and store the two halves as one dword (ds_write_b32, 16
// consecutive dwords per row: conflict-free).
//
// K (bricks of 4 x 32 output positions, all batch items in one sequence) is split over blocks; each split writes its
// partial [Cout][Cin][k^2] into the caller's workspace, a second kernel sums the splits in split order.  No atomics: the
// bits depend on the shape only.  Workspace bound as the fp32 kernel's (48 MB).
// Non-finite values: the positions of a brick outside the image are staged as g = 0 (and x = 0) and multiplied like any
// other, so a NaN or an Inf in x (a value that rounds to Inf included) next to the bottom / right edge of a plane that
// is no multiple of the brick meets a 0 of g: 0 * Inf = NaN in dW where the exact sum has no such product, as in
// csrc/conv2d_wgrad_cat.hip.  It stays in the rows of dW that belong to that input channel; an Inf of g stays in the rows
// of its output channel.
// (The ConvGRU gate arithmetic of these routes, with the rounding points of conv2d_mp.h's epilogues, is in
// csrc/gru_gates.hip and csrc/gru_gates_bf16.hip.)
#pragma once
#include "mp_elem.h"
#include "wgrad_splitk.h"

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int HW_CO = 64, HW_CI = 64, HW_THREADS = 256;
constexpr int HW_TY = 4, HW_TX = 32;                     // output brick: TY MFMA K steps of 32 positions
constexpr int HW_RS = 40;                                // halves per staged x row: [.. 7 = left halo | 8..39 | 40 = right halo]
constexpr int HW_X0 = 8;                                 // half of interior column 0 in its row
constexpr int HW_TARGET_BLOCKS = 256;                    // one block per CU on 256 CUs, one round

template <int KS_>
struct HwGeo {
  static constexpr int KS = KS_, KT = KS * KS, HALO = (KS - 1) / 2;
  static constexpr int HR = HW_TY + KS - 1;                             // staged x rows per channel
  // per-channel strides (halves): 2 * odd 16-byte slots (bank map above).  k = 3: the rows fill the stride; the right halo
  // of a channel's last row lies in half 0 of the next channel, which nothing else uses (the tile has 8 halves of tail)
  static constexpr int XS = KS == 1 ? 176 : HR * HW_RS;
  static constexpr int GS = HW_TY * HW_TX + 16;
  static_assert(XS >= HR * HW_RS && (XS / 8) % 4 == 2 && (GS / 8) % 4 == 2, "strides of 2 * odd slots");
  static constexpr int NX = HW_CI * HR / 8;                             // interior loads per thread (8 rows per pass)
  static constexpr int PER = HR == 6 ? 3 : 1;                           // passes after which (row % HR) repeats
  static constexpr int CPP = 8 * PER / HR;                              // channels per PER passes
  static constexpr int NE = KS == 1 ? 0 : HW_CI * HR * 2 / HW_THREADS;  // halo loads per thread
  static constexpr int NG = HW_CO * HW_TY / 8;                          // g loads per thread
  static_assert(XS % 8 == 0 && GS % 8 == 0, "16-byte aligned channel bases");
  static_assert((8 * PER) % HR == 0 && NX % PER == 0 && HR % 2 == 0 && HW_TY % 2 == 0, "whole channels per period");
  static_assert(KS == 1 || HW_CI * HR * 2 == NE * HW_THREADS, "whole halo passes");
  static_assert((HW_CI * XS + 8 + HW_CO * GS) * 2 <= 64 * 1024, "static LDS");
};

template <class G>
struct HwRegs {
  float x[G::NX];
  float e[G::NE == 0 ? 1 : G::NE];
  float g[G::NG];
};

// the calling thread's share of brick `br`, from global memory into registers (zeros outside the image / the channels).
// Interior and g: pass j covers the rows 8 j + (tid >> 5) of the [channel][row] list, lane tid & 31 = column.  The two
// half-waves of a wave hold rows 2 w and 2 w + 1: the same channel for every pass (HR and TY are even), so the plane's
// base is a scalar; the (channel, row) pattern repeats every PER passes, PER offsets per thread serve all of them.
template <class G>
__device__ __forceinline__ void hw_load(const DvCatArgs& a, long long br, int co0, int ci0, int tid, HwRegs<G>& r) {
  int b, by, bx;
  dv_brick_decode2(br, a.nby, a.nbx, b, by, bx);
  const int oy0 = by * HW_TY, ox0 = bx * HW_TX;
  const size_t plane = (size_t)a.H * a.W;
  const int col = tid & 31, rw = tid >> 5;
  const int ix = ox0 + col;
#pragma unroll
  for (int t = 0; t < G::PER; ++t) {
    const int row = t * 8 + rw, c = __builtin_amdgcn_readfirstlane(row / G::HR), hr = row % G::HR;
    const int iy = oy0 + hr - G::HALO;
    const bool in = iy >= 0 && iy < a.H && ix < a.W;
    const unsigned off = (unsigned)((in ? iy : 0) * a.W + (in ? ix : 0));     // (H*W < 2^30: checked by the entry)
#pragma unroll
    for (int m = 0; m < G::NX / G::PER; ++m) {
      const int ci = ci0 + c + m * G::CPP;
      float v = 0.f;
      if (in && ci < a.Cin) v = dv_cat_plane(a, ci, b, plane)[off];
      r.x[m * G::PER + t] = v;
    }
  }
  if constexpr (G::NE != 0) {                            // item i: channel row i >> 1, side i & 1 (column ox0 - 1 / ox0 + TX)
#pragma unroll
    for (int j = 0; j < G::NE; ++j) {
      const int i = tid + j * HW_THREADS, row = i >> 1, c = row / G::HR, hr = row - c * G::HR;
      const int iy = oy0 + hr - G::HALO, ci = ci0 + c, hx = (i & 1) ? ox0 + HW_TX : ox0 - 1;
      float v = 0.f;
      if (iy >= 0 && iy < a.H && hx >= 0 && hx < a.W && ci < a.Cin)
        v = dv_cat_plane(a, ci, b, plane)[(unsigned)(iy * a.W + hx)];
      r.e[j] = v;
    }
  }
  {
    const int py = rw % HW_TY, cb = __builtin_amdgcn_readfirstlane(rw / HW_TY);
    const int oy = oy0 + py;
    const bool in = oy < a.H && ix < a.W;
    const unsigned off = (unsigned)((in ? oy : 0) * a.W + (in ? ix : 0));
#pragma unroll
    for (int j = 0; j < G::NG; ++j) {
      const int co = co0 + cb + j * (8 / HW_TY);
      float v = 0.f;
      if (in && co < a.Cout) v = (a.g + ((size_t)b * a.Cout + co) * plane)[off];
      r.g[j] = v;
    }
  }
}

// own | right neighbour << 16 (meaningful in even lanes): the neighbour through a DPP quad permute [1, 0, 3, 2]
template <class T>
__device__ __forceinline__ unsigned hw_pair(float v) {
  const unsigned own = mp_bits<T>(v);                    // round to nearest even; beyond the range: Inf
  const unsigned other = (unsigned)__builtin_amdgcn_update_dpp(0, (int)own, 0xB1, 0xF, 0xF, false);
  return own | (other << 16);
}

template <class T, class G>
__device__ __forceinline__ void hw_store(typename T::elem* xs, typename T::elem* gs, int tid, const HwRegs<G>& r) {
  typedef typename T::elem elem;
  const int col = tid & 31, rw = tid >> 5;
#pragma unroll
  for (int t = 0; t < G::PER; ++t) {
    const int row = t * 8 + rw;
    elem* p = xs + (row / G::HR) * G::XS + (row % G::HR) * HW_RS + HW_X0 + col;
#pragma unroll
    for (int m = 0; m < G::NX / G::PER; ++m) {
      const unsigned v = hw_pair<T>(r.x[m * G::PER + t]);   // (every lane: the permute reads the odd lanes)
      if ((col & 1) == 0) *reinterpret_cast<unsigned*>(p + m * G::CPP * G::XS) = v;
    }
  }
  if constexpr (G::NE != 0) {
#pragma unroll
    for (int j = 0; j < G::NE; ++j) {
      const int i = tid + j * HW_THREADS, row = i >> 1, c = row / G::HR, hr = row - c * G::HR;
      xs[c * G::XS + hr * HW_RS + ((i & 1) ? HW_X0 + HW_TX : HW_X0 - 1)] = T::round(r.e[j]);
    }
  }
  {
    elem* p = gs + (rw / HW_TY) * G::GS + (rw % HW_TY) * HW_TX + col;
#pragma unroll
    for (int j = 0; j < G::NG; ++j) {
      const unsigned v = hw_pair<T>(r.g[j]);
      if ((col & 1) == 0) *reinterpret_cast<unsigned*>(p + j * (8 / HW_TY) * G::GS) = v;
    }
  }
}

__device__ __forceinline__ unsigned hw_align(unsigned lo, unsigned hi) { return (lo >> 16) | (hi << 16); }

template <class T, class G>
__global__ __launch_bounds__(HW_THREADS, 1) void conv2d_wgrad_cat_mp_kernel(DvCatArgs a) {
  typedef typename T::elem elem;
  typedef typename T::v8 h8;
  __shared__ __attribute__((aligned(16))) elem xs[HW_CI * G::XS + 8];
  __shared__ __attribute__((aligned(16))) elem gs[HW_CO * G::GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * HW_CO, ci0 = blockIdx.y * HW_CI, split = blockIdx.z;
  const int cow = wave & 1, ciw = wave >> 1;             // the wave's 32 co x 32 ci quarter
  const int li = lane & 15, lk = lane >> 4;

  f32x4 acc[4][G::KT];                                   // [2 co tiles x 2 ci tiles][taps]
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int t = 0; t < G::KT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const elem* xrd = xs + (ciw * 32 + li) * G::XS + 8 * lk;
  const elem* grd = gs + (cow * 32 + li) * G::GS + 8 * lk;

  HwRegs<G> regs;
  if (b0 < b1) hw_load<G>(a, b0, co0, ci0, tid, regs);
  for (long long br = b0; br < b1; ++br) {
    __syncthreads();                                     // the previous brick's reads are done
    hw_store<T, G>(xs, gs, tid, regs);
    __syncthreads();
    if (br + 1 < b1) hw_load<G>(a, br + 1, co0, ci0, tid, regs);     // in flight during the MFMAs below

#pragma unroll
    for (int py = 0; py < HW_TY; ++py) {
      const h8 a0 = *reinterpret_cast<const h8*>(grd + py * HW_TX);
      const h8 a1 = *reinterpret_cast<const h8*>(grd + 16 * G::GS + py * HW_TX);
#pragma unroll
      for (int ky = 0; ky < G::KS; ++ky) {
        h8 xf[2][G::KS];
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const elem* p = xrd + n * 16 * G::XS + (py + ky) * HW_RS;
          const u32x4 d = *reinterpret_cast<const u32x4*>(p + HW_X0);
          if constexpr (G::KS == 1) {
            xf[n][0] = __builtin_bit_cast(h8, d);
          } else {
            const unsigned before = *reinterpret_cast<const unsigned*>(p + HW_X0 - 2);
            const unsigned after = *reinterpret_cast<const unsigned*>(p + HW_X0 + 8);
            const unsigned s1 = hw_align(d[0], d[1]), s2 = hw_align(d[1], d[2]), s3 = hw_align(d[2], d[3]);
            xf[n][0] = __builtin_bit_cast(h8, (u32x4{hw_align(before, d[0]), s1, s2, s3}));
            xf[n][1] = __builtin_bit_cast(h8, d);
            xf[n][2] = __builtin_bit_cast(h8, (u32x4{s1, s2, s3, hw_align(d[3], after)}));
          }
        }
#pragma unroll
        for (int kx = 0; kx < G::KS; ++kx) {
          const int t = ky * G::KS + kx;
          acc[0][t] = T::mfma(a0, xf[0][kx], acc[0][t]);
          acc[1][t] = T::mfma(a0, xf[1][kx], acc[1][t]);
          acc[2][t] = T::mfma(a1, xf[0][kx], acc[2][t]);
          acc[3][t] = T::mfma(a1, xf[1][kx], acc[3][t]);
        }
      }
    }
  }

#pragma unroll
  for (int m = 0; m < 4; ++m)
    dv_wgrad_store_tile<G::KT>(a.ws, split, acc[m], co0 + cow * 32 + (m >> 1) * 16, ci0 + ciw * 32 + (m & 1) * 16, a.Cout,
                               a.Cin, li, lk);
}

struct HwPlan {
  int nby, nbx, splits;
  long long nbricks;
};

HwPlan hw_plan(int B, int Cin, int H, int W, int Cout, int k) {
  HwPlan p;
  p.nby = (H + HW_TY - 1) / HW_TY;
  p.nbx = (W + HW_TX - 1) / HW_TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  // split K so that the grid fills the device once (a block has a CU to itself), within the workspace bound, at least
  // two bricks per split
  const long long mn = (long long)((Cout + HW_CO - 1) / HW_CO) * ((Cin + HW_CI - 1) / HW_CI);
  p.splits = dv_wgrad_splits(HW_TARGET_BLOCKS / mn, (long long)Cout * Cin * k * k, p.nbricks, 2, false);
  return p;
}

bool hw_valid(long long cin, int B, int H, int W, int Cout, int k) {
  return (k == 1 || k == 3) && cin > 0 && B > 0 && H > 0 && W > 0 && Cout > 0 && (long long)H * W < (1ll << 30) &&
         (long long)Cout * cin * k * k <= DV_WGRAD_MAX_WS_FLOATS && (Cout + HW_CO - 1) / HW_CO <= 65535 &&
         (cin + HW_CI - 1) / HW_CI <= 65535;
}

template <class T, class G>
int hw_launch(const DvCatArgs& a, float* dw, hipStream_t s) {
  dim3 grid((unsigned)((a.Cout + HW_CO - 1) / HW_CO), (unsigned)((a.Cin + HW_CI - 1) / HW_CI), (unsigned)a.splits);
  hipLaunchKernelGGL((conv2d_wgrad_cat_mp_kernel<T, G>), grid, dim3(HW_THREADS), 0, s, a);
  return dv_splitk_finish(a.ws, dw, (long long)a.Cout * a.Cin * G::KT, a.splits, s, false);
}

// the two entries of a table: the size (the plan does not depend on the element type) and the checks and the launch
inline size_t conv2d_wgrad_cat_mp_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout, int k) {
  const long long cin = dv_cat_cin(channels, n_inputs);
  if (!hw_valid(cin, B, H, W, Cout, k)) return 0;
  const HwPlan p = hw_plan(B, (int)cin, H, W, Cout, k);
  return (size_t)p.splits * Cout * cin * k * k;
}

template <class T>
int conv2d_wgrad_cat_mp_launch(const float* const* inputs, const int* channels, int n_inputs, const float* g, float* dw,
                               float* workspace, int B, int H, int W, int Cout, int k, dv_stream_t stream) {
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(inputs);
  DV_REQUIRE_PTR(channels);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(n_inputs >= 1 && n_inputs <= DV_CAT_MAX_INPUTS, DV_ERR_SHAPE);
  const long long cin = dv_cat_cin(channels, n_inputs);
  DV_REQUIRE(hw_valid(cin, B, H, W, Cout, k), DV_ERR_SHAPE);
  for (int i = 0; i < n_inputs; ++i) DV_REQUIRE_PTR(inputs[i]);
  const HwPlan p = hw_plan(B, (int)cin, H, W, Cout, k);
  DvCatArgs a;
  dv_cat_fill(a, inputs, channels, n_inputs, (int)cin);
  a.g = g; a.ws = workspace;
  a.B = B; a.H = H; a.W = W; a.Cout = Cout;
  a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  hipStream_t s = (hipStream_t)stream;
  return k == 1 ? hw_launch<T, HwGeo<1>>(a, dw, s) : hw_launch<T, HwGeo<3>>(a, dw, s);
}

}  // namespace
