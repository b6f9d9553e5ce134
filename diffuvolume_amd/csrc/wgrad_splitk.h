// What the split-K weight gradients share (conv3d_wgrad, conv2d_wgrad, conv2d_wgrad_cat, conv2d_wgrad_cat_f16,
// deconv3d_k4_bwd, deconv2d_k4_bwd, igev_front_bwd): a block walks a contiguous range of output bricks and writes its
// partial dW into the caller's workspace [splits][n]; a second launch (csrc/splitk_reduce.hip) sums the splits in a fixed
// order.  No atomics: the bits of dW depend on the shape only -- through the split count and the brick ranges below, which
// is why they are written once, here, and pinned by tests/test_wgrad_plan_host.py.
// A kernel keeps what distinguishes it: its geometry, staging and MFMA loop, the number of splits it asks for (`want`) and
// the shapes it accepts ("Adding a split-K weight gradient").
#pragma once
#include "dv_common.h"

constexpr long long DV_WGRAD_MAX_WS_FLOATS = 12ll << 20;       // workspace bound: 48 MB

// n rounded up to 2 mod 32: a per-channel LDS stride with which a 32-lane half (16 channels x 2 adjacent positions) reads
// 32 different banks
constexpr int dv_pad_2mod32(int n) { return n + (((2 - n % 32) % 32) + 32) % 32; }

// The split count: the `want` splits that fill the device (the kernel's own figure), within the workspace bound, at least
// `min_bricks_per_split` bricks each, at most 65535 where `clamp_grid_z` asks for it (the limit of the grid dimension that
// carries the split index -- y or z, whichever the kernel uses -- for a kernel that does not check it itself), and one at
// least.
static inline int dv_wgrad_splits(long long want, long long floats_per_split, long long nbricks, int min_bricks_per_split,
                                  bool clamp_grid_z) {
  long long s = want;
  const long long cap = DV_WGRAD_MAX_WS_FLOATS / floats_per_split;
  if (s > cap) s = cap;
  if (s > nbricks / min_bricks_per_split) s = nbricks / min_bricks_per_split;
  if (clamp_grid_z && s > 65535) s = 65535;
  if (s < 1) s = 1;
  return (int)s;
}

// the bricks [b0, b1) of split `split`
__device__ __forceinline__ void dv_split_range(long long nbricks, int split, int splits, long long& b0, long long& b1) {
  b0 = nbricks * split / splits;
  b1 = nbricks * (split + 1) / splits;
}

// brick index -> batch item and brick coordinates (x fastest)
__device__ __forceinline__ void dv_brick_decode2(long long br, int nby, int nbx, int& b, int& by, int& bx) {
  bx = (int)(br % nbx); br /= nbx;
  by = (int)(br % nby); br /= nby;
  b = (int)br;
}
__device__ __forceinline__ void dv_brick_decode3(long long br, int nbz, int nby, int nbx, int& b, int& bz, int& by,
                                                 int& bx) {
  bx = (int)(br % nbx); br /= nbx;
  by = (int)(br % nby); br /= nby;
  bz = (int)(br % nbz); br /= nbz;
  b = (int)br;
}

// One 16 co x 16 ci accumulator tile per tap, its corner at (co0, ci0), into the partial [Cout][Cin][KT] of split `split`
// in the workspace `ws`.  D layout of the 16x16 MFMAs, li = lane & 15, lk = lane >> 4: col = li (ci), row = 4 * lk + r (co).
template <int KT>
__device__ __forceinline__ void dv_wgrad_store_tile(float* ws, int split, const f32x4 (&acc)[KT], int co0, int ci0,
                                                    int Cout, int Cin, int li, int lk) {
  const int ci = ci0 + li;
  if (ci >= Cin) return;
  float* out = ws + (size_t)split * Cout * Cin * KT;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int co = co0 + 4 * lk + rr;
    if (co >= Cout) continue;
    float* o = out + ((size_t)co * Cin + ci) * KT;
#pragma unroll
    for (int t = 0; t < KT; ++t) o[t] = acc[t][rr];
  }
}

// The tail of an entry, behind the main launch: its status, then the sum of the splits (dv_splitk_sum, or
// dv_splitk_sum_quartered for the kernels written with that order) and the status of that.
static inline int dv_splitk_finish(const float* ws, float* dw, long long n, int splits, hipStream_t s, bool quartered) {
  const int rc = dv_launch_status();
  if (rc != DV_OK) return rc;
  if (quartered) dv_splitk_sum_quartered(ws, dw, n, splits, s);
  else dv_splitk_sum(ws, dw, n, splits, s);
  return dv_launch_status();
}

// ---- the virtual channel concatenation of conv2d_wgrad_cat.hip and conv2d_wgrad_cat_f16.hip -------------------------
constexpr int DV_CAT_MAX_INPUTS = 4;

struct DvCatArgs {
  const float* src[DV_CAT_MAX_INPUTS];   // [B, c_i, H, W]
  int coff[DV_CAT_MAX_INPUTS + 1];       // first channel of source i in the concatenation; coff[n..4] = Cin
  const float* g;                        // [B, Cout, H, W]
  float* ws;                             // [splits, Cout, Cin, KT]
  int B, Cin, H, W, Cout;
  int nby, nbx, splits;
  long long nbricks;
};

// plane of channel ci (< Cin) of the concatenation, batch item b
__device__ __forceinline__ const float* dv_cat_plane(const DvCatArgs& a, int ci, int b, size_t plane) {
  const float* p = a.src[0];
  int lo = 0, hi = a.coff[1];
  if (ci >= a.coff[1]) { p = a.src[1]; lo = a.coff[1]; hi = a.coff[2]; }
  if (ci >= a.coff[2]) { p = a.src[2]; lo = a.coff[2]; hi = a.coff[3]; }
  if (ci >= a.coff[3]) { p = a.src[3]; lo = a.coff[3]; hi = a.coff[4]; }
  return p + ((size_t)b * (hi - lo) + (ci - lo)) * plane;
}

// sum of the channel counts, or 0 when the description of the sources is unusable
static inline long long dv_cat_cin(const int* channels, int n_inputs) {
  if (channels == nullptr || n_inputs < 1 || n_inputs > DV_CAT_MAX_INPUTS) return 0;
  long long c = 0;
  for (int i = 0; i < n_inputs; ++i) {
    if (channels[i] <= 0) return 0;
    c += channels[i];
  }
  return c > 0x3fffffff ? 0 : c;
}

// src / coff / Cin of `a` from the entry's description of the sources (cin = dv_cat_cin of it, > 0)
static inline void dv_cat_fill(DvCatArgs& a, const float* const* inputs, const int* channels, int n_inputs, int cin) {
  int off = 0;
  for (int i = 0; i < DV_CAT_MAX_INPUTS; ++i) {
    a.src[i] = inputs[i < n_inputs ? i : 0];
    a.coff[i] = i < n_inputs ? off : cin;
    if (i < n_inputs) off += channels[i];
  }
  a.coff[DV_CAT_MAX_INPUTS] = cin;
  a.Cin = cin;
}
