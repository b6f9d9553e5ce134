// Backward of the bilinear resize with align_corners=True (dv_resize_bilinear_ac_f32, csrc/update_glue.hip), the adjoint
// of that kernel in its own weights:
//
//   dx[bc,i,j] = sum_{Y,X} dy[bc,Y,X] wy(i;Y) wx(j;X),   wy(i;Y) = hy [y0 == i] + ly [y1 == i]   (wx likewise)
//
// with fy, y0, y1, ly, hy the float expressions of `resize_ac_at`.  ATen's backward of F.interpolate scatters with atomics;
// this is a gather: y0(Y) = (int)(sy * Y) is monotone in Y, so the destination rows that touch source row i are the
// contiguous range [first Y with y0 >= i - 1, first Y with y0 > i), found by bisection on that very expression (no
// division whose rounding could disagree with the forward).  Every dx element is written once by one thread, which adds
// its rows in ascending Y, each row a sum in ascending X: no atomics, the same bits on every launch and for every split
// of BC.
//
// One block of 256 threads owns one plane, a band of 8 source rows and a tile of 64 source columns (two outputs per
// thread).  It walks the band's destination rows in chunks of 8: the chunk's dy rows, cut to the tile's destination
// columns, are staged in LDS (16-byte loads when W % 4 == 0 and dy lies on a 16-byte line, element loads otherwise -- the
// same LDS contents, so the same bits), a horizontal pass leaves sum_X wx dy in hs[8][64], and the vertical pass adds
// wy * hs into the two accumulators.  A tile whose destination columns do not fit the stage (a ratio above ~4.7, e.g.
// w == 1) reads dy from memory in the horizontal pass instead: same arithmetic, same bits.
// The case that matters, [4,32,64,128] -> [4,32,256,512], reads 67 MB of dy and writes 4 MB; bands overlap by about
// 4 destination rows in 36, tiles by about 4 columns in 260, and the overlap is served by L2.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int RB = 8;        // source rows per block
constexpr int TW = 64;       // source columns per block
constexpr int YC = 8;        // destination rows per chunk
constexpr int XS = 320;      // floats per staged row: (TW + 1) * ratio + 6 for ratios up to ~4.7; a multiple of 4

// resize_ac_at's scale
__device__ __forceinline__ float scale_ac(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// smallest D in [0, n] with (int)(s * D) >= k; n when there is none.  (int)(s * D) is resize_ac_at's lower tap.
__device__ __forceinline__ int first_tap_ge(float s, int n, int k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((int)(s * (float)mid) >= k) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the weight destination index D gives source index i (of `in` sources), in resize_ac_at's expressions
__device__ __forceinline__ float tap_weight(float s, int in, int D, int i) {
  const float f = s * (float)D;
  const int i0 = (int)f;
  const int i1 = i0 + (i0 < in - 1 ? 1 : 0);
  const float l = f - (float)i0;
  const float h = 1.f - l;
  return (i0 == i ? h : 0.f) + (i1 == i ? l : 0.f);
}

template <bool VEC>
__global__ void __launch_bounds__(256) resize_bilinear_ac_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                                      int h, int w, int H, int W, int tiles, int bands) {
  __shared__ __attribute__((aligned(16))) float stage[YC][XS];
  __shared__ float hs[YC][TW];
  const int t = threadIdx.x, jc = t & (TW - 1), ir = t >> 6;            // ir in 0..3
  const unsigned b = blockIdx.x;
  const int tile = (int)(b % (unsigned)tiles), band = (int)((b / (unsigned)tiles) % (unsigned)bands);
  const size_t bc = b / ((unsigned)tiles * (unsigned)bands);
  const int j0 = tile * TW, i0 = band * RB;
  const int j = j0 + jc, ia = i0 + ir, ib = i0 + ir + 4;
  const float sy = scale_ac(h, H), sx = scale_ac(w, W);
  const float* __restrict__ p = dy + bc * (size_t)H * W;

  // this thread's destination columns, and the tile's (block-uniform)
  const int Xa = first_tap_ge(sx, W, j - 1), Xb = j < w ? first_tap_ge(sx, W, j + 1) : Xa;
  const int jl = min(j0 + TW, w) - 1;
  const int Xlo = first_tap_ge(sx, W, j0 - 1) & ~3, Xhi = first_tap_ge(sx, W, jl + 1);
  const bool staged = Xhi - Xlo <= XS - 3;                               // (a 16-byte load may run 3 past Xhi)
  // the band's destination rows, and this thread's two ranges
  const int il = min(i0 + RB, h) - 1;
  const int Ylo = first_tap_ge(sy, H, i0 - 1), Yhi = first_tap_ge(sy, H, il + 1);
  const int Ya0 = first_tap_ge(sy, H, ia - 1), Ya1 = ia < h ? first_tap_ge(sy, H, ia + 1) : Ya0;
  const int Yb0 = first_tap_ge(sy, H, ib - 1), Yb1 = ib < h ? first_tap_ge(sy, H, ib + 1) : Yb0;

  float acc_a = 0.f, acc_b = 0.f;
  for (int Yc = Ylo; Yc < Yhi; Yc += YC) {
    const int rows = min(YC, Yhi - Yc);
    if (staged) {
      if (VEC) {
        const int n4 = (Xhi - Xlo + 3) >> 2;                             // W % 4 == 0: Xlo + 4 n4 <= W
        for (int e = t; e < rows * n4; e += 256) {
          const int r = e / n4, q = e - r * n4;
          *reinterpret_cast<float4*>(&stage[r][4 * q]) =
              *reinterpret_cast<const float4*>(p + (size_t)(Yc + r) * W + Xlo + 4 * q);
        }
      } else {
        const int n = Xhi - Xlo;
        for (int e = t; e < rows * n; e += 256) {
          const int r = e / n, q = e - r * n;
          stage[r][q] = p[(size_t)(Yc + r) * W + Xlo + q];
        }
      }
      __syncthreads();
    }
    // horizontal pass: rows ir and ir + 4 of the chunk, column jc
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = ir + 4 * k;
      float s = 0.f;
      if (r < rows) {
        if (staged) {
          for (int X = Xa; X < Xb; ++X) s = fmaf(tap_weight(sx, w, X, j), stage[r][X - Xlo], s);
        } else {
          const float* __restrict__ row = p + (size_t)(Yc + r) * W;
          for (int X = Xa; X < Xb; ++X) s = fmaf(tap_weight(sx, w, X, j), row[X], s);
        }
      }
      hs[r][jc] = s;
    }
    __syncthreads();
    // vertical pass, ascending Y
    for (int r = 0; r < rows; ++r) {
      const int Y = Yc + r;
      const float v = hs[r][jc];
      if (Y >= Ya0 && Y < Ya1) acc_a = fmaf(tap_weight(sy, h, Y, ia), v, acc_a);
      if (Y >= Yb0 && Y < Yb1) acc_b = fmaf(tap_weight(sy, h, Y, ib), v, acc_b);
    }
    __syncthreads();
  }
  if (j < w) {
    float* __restrict__ o = dx + bc * (size_t)h * w;
    if (ia < h) o[(size_t)ia * w + j] = acc_a;
    if (ib < h) o[(size_t)ib * w + j] = acc_b;
  }
}

}  // namespace

extern "C" int dv_resize_bilinear_ac_bwd_f32(const float* dy, float* dx, int BC, int h, int w, int H, int W,
                                             dv_stream_t stream) {
  DV_REQUIRE_PTR(dy);
  DV_REQUIRE_PTR(dx);
  DV_REQUIRE(BC > 0 && h > 0 && w > 0 && H > 0 && W > 0, DV_ERR_NULL);   // (no plane: no element a pointer could name)
  const int tiles = (w + TW - 1) / TW, bands = (h + RB - 1) / RB;
  const long long blocks = (long long)BC * tiles * bands;
  DV_REQUIRE(blocks <= 0x7fffffffLL, DV_ERR_SHAPE);
  const dim3 grid((unsigned)blocks), block(256);
  if (W % 4 == 0 && dv_aligned16(dy))
    hipLaunchKernelGGL(resize_bilinear_ac_bwd_kernel<true>, grid, block, 0, (hipStream_t)stream, dy, dx, h, w, H, W, tiles,
                       bands);
  else
    hipLaunchKernelGGL(resize_bilinear_ac_bwd_kernel<false>, grid, block, 0, (hipStream_t)stream, dy, dx, h, w, H, W, tiles,
                       bands);
  return dv_launch_status();
}
