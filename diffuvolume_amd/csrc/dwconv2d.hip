// Depthwise 3x3 convolution (padding 1, stride 1 or 2) of MobileNetV2's blocks, forward and backward
// (include/diffuvolume_hip_volume_train.h, `dv_dwconv3x3_*`): nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) with
// eval BatchNorm folded into scale / shift and ReLU / ReLU6 applied inside the launch.
//
// A streaming kernel: 9 FMAs per 8 bytes, so everything here is about touching each byte once with 16-byte accesses.
//   * The unit of work is one WAVE and one tile of one (b, c) plane.  The 64 lanes are LX x LY (LX a power of two picked
//     from the row width alone): a lane owns four consecutive output columns and walks TH consecutive output rows.  Wide
//     planes (the 1/2 and 1/4 levels) take LX = 64, LY = 1; the narrow 1/16 and 1/32 planes fold several row bands into
//     one wave instead of idling three quarters of it.
//   * Register window: an input row is read ONCE per lane as one aligned quad (two at stride 2); the two halo columns
//     come from the neighbouring lanes by a wave shuffle (the outermost lanes of a row read theirs from memory).  The three
//     rows an output row needs are kept in registers and rotated, so a row serves its three vertical taps from one load.
//   * Items are numbered (plane, band, tile) and handed to the waves of a capped grid by a grid-stride loop.  The tiling
//     looks at H and W only, never at B or the grid, and a lane sums its nine taps in one fixed order (ky, then kx, one
//     fmaf each), so an item of a batch has the bits of the item run alone.
//   * VEC / element paths differ only in how a quad is moved (one 16-byte access, or four 4-byte accesses with the column
//     test per element); the arithmetic is the same statement, so both give the same bits.
//
// Backward of the bare convolution:
//   dx, stride 1   the forward kernel on dy with the taps reversed.
//   dx, stride 2   a gather: a lane reads a dy quad (+ the right neighbour's first column) of rows m and m + 1 and writes
//                  the eight dx columns and two dx rows (2m, 2m + 1) they own.  Which taps reach an element depends on the
//                  parity of its row and column: 1, 2, 2 or 4 of them.  Each dy row is read once, each dx element written once.
//   dw             the forward's window over x, times the dy quad of the lane: nine sums per lane, reduced over the wave by
//                  halving shuffles, one slot of nine floats per ITEM in the workspace (so the partials do not depend on
//                  the grid), then one wave per channel adds a channel's B * items-per-plane slots in a fixed order in double.
// No atomics anywhere; every output element is written exactly once.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

#include <math.h>

namespace {

constexpr int THREADS = 256, WAVES = THREADS / DV_WAVE;
constexpr int MAX_BLOCKS = 2048;                 // 256 CUs x 8 blocks: the rest of the items by the grid-stride loop
constexpr int MAX_ITEMS = 0x7fff0000;            // the item counter is an int and steps by at most MAX_BLOCKS * WAVES

// How one plane is cut into wave items: LX = 1 << lxlog lanes side by side (four output columns each), LY = 64 / LX row
// bands of th rows below one another.  A function of the OUTPUT plane's size only.
struct DwGeo {
  int lxlog, th, ntx, nby, ipp;
};

DwGeo dw_geo(int Ho, int Wo, int th_max) {
  DwGeo g;
  const int quads = (Wo + 3) / 4;
  g.lxlog = 0;
  while ((1 << g.lxlog) < quads && g.lxlog < 6) ++g.lxlog;
  const int LX = 1 << g.lxlog, LY = DV_WAVE / LX;
  g.th = (Ho + LY - 1) / LY;
  g.th = g.th > th_max ? th_max : g.th;
  g.ntx = (quads + LX - 1) / LX;
  g.nby = (Ho + LY * g.th - 1) / (LY * g.th);
  g.ipp = g.ntx * g.nby;
  return g;
}

// Keeps a wave-uniform value in a vector register: the forward kernel's nine taps, scale and shift would otherwise sit in
// scalar registers beside its pointers, sizes and loop state, which is more than a wave has.
__device__ __forceinline__ float in_vgpr(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Columns x .. x+3 of row y of a plane, 0 outside the image.  VEC: W % 4 == 0, x % 4 == 0 and the plane on a 16-byte line.
// Without a branch: the address is clamped into the plane (so it is always one of the plane's own elements) and the value
// is dropped afterwards -- a lane outside the image re-reads an element its neighbours have in cache.
template <bool VEC>
__device__ __forceinline__ f32x4 ld_quad(const float* __restrict__ plane, int y, int x, int H, int W) {
  const bool yin = (unsigned)y < (unsigned)H;
  const float* row = plane + (size_t)clampi(y, 0, H - 1) * W;
  f32x4 v;
  if (VEC) {
    v = *reinterpret_cast<const f32x4*>(row + clampi(x, 0, W - 4));
    const bool in = yin && (unsigned)x < (unsigned)W;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = in ? v[i] : 0.f;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float e = row[clampi(x + i, 0, W - 1)];
      v[i] = (yin && (unsigned)(x + i) < (unsigned)W) ? e : 0.f;
    }
  }
  return v;
}

__device__ __forceinline__ float ld_one(const float* __restrict__ plane, int y, int x, int H, int W) {
  const float e = plane[(size_t)clampi(y, 0, H - 1) * W + clampi(x, 0, W - 1)];
  return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? e : 0.f;
}

template <bool VEC>
__device__ __forceinline__ void st_quad(float* __restrict__ plane, int y, int x, int H, int W, const f32x4 v) {
  if ((unsigned)y >= (unsigned)H) return;
  float* row = plane + (size_t)y * W;
  if (VEC) {
    if ((unsigned)x < (unsigned)W) *reinterpret_cast<f32x4*>(row + x) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((unsigned)(x + i) < (unsigned)W) row[x + i] = v[i];
  }
}

// The input columns the four outputs of a lane read in row y: stride 1, x-1 .. x+4 (6); stride 2, x-1 .. x+7 (9) with x the
// input column of the lane's first output.  Every lane of the wave calls this (the shuffles need them all).
template <int S>
struct Win {
  static constexpr int N = S == 1 ? 6 : 9;
  float t[N];
};

template <int S, bool VEC>
__device__ __forceinline__ Win<S> window(const float* __restrict__ plane, int y, int x, int H, int W, bool first, bool last) {
  Win<S> r;
  const f32x4 a = ld_quad<VEC>(plane, y, x, H, W);
  if (S == 1) {
    float l = __shfl_up(a[3], 1, DV_WAVE), rt = __shfl_down(a[0], 1, DV_WAVE);
    if (first) l = ld_one(plane, y, x - 1, H, W);
    if (last) rt = ld_one(plane, y, x + 4, H, W);
    r.t[0] = l;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.t[1 + i] = a[i];
    r.t[5] = rt;
  } else {
    const f32x4 b = ld_quad<VEC>(plane, y, x + 4, H, W);
    float l = __shfl_up(b[3], 1, DV_WAVE);
    if (first) l = ld_one(plane, y, x - 1, H, W);
    r.t[0] = l;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r.t[1 + i] = a[i];
      r.t[5 + i] = b[i];
    }
  }
  return r;
}

struct Item {
  int bc, by, tx, r;
};

__device__ __forceinline__ Item split_item(int item, const DwGeo& g) {
  Item it;
  it.bc = item / g.ipp;
  it.r = item - it.bc * g.ipp;
  it.by = it.r / g.ntx;
  it.tx = it.r - it.by * g.ntx;
  return it;
}

// out = act(conv3x3(x) * scale + shift); `flip`: the taps reversed (the stride-1 input gradient).
template <int S, bool VIN, bool VOUT>
__global__ __launch_bounds__(THREADS) void dwconv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float* __restrict__ out,
                                                             int C, int H, int W, int Ho, int Wo, DwGeo g, int nitems,
                                                             int flip, int relu, float upper) {
  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  const int LX = 1 << g.lxlog, LY = DV_WAVE >> g.lxlog;
  const int lx = lane & (LX - 1), ly = lane >> g.lxlog;
  const bool first = lx == 0, last = lx == LX - 1;
  for (int it0 = blockIdx.x * WAVES + wave; it0 < nitems; it0 += gridDim.x * WAVES) {
    const Item it = split_item(__builtin_amdgcn_readfirstlane(it0), g);
    const int c = it.bc % C;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = in_vgpr(w[c * 9 + (flip ? 8 - i : i)]);
    const bool affine = scale != nullptr;
    const float sc = in_vgpr(affine ? scale[c] : 1.f), sh = in_vgpr(affine ? shift[c] : 0.f);
    const float* xp = x + (size_t)it.bc * H * W;
    float* op = out + (size_t)it.bc * Ho * Wo;
    const int ox = (it.tx * LX + lx) * 4, ix = ox * S;
    const int band0 = it.by * LY * g.th, oy0 = band0 + ly * g.th;
    Win<S> top = window<S, VIN>(xp, oy0 * S - 1, ix, H, W, first, last), mid, bot;
    if (S == 1) mid = window<S, VIN>(xp, oy0, ix, H, W, first, last);
    for (int j = 0; j < g.th; ++j) {
      if (band0 + j >= Ho) break;                                     // wave-uniform: the first band's row is the lowest
      const int oy = oy0 + j;
      if (S == 1) {
        bot = window<S, VIN>(xp, oy + 1, ix, H, W, first, last);
      } else {
        mid = window<S, VIN>(xp, 2 * oy, ix, H, W, first, last);
        bot = window<S, VIN>(xp, 2 * oy + 1, ix, H, W, first, last);
      }
      f32x4 v;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float a = 0.f;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) a = fmaf(k[kx], top.t[i * S + kx], a);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) a = fmaf(k[3 + kx], mid.t[i * S + kx], a);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) a = fmaf(k[6 + kx], bot.t[i * S + kx], a);
        if (affine) a = fmaf(a, sc, sh);
        if (relu) a = fminf(fmaxf(a, 0.f), upper);
        v[i] = a;
      }
      st_quad<VOUT>(op, oy, ox, Ho, Wo, v);
      if (S == 1) {
        top = mid;
        mid = bot;
      } else {
        top = bot;
      }
    }
  }
}

// dx of the stride-2 convolution.  The tiling is the forward's over the dy plane [Ho, Wo]; a lane with dy columns n .. n+3
// of rows m (cur) and m+1 (nxt) writes dx columns 2n .. 2n+7 of rows 2m and 2m+1:
//   dx[2m,   2n]   = w11 dy[m,n]
//   dx[2m,   2n+1] = w10 dy[m,n+1] + w12 dy[m,n]
//   dx[2m+1, 2n]   = w01 dy[m+1,n] + w21 dy[m,n]
//   dx[2m+1, 2n+1] = w00 dy[m+1,n+1] + w02 dy[m+1,n] + w20 dy[m,n+1] + w22 dy[m,n]
template <bool VDY, bool VDX>
__global__ __launch_bounds__(THREADS) void dwconv_dx_s2_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                               float* __restrict__ dx, int C, int H, int W, int Ho, int Wo,
                                                               DwGeo g, int nitems) {
  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  const int LX = 1 << g.lxlog, LY = DV_WAVE >> g.lxlog;
  const int lx = lane & (LX - 1), ly = lane >> g.lxlog;
  const bool last = lx == LX - 1;
  for (int it0 = blockIdx.x * WAVES + wave; it0 < nitems; it0 += gridDim.x * WAVES) {
    const Item it = split_item(__builtin_amdgcn_readfirstlane(it0), g);
    const int c = it.bc % C;
    float k[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = w[c * 9 + i];
    const float* gp = dy + (size_t)it.bc * Ho * Wo;
    float* dp = dx + (size_t)it.bc * H * W;
    const int n = (it.tx * LX + lx) * 4;
    const int band0 = it.by * LY * g.th, m0 = band0 + ly * g.th;
    float cur[5], nxt[5];
    {
      const f32x4 q = ld_quad<VDY>(gp, m0, n, Ho, Wo);
      float rt = __shfl_down(q[0], 1, DV_WAVE);
      if (last) rt = ld_one(gp, m0, n + 4, Ho, Wo);
#pragma unroll
      for (int i = 0; i < 4; ++i) cur[i] = q[i];
      cur[4] = rt;
    }
    for (int j = 0; j < g.th; ++j) {
      if (band0 + j >= Ho) break;
      const int m = m0 + j;
      {
        const f32x4 q = ld_quad<VDY>(gp, m + 1, n, Ho, Wo);
        float rt = __shfl_down(q[0], 1, DV_WAVE);
        if (last) rt = ld_one(gp, m + 1, n + 4, Ho, Wo);
#pragma unroll
        for (int i = 0; i < 4; ++i) nxt[i] = q[i];
        nxt[4] = rt;
      }
      f32x4 e0, e1, o0, o1;                    // dx row 2m columns 2n..2n+3, 2n+4..2n+7; row 2m+1 likewise
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ev = k[4] * cur[i];
        const float eo = fmaf(k[5], cur[i], k[3] * cur[i + 1]);
        const float ov = fmaf(k[7], cur[i], k[1] * nxt[i]);
        const float oo = fmaf(k[8], cur[i], fmaf(k[6], cur[i + 1], fmaf(k[2], nxt[i], k[0] * nxt[i + 1])));
        if (i < 2) {
          e0[2 * i] = ev; e0[2 * i + 1] = eo; o0[2 * i] = ov; o0[2 * i + 1] = oo;
        } else {
          e1[2 * i - 4] = ev; e1[2 * i - 3] = eo; o1[2 * i - 4] = ov; o1[2 * i - 3] = oo;
        }
      }
      if (m < Ho) {                            // rows past the dy plane own no dx row (2m >= H)
        st_quad<VDX>(dp, 2 * m, 2 * n, H, W, e0);
        st_quad<VDX>(dp, 2 * m, 2 * n + 4, H, W, e1);
        st_quad<VDX>(dp, 2 * m + 1, 2 * n, H, W, o0);
        st_quad<VDX>(dp, 2 * m + 1, 2 * n + 4, H, W, o1);
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) cur[i] = nxt[i];
    }
  }
}

// dw partials: slot (c, b * ipp + item-in-plane) of nine floats.
template <int S, bool VIN, bool VDY>
__global__ __launch_bounds__(THREADS) void dwconv_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            float* __restrict__ ws, int B, int C, int H, int W, int Ho,
                                                            int Wo, DwGeo g, int nitems) {
  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  const int LX = 1 << g.lxlog, LY = DV_WAVE >> g.lxlog;
  const int lx = lane & (LX - 1), ly = lane >> g.lxlog;
  const bool first = lx == 0, last = lx == LX - 1;
  for (int it0 = blockIdx.x * WAVES + wave; it0 < nitems; it0 += gridDim.x * WAVES) {
    const Item it = split_item(__builtin_amdgcn_readfirstlane(it0), g);
    const int c = it.bc % C, b = it.bc / C;
    const float* xp = x + (size_t)it.bc * H * W;
    const float* gp = dy + (size_t)it.bc * Ho * Wo;
    const int ox = (it.tx * LX + lx) * 4, ix = ox * S;
    const int band0 = it.by * LY * g.th, oy0 = band0 + ly * g.th;
    float s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0.f;
    Win<S> top = window<S, VIN>(xp, oy0 * S - 1, ix, H, W, first, last), mid, bot;
    if (S == 1) mid = window<S, VIN>(xp, oy0, ix, H, W, first, last);
    for (int j = 0; j < g.th; ++j) {
      if (band0 + j >= Ho) break;
      const int oy = oy0 + j;
      if (S == 1) {
        bot = window<S, VIN>(xp, oy + 1, ix, H, W, first, last);
      } else {
        mid = window<S, VIN>(xp, 2 * oy, ix, H, W, first, last);
        bot = window<S, VIN>(xp, 2 * oy + 1, ix, H, W, first, last);
      }
      const f32x4 q = ld_quad<VDY>(gp, oy, ox, Ho, Wo);                // 0 outside the dy plane
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[kx] = fmaf(q[i], top.t[i * S + kx], s[kx]);
          s[3 + kx] = fmaf(q[i], mid.t[i * S + kx], s[3 + kx]);
          s[6 + kx] = fmaf(q[i], bot.t[i * S + kx], s[6 + kx]);
        }
      if (S == 1) {
        top = mid;
        mid = bot;
      } else {
        top = bot;
      }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int off = DV_WAVE / 2; off > 0; off >>= 1) s[i] += __shfl_down(s[i], off, DV_WAVE);
    if (lane == 0) {
      float* slot = ws + (((size_t)c * B + b) * g.ipp + it.r) * 9;
#pragma unroll
      for (int i = 0; i < 9; ++i) slot[i] = s[i];
    }
  }
}

// One wave per channel: the channel's P slots in a fixed order (lane l takes slots l, l + 64, ... ascending, then the lanes
// by halving shuffles), in double.
__global__ __launch_bounds__(DV_WAVE) void dwconv_dw_combine_kernel(const float* __restrict__ ws, float* __restrict__ dw,
                                                                    long long P) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const float* base = ws + (size_t)c * (size_t)P * 9;
  for (int k = 0; k < 9; ++k) {
    double s = 0.0;
    for (long long p = lane; p < P; p += DV_WAVE) s += (double)base[(size_t)p * 9 + k];
#pragma unroll
    for (int off = DV_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, DV_WAVE);
    if (lane == 0) dw[c * 9 + k] = (float)s;
  }
}

struct DwPlan {
  DwGeo g;
  int Ho, Wo, nitems, blocks;
  bool ok;
};

DwPlan dw_plan(int B, int C, int H, int W, int stride) {
  DwPlan p;
  p.Ho = (H - 1) / stride + 1;
  p.Wo = (W - 1) / stride + 1;
  p.g = dw_geo(p.Ho, p.Wo, stride == 1 ? 16 : 8);
  const long long items = (long long)B * C * p.g.ipp;
  p.ok = items <= MAX_ITEMS && (long long)B * C <= 0x7fffffffLL;
  p.nitems = p.ok ? (int)items : 0;
  const long long blocks = (items + WAVES - 1) / WAVES;
  p.blocks = (int)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS);
  return p;
}

bool rows_vec(const void* p, int W) { return W % 4 == 0 && dv_aligned16(p); }

template <int S>
void launch_fwd(const float* x, const float* w, const float* scale, const float* shift, float* out, int C, int H, int W,
                const DwPlan& p, int flip, int relu, float upper, hipStream_t st) {
  const bool vin = rows_vec(x, W), vout = rows_vec(out, p.Wo);
#define DV_DW_FWD(VI, VO)                                                                                              \
  hipLaunchKernelGGL((dwconv_fwd_kernel<S, VI, VO>), dim3((unsigned)p.blocks), dim3(THREADS), 0, st, x, w, scale, shift, \
                     out, C, H, W, p.Ho, p.Wo, p.g, p.nitems, flip, relu, upper)
  if (vin && vout) DV_DW_FWD(true, true);
  else if (vin) DV_DW_FWD(true, false);
  else if (vout) DV_DW_FWD(false, true);
  else DV_DW_FWD(false, false);
#undef DV_DW_FWD
}

template <int S>
void launch_dw(const float* x, const float* dy, float* ws, int B, int C, int H, int W, const DwPlan& p, hipStream_t st) {
  const bool vin = rows_vec(x, W), vdy = rows_vec(dy, p.Wo);
#define DV_DW_DW(VI, VG)                                                                                               \
  hipLaunchKernelGGL((dwconv_dw_kernel<S, VI, VG>), dim3((unsigned)p.blocks), dim3(THREADS), 0, st, x, dy, ws, B, C, H, W, \
                     p.Ho, p.Wo, p.g, p.nitems)
  if (vin && vdy) DV_DW_DW(true, true);
  else if (vin) DV_DW_DW(true, false);
  else if (vdy) DV_DW_DW(false, true);
  else DV_DW_DW(false, false);
#undef DV_DW_DW
}

void launch_dx_s2(const float* dy, const float* w, float* dx, int C, int H, int W, const DwPlan& p, hipStream_t st) {
  const bool vdy = rows_vec(dy, p.Wo), vdx = rows_vec(dx, W);
#define DV_DW_DX(VG, VX)                                                                                               \
  hipLaunchKernelGGL((dwconv_dx_s2_kernel<VG, VX>), dim3((unsigned)p.blocks), dim3(THREADS), 0, st, dy, w, dx, C, H, W, \
                     p.Ho, p.Wo, p.g, p.nitems)
  if (vdy && vdx) DV_DW_DX(true, true);
  else if (vdy) DV_DW_DX(true, false);
  else if (vdx) DV_DW_DX(false, true);
  else DV_DW_DX(false, false);
#undef DV_DW_DX
}

}  // namespace

extern "C" int dv_dwconv3x3_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int B,
                                int C, int H, int W, int stride, int act, float relu_max, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(w);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE((scale == nullptr) == (shift == nullptr), DV_ERR_NULL);
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE(stride == 1 || stride == 2, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(act == DV_ACT_NONE || act == DV_ACT_RELU, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(relu_max >= 0.f && (act == DV_ACT_RELU || relu_max == 0.f), DV_ERR_UNSUPPORTED);     // (NaN fails too)
  const DwPlan p = dw_plan(B, C, H, W, stride);
  DV_REQUIRE(p.ok, DV_ERR_SHAPE);
  const float upper = relu_max > 0.f ? relu_max : INFINITY;
  hipStream_t st = (hipStream_t)stream;
  if (stride == 1) launch_fwd<1>(x, w, scale, shift, out, C, H, W, p, 0, act == DV_ACT_RELU, upper, st);
  else launch_fwd<2>(x, w, scale, shift, out, C, H, W, p, 0, act == DV_ACT_RELU, upper, st);
  return dv_launch_status();
}

extern "C" size_t dv_dwconv3x3_bwd_workspace_floats(int B, int C, int H, int W, int stride) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || (stride != 1 && stride != 2)) return 0;
  const DwPlan p = dw_plan(B, C, H, W, stride);
  return p.ok ? (size_t)p.nitems * 9 : 0;
}

extern "C" int dv_dwconv3x3_bwd_f32(const float* x, const float* w, const float* dy, float* dx, float* dw, float* workspace,
                                    int B, int C, int H, int W, int stride, dv_stream_t stream) {
  DV_REQUIRE_PTR(dy);
  DV_REQUIRE(dx != nullptr || dw != nullptr, DV_ERR_NULL);
  DV_REQUIRE(dx == nullptr || w != nullptr, DV_ERR_NULL);
  DV_REQUIRE(dw == nullptr || (x != nullptr && workspace != nullptr), DV_ERR_NULL);
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE(stride == 1 || stride == 2, DV_ERR_UNSUPPORTED);
  const DwPlan p = dw_plan(B, C, H, W, stride);
  DV_REQUIRE(p.ok, DV_ERR_SHAPE);
  hipStream_t st = (hipStream_t)stream;
  if (dx != nullptr) {
    if (stride == 1) launch_fwd<1>(dy, w, nullptr, nullptr, dx, C, H, W, p, 1, 0, INFINITY, st);
    else launch_dx_s2(dy, w, dx, C, H, W, p, st);
  }
  if (dw != nullptr) {
    if (stride == 1) launch_dw<1>(x, dy, workspace, B, C, H, W, p, st);
    else launch_dw<2>(x, dy, workspace, B, C, H, W, p, st);
    hipLaunchKernelGGL(dwconv_dw_combine_kernel, dim3((unsigned)C), dim3(DV_WAVE), 0, st, workspace, dw,
                       (long long)B * p.g.ipp);
  }
  return dv_launch_status();
}
