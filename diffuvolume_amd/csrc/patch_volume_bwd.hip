// Backward of K13 (patch_volume.hip): the two depth-wise (1,3,3) stencils the attention branch applies to the group-wise
// correlation volume (SceneFlow/models/acv_ddim.py:181-188, :377-381), for the training route of ACVNet_DDIM
// (include/diffuvolume_hip_volume_train.h, `dv_patch_volume_bwd_*`).
//
// Per plane (b, g, d), with dl the dilation of group g, (k-1) the 2-D tap offset (ky-1, kx-1), x the gwc plane, go the
// gradient of the output:
//   mid[p]  = sum_k w1[k] x[p + (k-1)]            p in the image, 0 outside (the second convolution pads the first's output)
//   dmid[p] = sum_k w2[k] go[p - (k-1) dl]        p in the image, 0 outside;  go = 0 outside
//   dx[p]   = sum_k w1[k] dmid[p - (k-1)]
//   dw2[k]  = sum_{b,d,p} go[p] mid[p + (k-1) dl]
//   dw1[k]  = sum_{b,d,p} dmid[p] x[p + (k-1)]
//
// One pass: a block owns a 16 x 128 tile of one plane.  It stages x and go with halo 1 + dl in LDS, recomputes mid on the
// tile + halo dl (with the forward's own statement, so with its bits) and dmid on the tile + halo 1 into two further LDS
// buffers, then forms dx and the 18 partial sums over the positions it owns: x and go are read once, dx is written once
// (12 B per element), mid never leaves the chip.  Everything runs on quads of four consecutive columns from aligned
// ds_read_b128, the dilation a template parameter so that every tap is a register index, as in the forward's fast path.
// The two kernels differ only in how they touch global memory -- 16-byte accesses when W % 4 == 0 and x, go, dx lie on
// 16-byte lines, one element at a time otherwise -- so both give the same bits.
//
// Weight gradients: the block reduces its 18 sums by wave shuffles and over its four waves in LDS, in a fixed order, and
// writes them to the workspace slot of its block index; a second launch (one wave per group) adds a group's slots in a
// fixed order in double.  No atomics; every output element is written exactly once.  Work for an output that is not
// wanted (NULL) is skipped: frozen stencils read go and write dx only, and a result that is computed does not depend on
// which of the others are.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int TY = 16, TXB = 128;    // the tile a block owns (the forward's)
constexpr int FIW = TXB + 16;        // x / go row in LDS: image columns x0 - 8 .. x0 + 135 (tile at column 8)
constexpr int FMW = TXB + 8;         // mid / dmid row in LDS: image columns x0 - 4 .. x0 + 131 (tile at column 4)
constexpr int IQ = FIW / 4, MQ = FMW / 4, OQ = TXB / 4;
constexpr int NSUM = 18;             // dw1[0..9), dw2[0..9) of one group
constexpr int THREADS = 256, WAVES = THREADS / DV_WAVE;

struct PatchGeo {
  int gx, gy;
  long long P;        // partial slots per group = B * D * gy * gx
};

PatchGeo patch_geo(int B, int D, int H, int W) {
  PatchGeo g;
  g.gx = (W + TXB - 1) / TXB;
  g.gy = (H + TY - 1) / TY;
  g.P = (long long)B * D * g.gy * g.gx;
  return g;
}

// Four consecutive columns x .. x+3 of image row y of a plane; 0 outside the image.
template <bool VEC>
__device__ __forceinline__ f32x4 load_quad(const float* __restrict__ plane, int y, int x, int H, int W) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if ((unsigned)y >= (unsigned)H) return v;
  const float* row = plane + (size_t)y * W;
  if (VEC) {                                   // W % 4 == 0 and x % 4 == 0: a quad is all in or all out
    if ((unsigned)x < (unsigned)W) v = *reinterpret_cast<const f32x4*>(row + x);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if ((unsigned)(x + i) < (unsigned)W) v[i] = row[x + i];
  }
  return v;
}

template <int DL, bool VEC>
__global__ __launch_bounds__(THREADS) void patch_bwd_kernel(const float* __restrict__ xin, const float* __restrict__ w1,
                                                            const float* __restrict__ w2, const float* __restrict__ gout,
                                                            float* __restrict__ dx, float* __restrict__ ws, long long P,
                                                            long long plane0, int g0, int ng, int G, int D, int H, int W,
                                                            int want_dw1, int want_dw2) {
  constexpr int H1 = 1 + DL, IHV = TY + 2 * H1, MHV = TY + 2 * DL, DHV = TY + 2;
  __shared__ __attribute__((aligned(16))) float x_s[IHV][FIW];
  __shared__ __attribute__((aligned(16))) float g_s[IHV][FIW];
  __shared__ __attribute__((aligned(16))) float mid_s[MHV][FMW];
  __shared__ __attribute__((aligned(16))) float dm_s[DHV][FMW];
  __shared__ float red[NSUM][WAVES];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * TXB, y0 = blockIdx.y * TY;
  // blockIdx.z walks the (b, g in [g0, g0+ng), d) planes of this dilation run
  const unsigned z = (unsigned)(plane0 + blockIdx.z);
  const unsigned d = z % (unsigned)D, r1 = z / (unsigned)D;
  const int g = g0 + (int)(r1 % (unsigned)ng), b = (int)(r1 / (unsigned)ng);
  const size_t pl = ((size_t)b * G + g) * D + d;
  const float* xp = xin + pl * (size_t)H * W;
  const float* gp = gout + pl * (size_t)H * W;
  const bool want_dx = dx != nullptr;
  const bool need_x = want_dw1 || want_dw2, need_dm = want_dx || want_dw1;
  float a[9], c[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { a[i] = w1[g * 9 + i]; c[i] = w2[g * 9 + i]; }

  // x and go, rows y0 - H1 .. y0 + TY + H1, columns x0 - 4 .. x0 + TXB + 4 as quads; the outermost quad of each side is
  // zero (read by the quads next to it, never used)
  for (int e = tid; e < IHV * IQ; e += THREADS) {
    const int r = e / IQ, q = e - r * IQ;
    const int y = y0 - H1 + r, x = x0 - 8 + 4 * q;
    const bool slack = q == 0 || q == IQ - 1;
    f32x4 vx = {0.f, 0.f, 0.f, 0.f}, vg = {0.f, 0.f, 0.f, 0.f};
    if (!slack) {
      vg = load_quad<VEC>(gp, y, x, H, W);
      if (need_x) vx = load_quad<VEC>(xp, y, x, H, W);
    }
    *reinterpret_cast<f32x4*>(&g_s[r][4 * q]) = vg;
    *reinterpret_cast<f32x4*>(&x_s[r][4 * q]) = vx;
  }
  __syncthreads();

  // mid on rows y0 - DL .. y0 + TY + DL, columns x0 - 4 .. x0 + TXB + 4: the forward's statement
  if (want_dw2) {
    for (int e = tid; e < MHV * MQ; e += THREADS) {
      const int r = e / MQ, q = e - r * MQ;
      const int y = y0 - DL + r, x = x0 - 4 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)y < (unsigned)H) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          // image row y + ky - 1 is x_s row r + ky; image column x is x_s column x - x0 + 8 = 4 q + 4
          const float* row = &x_s[r + ky][4 * q];             // image x - 4 .. x + 7
          const f32x4 lo = *reinterpret_cast<const f32x4*>(row), mi = *reinterpret_cast<const f32x4*>(row + 4),
                      hi = *reinterpret_cast<const f32x4*>(row + 8);
          const float t[6] = {lo[3], mi[0], mi[1], mi[2], mi[3], hi[0]};          // x - 1 .. x + 4
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) v[i] = fmaf(a[ky * 3 + kx], t[i + kx], v[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((unsigned)(x + i) >= (unsigned)W) v[i] = 0.f;
      }
      *reinterpret_cast<f32x4*>(&mid_s[r][4 * q]) = v;
    }
  }
  // dmid on rows y0 - 1 .. y0 + TY + 1, the same columns
  if (need_dm) {
    for (int e = tid; e < DHV * MQ; e += THREADS) {
      const int r = e / MQ, q = e - r * MQ;
      const int y = y0 - 1 + r, x = x0 - 4 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if ((unsigned)y < (unsigned)H) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
          // image row y - (ky - 1) DL is g_s row r + (2 - ky) DL; image column x is g_s column 4 q + 4
          const float* row = &g_s[r + (2 - ky) * DL][4 * q];  // image x - 4 .. x + 7
          const f32x4 lo = *reinterpret_cast<const f32x4*>(row), mi = *reinterpret_cast<const f32x4*>(row + 4),
                      hi = *reinterpret_cast<const f32x4*>(row + 8);
          const float t[12] = {lo[0], lo[1], lo[2], lo[3], mi[0], mi[1], mi[2], mi[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) v[i] = fmaf(c[ky * 3 + kx], t[4 + i - (kx - 1) * DL], v[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if ((unsigned)(x + i) >= (unsigned)W) v[i] = 0.f;
      }
      *reinterpret_cast<f32x4*>(&dm_s[r][4 * q]) = v;
    }
  }
  __syncthreads();

  float s1[9], s2[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) s1[i] = s2[i] = 0.f;
  for (int e = tid; e < TY * OQ; e += THREADS) {
    const int r = e / OQ, q = e - r * OQ;
    const int y = y0 + r, x = x0 + 4 * q;
    if (y >= H || x >= W) continue;
    if (want_dx) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        // image row y - (ky - 1) is dm_s row r + 2 - ky; image column x is dm_s column 4 q + 4
        const float* row = &dm_s[r + 2 - ky][4 * q];
        const f32x4 lo = *reinterpret_cast<const f32x4*>(row), mi = *reinterpret_cast<const f32x4*>(row + 4),
                    hi = *reinterpret_cast<const f32x4*>(row + 8);
        const float t[6] = {lo[3], mi[0], mi[1], mi[2], mi[3], hi[0]};            // x - 1 .. x + 4
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) v[i] = fmaf(a[ky * 3 + kx], t[i + 2 - kx], v[i]);
      }
      float* dst = dx + pl * (size_t)H * W + (size_t)y * W + x;
      if (VEC) {
        *reinterpret_cast<f32x4*>(dst) = v;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i < W) dst[i] = v[i];
      }
    }
    if (want_dw1) {
      // dmid of the owned positions (0 outside the image) times x at the nine taps around them
      const f32x4 dm = *reinterpret_cast<const f32x4*>(&dm_s[r + 1][4 * q + 4]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        // image row y + ky - 1 is x_s row r + ky + DL; image column x is x_s column 4 q + 8
        const float* row = &x_s[r + ky + DL][4 * q + 4];
        const f32x4 lo = *reinterpret_cast<const f32x4*>(row), mi = *reinterpret_cast<const f32x4*>(row + 4),
                    hi = *reinterpret_cast<const f32x4*>(row + 8);
        const float t[6] = {lo[3], mi[0], mi[1], mi[2], mi[3], hi[0]};            // x - 1 .. x + 4
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int i = 0; i < 4; ++i) s1[ky * 3 + kx] = fmaf(dm[i], t[i + kx], s1[ky * 3 + kx]);
      }
    }
    if (want_dw2) {
      // go of the owned positions (0 outside the image) times mid at the nine dilated taps around them
      const f32x4 gc = *reinterpret_cast<const f32x4*>(&g_s[r + H1][4 * q + 8]);
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        // image row y + (ky - 1) DL is mid_s row r + ky DL; image column x is mid_s column 4 q + 4
        const float* row = &mid_s[r + ky * DL][4 * q];        // image x - 4 .. x + 7
        const f32x4 lo = *reinterpret_cast<const f32x4*>(row), mi = *reinterpret_cast<const f32x4*>(row + 4),
                    hi = *reinterpret_cast<const f32x4*>(row + 8);
        const float t[12] = {lo[0], lo[1], lo[2], lo[3], mi[0], mi[1], mi[2], mi[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int i = 0; i < 4; ++i) s2[ky * 3 + kx] = fmaf(gc[i], t[4 + i + (kx - 1) * DL], s2[ky * 3 + kx]);
      }
    }
  }
  if (!need_x) return;                                      // block-uniform

  // the block's 18 sums in a fixed order: lanes by halving shuffles, then the four waves in ascending order
#pragma unroll
  for (int k = 0; k < 9; ++k) {
#pragma unroll
    for (int off = DV_WAVE / 2; off > 0; off >>= 1) {
      s1[k] += __shfl_down(s1[k], off, DV_WAVE);
      s2[k] += __shfl_down(s2[k], off, DV_WAVE);
    }
  }
  const int lane = tid & (DV_WAVE - 1), wave = tid / DV_WAVE;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      red[k][wave] = s1[k];
      red[9 + k][wave] = s2[k];
    }
  }
  __syncthreads();
  if (tid < NSUM && (tid < 9 ? want_dw1 : want_dw2)) {
    float s = red[tid][0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) s += red[tid][w];
    // slot of this block among its group's P = B D gy gx: ((b D + d) gy + by) gx + bx
    const size_t slot = (((size_t)b * D + d) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    ws[((size_t)g * (size_t)P + slot) * NSUM + tid] = s;
  }
}

// One wave per group: the group's P slots in a fixed order (lane l takes slots l, l + 64, ... in ascending order, then the
// lanes by halving shuffles), in double.
__global__ __launch_bounds__(DV_WAVE) void patch_bwd_combine_kernel(const float* __restrict__ ws, float* __restrict__ dw1,
                                                                    float* __restrict__ dw2, long long P) {
  const int g = blockIdx.x, lane = threadIdx.x;
  const float* base = ws + (size_t)g * (size_t)P * NSUM;
  for (int k = 0; k < NSUM; ++k) {
    float* out = k < 9 ? dw1 : dw2;
    if (out == nullptr) continue;
    double s = 0.0;
    for (long long p = lane; p < P; p += DV_WAVE) s += (double)base[(size_t)p * NSUM + k];
#pragma unroll
    for (int off = DV_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, DV_WAVE);
    if (lane == 0) out[g * 9 + (k < 9 ? k : k - 9)] = (float)s;
  }
}

template <int DL, bool VEC>
void launch_run(const float* gwc, const float* w1, const float* w2, const float* dout, float* dgwc, float* ws,
                const PatchGeo& geo, int g0, int ng, int B, int G, int D, int H, int W, int want_dw1, int want_dw2,
                hipStream_t stream) {
  const long long planes = (long long)B * ng * D;
  for (long long p0 = 0; p0 < planes; p0 += 65535) {        // grid.z is limited to 65535 planes per launch
    const long long n = planes - p0 < 65535 ? planes - p0 : 65535;
    hipLaunchKernelGGL((patch_bwd_kernel<DL, VEC>), dim3((unsigned)geo.gx, (unsigned)geo.gy, (unsigned)n), dim3(THREADS),
                       0, stream, gwc, w1, w2, dout, dgwc, ws, geo.P, p0, g0, ng, G, D, H, W, want_dw1, want_dw2);
  }
}

}  // namespace

extern "C" size_t dv_patch_volume_bwd_workspace_floats(int B, int G, int D, int H, int W) {
  if (B <= 0 || G <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return (size_t)G * (size_t)patch_geo(B, D, H, W).P * NSUM;
}

extern "C" int dv_patch_volume_bwd_f32(const float* gwc, const float* w1, const float* w2, const float* dout, float* dgwc,
                                       float* dw1, float* dw2, float* workspace, int B, int G, int D, int H, int W,
                                       int nruns, const int* run_g0, const int* run_ng, const int* run_dil,
                                       dv_stream_t stream) {
  DV_REQUIRE_PTR(gwc);
  DV_REQUIRE_PTR(w1);
  DV_REQUIRE_PTR(w2);
  DV_REQUIRE_PTR(dout);
  DV_REQUIRE(dgwc != nullptr || dw1 != nullptr || dw2 != nullptr, DV_ERR_NULL);
  DV_REQUIRE(workspace != nullptr || (dw1 == nullptr && dw2 == nullptr), DV_ERR_NULL);
  DV_REQUIRE(B > 0 && G > 0 && D > 0 && H > 0 && W > 0 && nruns > 0, DV_ERR_SHAPE);
  DV_REQUIRE_PTR(run_g0);
  DV_REQUIRE_PTR(run_ng);
  DV_REQUIRE_PTR(run_dil);
  int covered = 0;
  for (int r = 0; r < nruns; ++r) {
    DV_REQUIRE(run_g0[r] == covered && run_ng[r] > 0 && run_ng[r] <= G - covered && run_dil[r] >= 1 && run_dil[r] <= 3,
               DV_ERR_SHAPE);
    covered += run_ng[r];
  }
  DV_REQUIRE(covered == G, DV_ERR_SHAPE);
  const PatchGeo geo = patch_geo(B, D, H, W);
  DV_REQUIRE(geo.gy <= 65535 && geo.P <= 0x7fffffffLL && (long long)B * G * D <= 0x7fffffffLL, DV_ERR_SHAPE);
  const bool fast = (W % 4 == 0) && dv_aligned16(gwc) && dv_aligned16(dout) && dv_aligned16(dgwc);
  const int want1 = dw1 != nullptr, want2 = dw2 != nullptr;
  hipStream_t st = (hipStream_t)stream;
  for (int r = 0; r < nruns; ++r) {
    const int g0 = run_g0[r], ng = run_ng[r];
#define DV_PATCH_BWD_RUN(DL)                                                                                            \
  (fast ? launch_run<DL, true>(gwc, w1, w2, dout, dgwc, workspace, geo, g0, ng, B, G, D, H, W, want1, want2, st)        \
        : launch_run<DL, false>(gwc, w1, w2, dout, dgwc, workspace, geo, g0, ng, B, G, D, H, W, want1, want2, st))
    switch (run_dil[r]) {
      case 1: DV_PATCH_BWD_RUN(1); break;
      case 2: DV_PATCH_BWD_RUN(2); break;
      default: DV_PATCH_BWD_RUN(3); break;
    }
#undef DV_PATCH_BWD_RUN
  }
  if (want1 || want2)
    hipLaunchKernelGGL(patch_bwd_combine_kernel, dim3((unsigned)G), dim3(DV_WAVE), 0, st, workspace, dw1, dw2, geo.P);
  return dv_launch_status();
}
