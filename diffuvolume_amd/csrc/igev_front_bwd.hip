// The two backward kernels IGEV's once-per-pair 2-D front needs beside the convolution backward kernels of
// conv2d_wgrad*.hip / deconv2d_k4_bwd.hip, so that it trains without MIOpen (whose backward-weights does not return the
// same bits twice).  Both are fp32 and atomics-free: every output element is written once, in an order that depends on
// the shape only.
//   dv_instance_norm_act_bwd_f32  backward of dv_instance_norm_act_f32 (csrc/igev_front.hip): nn.InstanceNorm2d
//                                 (affine=False) + none / ReLU / LeakyReLU(0.01) of BasicConv_IN and the stems
//                                 (KITTI15/core/submodule.py:79-107, igev_stereo_ddim.py:100-117).
//   dv_conv2d_fewin_wgrad_f32     weight gradient of dv_conv2d_fewin_f32: `stem_2[0]` (3 -> 32, k3, s2,
//                                 igev_stereo_ddim.py:100-103), `cnet.conv1` (3 -> 64, k7, s2, core/extractor.py:197) and a
//                                 plain backbone's `conv_stem`.  Images are data: there is no input gradient.
#include "wgrad_splitk.h"

namespace {

// ---- InstanceNorm + activation, backward -----------------------------------------------------------------------------
// One block of 1024 threads per (b, c) plane, like the forward.  Passes 1 and 2 are the forward's, statement for statement
// (per-thread sums over the stride-1024 elements, the same tree), so mean and rstd -- and with them the sign of every
// x_hat the activation's derivative looks at -- are the forward's bits.  Pass 3 sums gh = g * act'(x_hat) and gh * x_hat,
// pass 4 writes dx = rstd * (gh - mean(gh) - x_hat * mean(gh * x_hat)); both as float4 when the plane allows it.  A plane
// is read four times (g twice): after the first pass it comes from L2 (the largest plane of the real workload, 160 x 368
// floats, is 230 KB).  HW = 1: x_hat = 0 and gh = mean(gh), so dx = 0 exactly (rstd = 1/sqrt(eps) is finite).
__device__ __forceinline__ float in_act_grad(float xh, int act) {
  if (act == DV_ACT_RELU) return xh > 0.0f ? 1.0f : 0.0f;
  if (act == DV_ACT_LEAKY) return xh > 0.0f ? 1.0f : 0.01f;
  return 1.0f;
}

template <bool VEC4>
__global__ __launch_bounds__(1024) void instance_norm_act_bwd_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ g, float* __restrict__ dx,
                                                                     int HW, float eps, int act) {
  __shared__ float red[16];
  __shared__ float stat;
  const size_t base = (size_t)blockIdx.x * HW;
  const float* p = x + base;
  const float* gp = g + base;
  float* o = dx + base;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  auto block_sum = [&](float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();                                 // `red` / `stat` of the previous reduction have been read
    if (lane == 0) red[wv] = v;
    __syncthreads();
    if (tid == 0) {
      float s = 0.f;
      for (int i = 0; i < 16; ++i) s += red[i];
      stat = s;
    }
    __syncthreads();
    return stat;
  };
  float s = 0.f;
  for (int i = tid; i < HW; i += 1024) s += p[i];
  const float mean = block_sum(s) / (float)HW;
  float q = 0.f;
  for (int i = tid; i < HW; i += 1024) {
    const float d = p[i] - mean;
    q = fmaf(d, d, q);
  }
  const float rstd = 1.0f / sqrtf(block_sum(q) / (float)HW + eps);

  float s1 = 0.f, s2 = 0.f;
  if (VEC4) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(gp);
    for (int i = tid; i < HW / 4; i += 1024) {
      const float4 xv = p4[i], gv = g4[i];
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (xs[j] - mean) * rstd;
        const float gh = gs[j] * in_act_grad(xh, act);
        s1 += gh;
        s2 = fmaf(gh, xh, s2);
      }
    }
  } else {
    for (int i = tid; i < HW; i += 1024) {
      const float xh = (p[i] - mean) * rstd;
      const float gh = gp[i] * in_act_grad(xh, act);
      s1 += gh;
      s2 = fmaf(gh, xh, s2);
    }
  }
  const float m1 = block_sum(s1) / (float)HW;
  const float m2 = block_sum(s2) / (float)HW;

  if (VEC4) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4* g4 = reinterpret_cast<const float4*>(gp);
    float4* o4 = reinterpret_cast<float4*>(o);
    for (int i = tid; i < HW / 4; i += 1024) {
      const float4 xv = p4[i], gv = g4[i];
      const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, gs[4] = {gv.x, gv.y, gv.z, gv.w};
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float xh = (xs[j] - mean) * rstd;
        const float gh = gs[j] * in_act_grad(xh, act);
        r[j] = rstd * ((gh - m1) - xh * m2);
      }
      o4[i] = make_float4(r[0], r[1], r[2], r[3]);
    }
  } else {
    for (int i = tid; i < HW; i += 1024) {
      const float xh = (p[i] - mean) * rstd;
      const float gh = gp[i] * in_act_grad(xh, act);
      o[i] = rstd * ((gh - m1) - xh * m2);
    }
  }
}

// ---- few-input-channel convolution, weight gradient ------------------------------------------------------------------
//   dw[co,ci,ky,kx] = sum_{b,y,x} g[b,co,y,x] * x[b,ci,y*S-P+ky,x*S-P+kx]          (x zero outside the image)
// VALU.  A block owns FW_COB output channels and one split of the reduction; thread t < Cin*K*K owns the tap
// (ci, ky, kx) = t and keeps its FW_COB sums in registers.  The reduction runs over bricks of FW_TY x FW_TX output
// pixels of the whole batch: the haloed input tile of all (<= 4) input channels and the g tile [FW_COB][brick] are staged
// in LDS (zero outside the image / beyond Cout, so edges need no branch in the inner loop); a thread gathers four
// neighbouring pixels of its tap from the halo and reads g as float4 broadcasts (all lanes the same address).
// Summation order of one dw element: one fma chain over the pixels of the split's bricks in brick order, then the splits
// by dv_splitk_sum_quartered (four quarters of the split range in split order each, then the quarters in order).
constexpr int FW_TY = 8, FW_TX = 16, FW_PIX = FW_TY * FW_TX;
constexpr int FW_COB = 16, FW_THREADS = 256, FW_MAX_CIN = 4;
constexpr int FW_TARGET_BLOCKS = 1024;                           // four blocks per CU on 256 CUs

struct FwArgs {
  const float* x;     // [B, Cin, H, W]
  const float* g;     // [B, Cout, Ho, Wo]
  float* ws;          // [splits, Cout, Cin*K*K]
  int B, Cin, H, W, Cout, Ho, Wo;
  int nby, nbx, splits;
  long long nbricks;
};

template <int K, int S>
__global__ __launch_bounds__(FW_THREADS) void conv2d_fewin_wgrad_kernel(FwArgs a) {
  constexpr int P = K / 2;
  constexpr int IY = (FW_TY - 1) * S + K, IX = (FW_TX - 1) * S + K;
  constexpr int IXP = IX | 1;                                    // odd row stride
  __shared__ float xs[FW_MAX_CIN * IY * IXP];
  __shared__ __attribute__((aligned(16))) float gs[FW_COB * FW_PIX];
  const int tid = threadIdx.x;
  const int co0 = blockIdx.x * FW_COB, split = blockIdx.y;
  const int ntaps = a.Cin * K * K;
  const bool owner = tid < ntaps;
  const int t = owner ? tid : 0;                                 // idle threads gather tap 0 and write nothing
  const int ci = t / (K * K), ky = (t % (K * K)) / K, kx = t % K;
  const float* xrd = xs + (ci * IY + ky) * IXP + kx;

  float acc[FW_COB];
#pragma unroll
  for (int n = 0; n < FW_COB; ++n) acc[n] = 0.f;

  long long b0, b1;
  dv_split_range(a.nbricks, split, a.splits, b0, b1);
  const size_t xplane = (size_t)a.H * a.W, gplane = (size_t)a.Ho * a.Wo;
  for (long long br = b0; br < b1; ++br) {
    int b, by, bx;
    dv_brick_decode2(br, a.nby, a.nbx, b, by, bx);
    const int oy0 = by * FW_TY, ox0 = bx * FW_TX;
    __syncthreads();                                             // the previous brick's reads are done
    for (int i = tid; i < a.Cin * IY * IX; i += FW_THREADS) {
      const int xx = i % IX, yy = (i / IX) % IY, c = i / (IX * IY);
      const int yi = oy0 * S - P + yy, xi = ox0 * S - P + xx;
      float v = 0.f;
      if ((unsigned)yi < (unsigned)a.H && (unsigned)xi < (unsigned)a.W)
        v = a.x[((size_t)b * a.Cin + c) * xplane + (size_t)yi * a.W + xi];
      xs[(c * IY + yy) * IXP + xx] = v;
    }
    for (int i = tid; i < FW_COB * FW_PIX; i += FW_THREADS) {
      const int px = i % FW_TX, py = (i / FW_TX) % FW_TY, c = i / FW_PIX;
      const int co = co0 + c, y = oy0 + py, xo = ox0 + px;
      float v = 0.f;
      if (co < a.Cout && y < a.Ho && xo < a.Wo) v = a.g[((size_t)b * a.Cout + co) * gplane + (size_t)y * a.Wo + xo];
      gs[i] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int py = 0; py < FW_TY; ++py) {
#pragma unroll
      for (int p4 = 0; p4 < FW_TX / 4; ++p4) {
        float xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = xrd[py * S * IXP + (p4 * 4 + j) * S];
#pragma unroll
        for (int n = 0; n < FW_COB; ++n) {
          const float4 gv = *reinterpret_cast<const float4*>(gs + n * FW_PIX + py * FW_TX + p4 * 4);
          acc[n] = fmaf(xv[0], gv.x, acc[n]);
          acc[n] = fmaf(xv[1], gv.y, acc[n]);
          acc[n] = fmaf(xv[2], gv.z, acc[n]);
          acc[n] = fmaf(xv[3], gv.w, acc[n]);
        }
      }
    }
  }
  if (!owner) return;
  float* out = a.ws + (size_t)split * a.Cout * ntaps;
#pragma unroll
  for (int n = 0; n < FW_COB; ++n)
    if (co0 + n < a.Cout) out[(size_t)(co0 + n) * ntaps + t] = acc[n];
}

struct FwPlan {
  int Ho, Wo, cogroups, nby, nbx, splits;
  long long nbricks;
};

bool fw_valid(int B, int Cin, int H, int W, int Cout, int k, int stride) {
  return B > 0 && Cin > 0 && Cin <= FW_MAX_CIN && H > 0 && W > 0 && Cout > 0 && (k == 3 || k == 5 || k == 7) &&
         (stride == 1 || stride == 2) && (long long)H * W < (1ll << 28) && (long long)B * H * W < (1ll << 40) &&
         (long long)Cout * Cin * k * k <= DV_WGRAD_MAX_WS_FLOATS && (Cout + FW_COB - 1) / FW_COB <= 65535;
}

FwPlan fw_plan(int B, int Cin, int H, int W, int Cout, int k, int stride) {
  FwPlan p;
  p.Ho = (H - 1) / stride + 1;                                   // padding k/2
  p.Wo = (W - 1) / stride + 1;
  p.cogroups = (Cout + FW_COB - 1) / FW_COB;
  p.nby = (p.Ho + FW_TY - 1) / FW_TY;
  p.nbx = (p.Wo + FW_TX - 1) / FW_TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  // at least two bricks per split; the split index is grid.y
  p.splits = dv_wgrad_splits((FW_TARGET_BLOCKS + p.cogroups - 1) / p.cogroups, (long long)Cout * Cin * k * k, p.nbricks, 2,
                             true);
  return p;
}

}  // namespace

extern "C" int dv_instance_norm_act_bwd_f32(const float* x, const float* g, float* dx, int BC, int HW, float eps, int act,
                                            dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dx);
  DV_REQUIRE(BC > 0 && HW > 0, DV_ERR_SHAPE);
  DV_REQUIRE(act == DV_ACT_NONE || act == DV_ACT_RELU || act == DV_ACT_LEAKY, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(dx != x && dx != g, DV_ERR_UNSUPPORTED);            // out of place: every pass re-reads x and g
  const bool vec = HW % 4 == 0 && dv_aligned16(x) && dv_aligned16(g) && dv_aligned16(dx);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(instance_norm_act_bwd_kernel<true>, dim3((unsigned)BC), dim3(1024), 0, s, x, g, dx, HW, eps, act);
  else
    hipLaunchKernelGGL(instance_norm_act_bwd_kernel<false>, dim3((unsigned)BC), dim3(1024), 0, s, x, g, dx, HW, eps, act);
  return dv_launch_status();
}

extern "C" size_t dv_conv2d_fewin_wgrad_workspace_floats(int B, int Cin, int H, int W, int Cout, int k, int stride) {
  if (!fw_valid(B, Cin, H, W, Cout, k, stride)) return 0;
  return (size_t)fw_plan(B, Cin, H, W, Cout, k, stride).splits * Cout * Cin * k * k;
}

extern "C" int dv_conv2d_fewin_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int H,
                                         int W, int Cout, int k, int stride, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(B > 0 && Cin > 0 && H > 0 && W > 0 && Cout > 0, DV_ERR_SHAPE);
  DV_REQUIRE(Cin <= FW_MAX_CIN && (k == 3 || k == 5 || k == 7) && (stride == 1 || stride == 2), DV_ERR_UNSUPPORTED);
  DV_REQUIRE(fw_valid(B, Cin, H, W, Cout, k, stride), DV_ERR_SHAPE);
  const FwPlan p = fw_plan(B, Cin, H, W, Cout, k, stride);
  FwArgs a;
  a.x = x; a.g = g; a.ws = workspace;
  a.B = B; a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.Ho = p.Ho; a.Wo = p.Wo;
  a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  const dim3 grid((unsigned)p.cogroups, (unsigned)p.splits), block(FW_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define DV_FW(K, S) hipLaunchKernelGGL((conv2d_fewin_wgrad_kernel<K, S>), grid, block, 0, s, a)
  if (k == 3 && stride == 1) DV_FW(3, 1);
  else if (k == 3) DV_FW(3, 2);
  else if (k == 5 && stride == 1) DV_FW(5, 1);
  else if (k == 5) DV_FW(5, 2);
  else if (stride == 1) DV_FW(7, 1);
  else DV_FW(7, 2);
#undef DV_FW
  return dv_splitk_finish(workspace, dw, (long long)Cout * Cin * k * k, p.splits, s, true);
}
