// FeatureAtt's volume gate (KITTI15/core/submodule.py:234-239): cv[b,c,d,y,x] *= sigmoid(logit[b,c,y,x]).
// The 2-D logits come from the image-feature branch (two 1x1 Conv2d, PyTorch side); the broadcast over
// the disparity axis is the HBM-bound part: one read + one write of the volume, the [C,H,W] logit plane
// stays in L2 across the D slices a block walks.
#include "dv_common.h"

namespace {

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + expf(-v)); }

// grid: (plane chunks, D split, B*C); each thread owns VEC consecutive x of one (y,x) position and walks d.
template <int VEC>
__global__ __launch_bounds__(256) void feature_gate_kernel(const float* __restrict__ cv,
                                                           const float* __restrict__ logit,
                                                           float* __restrict__ out, int D, int HW) {
  const int bc = blockIdx.z;
  const int i = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (i >= HW) return;
  const float* lp = logit + (size_t)bc * HW + i;
  float g[VEC];
  if (VEC == 4) {
    const float4 l = *reinterpret_cast<const float4*>(lp);
    g[0] = sigmoidf_(l.x); g[1 % VEC] = sigmoidf_(l.y); g[2 % VEC] = sigmoidf_(l.z); g[3 % VEC] = sigmoidf_(l.w);
  } else {
    g[0] = sigmoidf_(lp[0]);
  }
  const size_t base = (size_t)bc * D * HW + i;
  for (int d = blockIdx.y; d < D; d += gridDim.y) {
    const size_t o = base + (size_t)d * HW;
    if (VEC == 4) {
      float4 v = *reinterpret_cast<const float4*>(cv + o);
      v.x *= g[0]; v.y *= g[1 % VEC]; v.z *= g[2 % VEC]; v.w *= g[3 % VEC];
      *reinterpret_cast<float4*>(out + o) = v;
    } else {
      out[o] = cv[o] * g[0];
    }
  }
}

// Backward of the gate: dcv = g * sigmoid(logit), dlogit = s (1 - s) * sum_d g * cv with s = sigmoid(logit) recomputed.
// Same grid as the forward; a thread owns VEC positions of one (b, c) plane and walks a contiguous d range in ascending
// order, reading g and cv once each.  gridDim.y == 1: the thread finishes dlogit itself.  Otherwise (a plane too small to
// fill the chip) it writes its partial sum to part[split][b*c][HW] and feature_gate_bwd_reduce_kernel adds the partials in
// split order: no atomics, the same bits on every launch.
template <int VEC>
__global__ __launch_bounds__(256) void feature_gate_bwd_kernel(const float* __restrict__ cv,
                                                               const float* __restrict__ logit,
                                                               const float* __restrict__ g, float* __restrict__ dcv,
                                                               float* __restrict__ dlogit, float* __restrict__ part,
                                                               int D, int HW, int per_split) {
  const int bc = blockIdx.z;
  const int i = (blockIdx.x * 256 + threadIdx.x) * VEC;
  if (i >= HW) return;
  const float* lp = logit + (size_t)bc * HW + i;
  float s[VEC], sum[VEC];
  if (VEC == 4) {
    const float4 l = *reinterpret_cast<const float4*>(lp);
    s[0] = sigmoidf_(l.x); s[1 % VEC] = sigmoidf_(l.y); s[2 % VEC] = sigmoidf_(l.z); s[3 % VEC] = sigmoidf_(l.w);
  } else {
    s[0] = sigmoidf_(lp[0]);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) sum[v] = 0.f;
  const size_t base = (size_t)bc * D * HW + i;
  const int d0 = blockIdx.y * per_split, d1 = d0 + per_split < D ? d0 + per_split : D;
  for (int d = d0; d < d1; ++d) {
    const size_t o = base + (size_t)d * HW;
    if (VEC == 4) {
      const float4 gv = *reinterpret_cast<const float4*>(g + o);
      const float4 c = *reinterpret_cast<const float4*>(cv + o);
      *reinterpret_cast<float4*>(dcv + o) = make_float4(gv.x * s[0], gv.y * s[1 % VEC], gv.z * s[2 % VEC], gv.w * s[3 % VEC]);
      sum[0] = fmaf(gv.x, c.x, sum[0]); sum[1 % VEC] = fmaf(gv.y, c.y, sum[1 % VEC]);
      sum[2 % VEC] = fmaf(gv.z, c.z, sum[2 % VEC]); sum[3 % VEC] = fmaf(gv.w, c.w, sum[3 % VEC]);
    } else {
      const float gv = g[o];
      dcv[o] = gv * s[0];
      sum[0] = fmaf(gv, cv[o], sum[0]);
    }
  }
  const bool last = gridDim.y == 1;
  float* o = last ? dlogit + (size_t)bc * HW + i : part + ((size_t)blockIdx.y * gridDim.z + bc) * HW + i;
#pragma unroll
  for (int v = 0; v < VEC; ++v) o[v] = last ? s[v] * (1.f - s[v]) * sum[v] : sum[v];
}

// dlogit[e] = s (1 - s) * (part[0][e] + part[1][e] + ...), in split order
__global__ __launch_bounds__(256) void feature_gate_bwd_reduce_kernel(const float* __restrict__ part,
                                                                      const float* __restrict__ logit,
                                                                      float* __restrict__ dlogit, long long n, int splits) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += stride) {
    float sum = part[e];
    for (int k = 1; k < splits; ++k) sum += part[(size_t)k * n + e];
    const float s = sigmoidf_(logit[e]);
    dlogit[e] = s * (1.f - s) * sum;
  }
}

struct GateBwdPlan {
  int gx, splits, per_split;
};

// D is split only when the plane alone cannot fill the chip, and never into ranges shorter than 4 slices
GateBwdPlan gate_bwd_plan(int B, int C, int D, int HW) {
  GateBwdPlan p;
  const int per = HW % 4 == 0 ? 1024 : 256;
  p.gx = (HW + per - 1) / per;
  const int most = (D + 3) / 4;
  int gy = 1;
  while (gy < most && (long long)p.gx * gy * B * C < 2048) gy *= 2;
  if (gy > most) gy = most;
  p.per_split = (D + gy - 1) / gy;
  p.splits = (D + p.per_split - 1) / p.per_split;
  return p;
}

}  // namespace

extern "C" size_t dv_feature_gate_bwd_workspace_floats(int B, int C, int D, int H, int W) {
  if (B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  const GateBwdPlan p = gate_bwd_plan(B, C, D, H * W);
  return p.splits > 1 ? (size_t)p.splits * B * C * H * W : 0;
}

extern "C" int dv_feature_gate_bwd_f32(const float* cv, const float* logit, const float* g, float* dcv, float* dlogit,
                                       float* workspace, int B, int C, int D, int H, int W, dv_stream_t stream) {
  DV_REQUIRE_PTR(cv);
  DV_REQUIRE_PTR(logit);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dcv);
  DV_REQUIRE_PTR(dlogit);
  DV_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE((long long)B * C <= 65535, DV_ERR_SHAPE);
  const int HW = H * W;
  const GateBwdPlan p = gate_bwd_plan(B, C, D, HW);
  if (p.splits > 1) DV_REQUIRE_PTR(workspace);
  const bool vec = (HW % 4 == 0) && dv_aligned16(cv) && dv_aligned16(logit) && dv_aligned16(g) && dv_aligned16(dcv) &&
                   dv_aligned16(dlogit) && (p.splits == 1 || dv_aligned16(workspace));
  const int gx = vec ? p.gx : (HW + 255) / 256;
  const dim3 grid((unsigned)gx, (unsigned)p.splits, (unsigned)(B * C));
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((feature_gate_bwd_kernel<4>), grid, dim3(256), 0, s, cv, logit, g, dcv, dlogit, workspace, D, HW,
                       p.per_split);
  else
    hipLaunchKernelGGL((feature_gate_bwd_kernel<1>), grid, dim3(256), 0, s, cv, logit, g, dcv, dlogit, workspace, D, HW,
                       p.per_split);
  int rc = dv_launch_status();
  if (rc != DV_OK || p.splits == 1) return rc;
  const long long n = (long long)B * C * HW;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(feature_gate_bwd_reduce_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, s, workspace,
                     logit, dlogit, n, p.splits);
  return dv_launch_status();
}

extern "C" int dv_feature_gate_f32(const float* cv, const float* logit, float* out, int B, int C, int D,
                                   int H, int W, dv_stream_t stream) {
  DV_REQUIRE_PTR(cv);
  DV_REQUIRE_PTR(logit);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE((long long)B * C <= 65535, DV_ERR_SHAPE);
  const int HW = H * W;
  const bool vec = (HW % 4 == 0) && dv_aligned16(cv) && dv_aligned16(out) && dv_aligned16(logit);
  const int per = vec ? 1024 : 256;
  const int gx = (HW + per - 1) / per;
  int gy = 1;                                   // split D only when the plane alone cannot fill the chip
  while (gy < D && (long long)gx * gy * B * C < 2048) gy *= 2;
  if (gy > D) gy = D;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)(B * C));
  if (vec)
    hipLaunchKernelGGL((feature_gate_kernel<4>), grid, dim3(256), 0, (hipStream_t)stream, cv, logit, out, D, HW);
  else
    hipLaunchKernelGGL((feature_gate_kernel<1>), grid, dim3(256), 0, (hipStream_t)stream, cv, logit, out, D, HW);
  return dv_launch_status();
}
