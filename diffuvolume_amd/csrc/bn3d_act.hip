// BatchNorm3d with batch statistics + optional skip add + activation, forward and backward, for the training routes of
// the ACV and PCW aggregation stacks (include/diffuvolume_hip_volume_train.h, `dv_bn3d_*`).
//
//   x [B,C,S] (S = D*H*W), per-channel statistics over the B*S elements of a channel
//   y = act((x - mean) * invstd * gamma + beta + skip)
//
// Everything is plain fp32 VALU and bound by memory.  One block owns one chunk of BN_CHUNK consecutive floats of one
// (b,c) slab, in every kernel: the statistics kernel and pass 1 of the backward leave one partial per block in the caller's
// workspace, and a small combine launch (one wave per channel) merges a channel's partials in a fixed order with a double
// accumulator.  No atomics and no "last block finishes": the same call gives the same bits on every launch.
//
// The 16-byte kernels (S % 4 == 0, every tensor operand on a 16-byte line) and the scalar ones visit the elements of a
// chunk in the same thread / order assignment -- thread t takes floats 4*(t + 256*j) .. +3 in both -- so the two paths give
// the same bits, not only the same values within rounding.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int BN_THREADS = 256;
constexpr int BN_CHUNK = 8192;                 // floats of one (b,c) slab per block: 8 quads per thread

struct BnGeo {
  int nchunk;          // chunks per (b,c) slab
  int P;               // partials per channel = B * nchunk
  long long blocks;    // C * P
};

BnGeo bn_geo(int B, int C, int S) {
  BnGeo g;
  g.nchunk = (int)(((long long)S + BN_CHUNK - 1) / BN_CHUNK);
  const long long P = (long long)B * g.nchunk;
  g.P = (int)(P <= 0x7fffffffll ? P : 0);
  g.blocks = P * C;
  return g;
}

bool bn_valid(int B, int C, int S) {
  if (B <= 0 || C <= 0 || S <= 0) return false;
  const BnGeo g = bn_geo(B, C, S);
  return g.P > 0 && g.blocks <= 0x7fffffffll;
}

// Where a block works: channel c, partial p = b * nchunk + k, the chunk's first float and its length.
struct BnBlock {
  int c, p, n;
  size_t base;
};

__device__ __forceinline__ BnBlock bn_block(int B, int C, int S, int nchunk) {
  const unsigned bid = blockIdx.x;
  const unsigned P = (unsigned)B * (unsigned)nchunk;
  BnBlock q;
  q.c = (int)(bid / P);
  q.p = (int)(bid - (unsigned)q.c * P);
  const int b = q.p / nchunk, k = q.p - b * nchunk;
  const int first = k * BN_CHUNK;
  q.n = S - first < BN_CHUNK ? S - first : BN_CHUNK;
  q.base = ((size_t)b * C + q.c) * (size_t)S + (size_t)first;
  return q;
}

struct BnCh {
  float mean, invstd, gamma, beta;
};

// z and xhat of one element; the forward and the backward share this statement, so the backward recomputes the forward's z
// bit for bit.
__device__ __forceinline__ float bn_z(float x, float sk, const BnCh& p, float& xhat) {
  xhat = (x - p.mean) * p.invstd;
  return fmaf(xhat, p.gamma, p.beta) + sk;
}

template <int ACT>
__device__ __forceinline__ float bn_act_grad(float z) {
  if (ACT == DV_ACT_RELU) return z > 0.0f ? 1.0f : 0.0f;
  if (ACT == DV_ACT_MISH) {
    // dv_act's e and n: mish = z t, t = n / (n + 2);  t' = (1 - t^2) e / (1 + e), and 1 - t = 2 / (n + 2) has no
    // cancellation, so 1 - t^2 = (1 - t)(1 + t) is formed from it.
    if (z > 20.0f) return 1.0f;
    const float e = expf(z);
    const float n = e * (e + 2.0f);
    const float t = n / (n + 2.0f);
    const float w = 2.0f / (n + 2.0f);
    return fmaf(z * (w * (1.0f + t)), e / (1.0f + e), t);
  }
  return 1.0f;
}

// Sum of a and of b over the block, in a fixed order: lanes by halving shuffles, then the four waves in ascending order.
// The result is valid in thread 0.
__device__ __forceinline__ void bn_block_sum2(float& a, float& b) {
  __shared__ float red[2][BN_THREADS / DV_WAVE];
#pragma unroll
  for (int off = DV_WAVE / 2; off > 0; off >>= 1) {
    a += __shfl_down(a, off, DV_WAVE);
    b += __shfl_down(b, off, DV_WAVE);
  }
  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  if (lane == 0) {
    red[0][wave] = a;
    red[1][wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    a = red[0][0];
    b = red[1][0];
#pragma unroll
    for (int w = 1; w < BN_THREADS / DV_WAVE; ++w) {
      a += red[0][w];
      b += red[1][w];
    }
  }
}

// The quad at offset i of a chunk of n floats.  VEC: n % 4 == 0 and the chunk starts on a 16-byte line, one 16-byte access;
// otherwise four scalar ones, and floats past the chunk's end read as 0 and are not written.
template <bool VEC>
__device__ __forceinline__ void bn_load4(const float* __restrict__ p, int i, int n, float v[4]) {
  if (VEC) {
    const float4 q = *reinterpret_cast<const float4*>(p + i);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < n ? p[i + j] : 0.0f;
  }
}

template <bool VEC>
__device__ __forceinline__ void bn_store4(float* p, int i, int n, const float v[4]) {
  if (VEC) {
    *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (i + j < n) p[i + j] = v[j];
  }
}

// ---- statistics ------------------------------------------------------------------------------------------------------
// One partial (count, mean, M2) per block in the shifted form: with K the chunk's first element, s1 = sum (x - K) and
// s2 = sum (x - K)^2 stay of the size of the spread however large the mean is; mean = K + s1 / n, M2 = s2 - s1^2 / n.
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn3d_stats_kernel(const float* __restrict__ x, float* __restrict__ ws,
                                                                int B, int C, int S, int nchunk) {
  const BnBlock q = bn_block(B, C, S, nchunk);
  const float* xs = x + q.base;
  const float K = xs[0];
  float s1 = 0.0f, s2 = 0.0f;
  for (int i = 4 * threadIdx.x; i < q.n; i += 4 * BN_THREADS) {
    float v[4];
    bn_load4<VEC>(xs, i, q.n, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = (VEC || i + j < q.n) ? v[j] - K : 0.0f;
      s1 += d;
      s2 = fmaf(d, d, s2);
    }
  }
  bn_block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    const float n = (float)q.n;
    const float m = s1 / n;
    float* o = ws + ((size_t)q.c * (B * nchunk) + q.p) * 3;
    o[0] = n;
    o[1] = K + m;
    o[2] = fmaxf(fmaf(-s1, m, s2), 0.0f);
  }
}

// Chan's merge of (nb, mb, Mb) into (na, ma, Ma); an empty side leaves the other as it is.
__device__ __forceinline__ void bn_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (na == 0.0) {
    na = nb; ma = mb; Ma = Mb;
    return;
  }
  const double n = na + nb, d = mb - ma;
  ma += d * (nb / n);
  Ma += Mb + d * d * (na * nb / n);
  na = n;
}

// One wave per channel: lane l merges partials l, l + 64, ... in ascending order, then the lanes merge by halving.
__global__ __launch_bounds__(DV_WAVE) void bn3d_stats_combine_kernel(const float* __restrict__ ws, float* __restrict__ mean,
                                                                     float* __restrict__ invstd, float* running_mean,
                                                                     float* running_var, int P, float momentum, float eps) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const float* w = ws + (size_t)c * P * 3;
  double n = 0.0, m = 0.0, M2 = 0.0;
  for (int p = lane; p < P; p += DV_WAVE) bn_merge(n, m, M2, (double)w[3 * p], (double)w[3 * p + 1], (double)w[3 * p + 2]);
#pragma unroll
  for (int off = DV_WAVE / 2; off > 0; off >>= 1) {
    const double nb = __shfl_down(n, off, DV_WAVE), mb = __shfl_down(m, off, DV_WAVE), Mb = __shfl_down(M2, off, DV_WAVE);
    bn_merge(n, m, M2, nb, mb, Mb);
  }
  if (lane == 0) {
    const double var = M2 / n;
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean != nullptr) {
      const double mo = (double)momentum;
      running_mean[c] = (float)((1.0 - mo) * (double)running_mean[c] + mo * m);
      running_var[c] = (float)((1.0 - mo) * (double)running_var[c] + mo * (M2 / (n - 1.0)));
    }
  }
}

// ---- apply -----------------------------------------------------------------------------------------------------------
template <bool VEC, int ACT>
__global__ __launch_bounds__(BN_THREADS) void bn3d_apply_kernel(const float* __restrict__ x, const float* __restrict__ skip,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, float* __restrict__ y, int B,
                                                                int C, int S, int nchunk) {
  const BnBlock q = bn_block(B, C, S, nchunk);
  const BnCh ch = {mean[q.c], invstd[q.c], gamma[q.c], beta[q.c]};
  const float* xs = x + q.base;
  const float* ss = skip != nullptr ? skip + q.base : nullptr;
  float* ys = y + q.base;
  for (int i = 4 * threadIdx.x; i < q.n; i += 4 * BN_THREADS) {
    float v[4], s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4];
    bn_load4<VEC>(xs, i, q.n, v);
    if (ss != nullptr) bn_load4<VEC>(ss, i, q.n, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xhat;
      o[j] = dv_act(bn_z(v[j], s[j], ch, xhat), ACT);
    }
    bn_store4<VEC>(ys, i, q.n, o);
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
// Pass 1: dz = dy act'(z) into `dz` (NULL: not stored) and the block's sums of dz and dz xhat into the workspace.
template <bool VEC, int ACT>
__global__ __launch_bounds__(BN_THREADS) void bn3d_bwd_dz_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                 const float* __restrict__ skip,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ dz,
                                                                 float* __restrict__ ws, int B, int C, int S, int nchunk) {
  const BnBlock q = bn_block(B, C, S, nchunk);
  const BnCh ch = {mean[q.c], invstd[q.c], gamma[q.c], beta[q.c]};
  const float* gs = dy + q.base;
  const float* xs = x + q.base;
  const float* ss = skip != nullptr ? skip + q.base : nullptr;
  float* zs = dz != nullptr ? dz + q.base : nullptr;
  float s1 = 0.0f, s2 = 0.0f;
  for (int i = 4 * threadIdx.x; i < q.n; i += 4 * BN_THREADS) {
    float g[4], v[4], s[4] = {0.0f, 0.0f, 0.0f, 0.0f}, o[4];
    bn_load4<VEC>(gs, i, q.n, g);
    bn_load4<VEC>(xs, i, q.n, v);
    if (ss != nullptr) bn_load4<VEC>(ss, i, q.n, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xhat;
      const float z = bn_z(v[j], s[j], ch, xhat);
      const float d = (VEC || i + j < q.n) ? g[j] * bn_act_grad<ACT>(z) : 0.0f;
      o[j] = d;
      s1 += d;
      s2 = fmaf(d, xhat, s2);
    }
    if (zs != nullptr) bn_store4<VEC>(zs, i, q.n, o);
  }
  bn_block_sum2(s1, s2);
  if (threadIdx.x == 0) {
    float* o = ws + ((size_t)q.c * (B * nchunk) + q.p) * 2;
    o[0] = s1;
    o[1] = s2;
  }
}

// One wave per channel: the partial sums in a fixed order in double -> dbeta, dgamma and the two means pass 2 subtracts.
__global__ __launch_bounds__(DV_WAVE) void bn3d_bwd_combine_kernel(const float* __restrict__ ws, float* __restrict__ sums,
                                                                   float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                   int P, double count) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const float* w = ws + (size_t)c * P * 2;
  double a = 0.0, b = 0.0;
  for (int p = lane; p < P; p += DV_WAVE) {
    a += (double)w[2 * p];
    b += (double)w[2 * p + 1];
  }
#pragma unroll
  for (int off = DV_WAVE / 2; off > 0; off >>= 1) {
    a += __shfl_down(a, off, DV_WAVE);
    b += __shfl_down(b, off, DV_WAVE);
  }
  if (lane == 0) {
    sums[2 * c] = (float)(a / count);
    sums[2 * c + 1] = (float)(b / count);
    if (dbeta != nullptr) dbeta[c] = (float)a;
    if (dgamma != nullptr) dgamma[c] = (float)b;
  }
}

// Pass 2: dx = gamma invstd (dz - mean(dz) - xhat mean(dz xhat)).  `dz` may be `dx` itself (in place over the scratch):
// every thread reads the quad it then writes, so neither is __restrict__.
template <bool VEC>
__global__ __launch_bounds__(BN_THREADS) void bn3d_bwd_dx_kernel(const float* dz, const float* __restrict__ x,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ sums, float* dx, int B, int C,
                                                                 int S, int nchunk) {
  const BnBlock q = bn_block(B, C, S, nchunk);
  const float mu = mean[q.c], is = invstd[q.c], scale = gamma[q.c] * is;
  const float m1 = sums[2 * q.c], m2 = sums[2 * q.c + 1];
  const float* zs = dz + q.base;
  const float* xs = x + q.base;
  float* os = dx + q.base;
  for (int i = 4 * threadIdx.x; i < q.n; i += 4 * BN_THREADS) {
    float d[4], v[4], o[4];
    bn_load4<VEC>(zs, i, q.n, d);
    bn_load4<VEC>(xs, i, q.n, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float xhat = (v[j] - mu) * is;
      o[j] = scale * ((d[j] - m1) - xhat * m2);
    }
    bn_store4<VEC>(os, i, q.n, o);
  }
}

template <bool VEC>
void launch_apply(int act, dim3 grid, hipStream_t s, const float* x, const float* skip, const float* mean,
                  const float* invstd, const float* gamma, const float* beta, float* y, int B, int C, int S, int nchunk) {
  const dim3 blk(BN_THREADS);
  if (act == DV_ACT_RELU)
    hipLaunchKernelGGL((bn3d_apply_kernel<VEC, DV_ACT_RELU>), grid, blk, 0, s, x, skip, mean, invstd, gamma, beta, y, B, C, S,
                       nchunk);
  else if (act == DV_ACT_MISH)
    hipLaunchKernelGGL((bn3d_apply_kernel<VEC, DV_ACT_MISH>), grid, blk, 0, s, x, skip, mean, invstd, gamma, beta, y, B, C, S,
                       nchunk);
  else
    hipLaunchKernelGGL((bn3d_apply_kernel<VEC, DV_ACT_NONE>), grid, blk, 0, s, x, skip, mean, invstd, gamma, beta, y, B, C, S,
                       nchunk);
}

template <bool VEC>
void launch_dz(int act, dim3 grid, hipStream_t s, const float* dy, const float* x, const float* skip, const float* mean,
               const float* invstd, const float* gamma, const float* beta, float* dz, float* ws, int B, int C, int S,
               int nchunk) {
  const dim3 blk(BN_THREADS);
  if (act == DV_ACT_RELU)
    hipLaunchKernelGGL((bn3d_bwd_dz_kernel<VEC, DV_ACT_RELU>), grid, blk, 0, s, dy, x, skip, mean, invstd, gamma, beta, dz, ws,
                       B, C, S, nchunk);
  else if (act == DV_ACT_MISH)
    hipLaunchKernelGGL((bn3d_bwd_dz_kernel<VEC, DV_ACT_MISH>), grid, blk, 0, s, dy, x, skip, mean, invstd, gamma, beta, dz, ws,
                       B, C, S, nchunk);
  else
    hipLaunchKernelGGL((bn3d_bwd_dz_kernel<VEC, DV_ACT_NONE>), grid, blk, 0, s, dy, x, skip, mean, invstd, gamma, beta, dz, ws,
                       B, C, S, nchunk);
}

bool bn_act_ok(int act) { return act == DV_ACT_NONE || act == DV_ACT_RELU || act == DV_ACT_MISH; }

}  // namespace

extern "C" size_t dv_bn3d_train_workspace_floats(int B, int C, int S) {
  if (!bn_valid(B, C, S)) return 0;
  const BnGeo g = bn_geo(B, C, S);
  return (size_t)C * (3 * (size_t)g.P + 2);
}

extern "C" int dv_bn3d_stats_f32(const float* x, float* mean, float* invstd, float* running_mean, float* running_var,
                                 float* workspace, int B, int C, int S, float momentum, float eps, dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(mean);
  DV_REQUIRE_PTR(invstd);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE((running_mean == nullptr) == (running_var == nullptr), DV_ERR_NULL);
  DV_REQUIRE(bn_valid(B, C, S), DV_ERR_SHAPE);
  DV_REQUIRE((long long)B * S > 1, DV_ERR_UNSUPPORTED);        // one value per channel has no variance
  DV_REQUIRE(eps >= 0.0f, DV_ERR_SHAPE);
  const BnGeo g = bn_geo(B, C, S);
  const bool vec = S % 4 == 0 && dv_aligned16(x);
  const dim3 grid((unsigned)g.blocks), blk(BN_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL(bn3d_stats_kernel<true>, grid, blk, 0, s, x, workspace, B, C, S, g.nchunk);
  else
    hipLaunchKernelGGL(bn3d_stats_kernel<false>, grid, blk, 0, s, x, workspace, B, C, S, g.nchunk);
  const int rc = dv_launch_status();
  if (rc != DV_OK) return rc;
  hipLaunchKernelGGL(bn3d_stats_combine_kernel, dim3((unsigned)C), dim3(DV_WAVE), 0, s, workspace, mean, invstd, running_mean,
                     running_var, g.P, momentum, eps);
  return dv_launch_status();
}

extern "C" int dv_bn3d_apply_act_f32(const float* x, const float* skip, const float* mean, const float* invstd,
                                     const float* gamma, const float* beta, float* y, int B, int C, int S, int act,
                                     dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(mean);
  DV_REQUIRE_PTR(invstd);
  DV_REQUIRE_PTR(gamma);
  DV_REQUIRE_PTR(beta);
  DV_REQUIRE_PTR(y);
  DV_REQUIRE(bn_valid(B, C, S), DV_ERR_SHAPE);
  DV_REQUIRE(bn_act_ok(act), DV_ERR_UNSUPPORTED);
  const BnGeo g = bn_geo(B, C, S);
  const bool vec = S % 4 == 0 && dv_aligned16(x) && dv_aligned16(y) && (skip == nullptr || dv_aligned16(skip));
  const dim3 grid((unsigned)g.blocks);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    launch_apply<true>(act, grid, s, x, skip, mean, invstd, gamma, beta, y, B, C, S, g.nchunk);
  else
    launch_apply<false>(act, grid, s, x, skip, mean, invstd, gamma, beta, y, B, C, S, g.nchunk);
  return dv_launch_status();
}

extern "C" int dv_bn3d_act_bwd_f32(const float* dy, const float* x, const float* skip, const float* mean,
                                   const float* invstd, const float* gamma, const float* beta, float* dx, float* dskip,
                                   float* dgamma, float* dbeta, float* workspace, int B, int C, int S, int act,
                                   dv_stream_t stream) {
  DV_REQUIRE_PTR(dy);
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(mean);
  DV_REQUIRE_PTR(invstd);
  DV_REQUIRE_PTR(gamma);
  DV_REQUIRE_PTR(beta);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(dx != nullptr || dskip != nullptr || dgamma != nullptr || dbeta != nullptr, DV_ERR_NULL);
  DV_REQUIRE(dskip == nullptr || skip != nullptr, DV_ERR_NULL);
  DV_REQUIRE(bn_valid(B, C, S), DV_ERR_SHAPE);
  DV_REQUIRE((long long)B * S > 1, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(bn_act_ok(act), DV_ERR_UNSUPPORTED);
  const BnGeo g = bn_geo(B, C, S);
  // dz = dy when nothing stands between the normalisation and the output: no store in pass 1, pass 2 reads dy
  const bool plain = act == DV_ACT_NONE && skip == nullptr;
  float* dz = dskip != nullptr ? dskip : (plain ? nullptr : dx);
  const bool vec = S % 4 == 0 && dv_aligned16(dy) && dv_aligned16(x) && (skip == nullptr || dv_aligned16(skip)) &&
                   (dx == nullptr || dv_aligned16(dx)) && (dskip == nullptr || dv_aligned16(dskip));
  float* sums = workspace + (size_t)C * 3 * (size_t)g.P;
  const dim3 grid((unsigned)g.blocks);
  hipStream_t s = (hipStream_t)stream;
  if (vec)
    launch_dz<true>(act, grid, s, dy, x, skip, mean, invstd, gamma, beta, dz, workspace, B, C, S, g.nchunk);
  else
    launch_dz<false>(act, grid, s, dy, x, skip, mean, invstd, gamma, beta, dz, workspace, B, C, S, g.nchunk);
  int rc = dv_launch_status();
  if (rc != DV_OK) return rc;
  hipLaunchKernelGGL(bn3d_bwd_combine_kernel, dim3((unsigned)C), dim3(DV_WAVE), 0, s, workspace, sums, dgamma, dbeta, g.P,
                     (double)B * (double)S);
  rc = dv_launch_status();
  if (rc != DV_OK || dx == nullptr) return rc;
  const float* src = dz != nullptr ? dz : dy;
  if (vec)
    hipLaunchKernelGGL(bn3d_bwd_dx_kernel<true>, grid, dim3(BN_THREADS), 0, s, src, x, mean, invstd, gamma, sums, dx, B, C, S,
                       g.nchunk);
  else
    hipLaunchKernelGGL(bn3d_bwd_dx_kernel<false>, grid, dim3(BN_THREADS), 0, s, src, x, mean, invstd, gamma, sums, dx, B, C, S,
                       g.nchunk);
  return dv_launch_status();
}
