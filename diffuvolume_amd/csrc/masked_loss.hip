// The masked training losses, forward and backward, for all K predictions of a step at once:
//
//   loss = sum_k w_k * mean_{i selected} g_k(pred_k[i] - gt[i]),   g = |d| (L1) or smooth-L1 with beta 1
//
// (SceneFlow/models/loss.py, KITTI12/models/loss.py, KITTI15/train_stereo.py:33-62).  The reference gathers est[mask] and
// gt[mask] per prediction: a nonzero with a host synchronisation, an int64 index tensor and two gathered copies kept for
// the backward, and an index_put there.  Here one grid-stride pass reads gt and the mask once for all K predictions and
// leaves per-block partial sums in double; a one-block launch merges them in a fixed order and writes the loss.  The
// backward is one launch that writes every element of every gradient once, zero at unselected pixels BY SELECTION (a NaN
// or Inf behind the mask never reaches a sum or a gradient).  No atomics: the same bits on every launch.
//
// Work unit: a quad of four consecutive elements, quad q to thread (q mod threads-of-the-grid), quads of a thread in
// ascending order.  A quad is read with 16-byte loads (its four mask bytes as one word) when every operand lies on such a
// line, element by element otherwise and at the tail; the assignment and the order of the additions are the same, so the
// two paths give the same bits.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int kMaxK = DV_MASKED_LOSS_MAX_K;
constexpr int kThreads = 256;
constexpr int kMaxBlocks = DV_MASKED_LOSS_MAX_BLOCKS;
constexpr int kExtra = 6;            // count, sum |d|, #(|d| < 1), #(|d| < 3), #(|d| < 5), #(selected gt infinite)

struct LossTable {
  const float* pred[kMaxK];
  float* grad[kMaxK];
  double w[kMaxK];
  int kind[kMaxK];
};

struct Quad {
  float v[4];
};

// four elements from element index i0 on; elements at or beyond n read as 0
__device__ __forceinline__ Quad load_quad(const float* __restrict__ p, long long i0, long long n, bool vec) {
  Quad q;
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p + i0);
    q.v[0] = t.x; q.v[1] = t.y; q.v[2] = t.z; q.v[3] = t.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) q.v[e] = i0 + e < n ? p[i0 + e] : 0.f;
  }
  return q;
}

// the selection of the four elements of a quad, bit e for element i0 + e
__device__ __forceinline__ unsigned select_quad(const void* __restrict__ mask, int mode, float max_disp, const Quad& g,
                                                long long i0, long long n, bool vec) {
  unsigned sel = 0;
  if (mode == DV_MASK_U8) {
    const unsigned char* __restrict__ m = static_cast<const unsigned char*>(mask);
    if (vec) {
      const unsigned word = *reinterpret_cast<const unsigned*>(m + i0);
#pragma unroll
      for (int e = 0; e < 4; ++e) sel |= ((word >> (8 * e)) & 0xffu) ? (1u << e) : 0u;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) sel |= (i0 + e < n && m[i0 + e]) ? (1u << e) : 0u;
    }
  } else {
    const Quad v = load_quad(static_cast<const float*>(mask), i0, n, vec);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      sel |= (i0 + e < n && v.v[e] >= 0.5f && sqrtf(g.v[e] * g.v[e]) < max_disp) ? (1u << e) : 0u;
  }
  return sel;
}

__device__ __forceinline__ float loss_term(float d, int kind) {
  const float a = fabsf(d);
  return kind == DV_LOSS_SMOOTH_L1 ? (a < 1.f ? 0.5f * d * d : a - 0.5f) : a;      // (NaN: a < 1 is false, a - 0.5 is NaN)
}

__device__ __forceinline__ float loss_slope(float d, int kind) {
  if (d != d) return d;
  const float s = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  return (kind == DV_LOSS_SMOOTH_L1 && fabsf(d) < 1.f) ? d : s;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, DV_WAVE);
  return v;
}

// partials [gridDim.x][K + kExtra] in double: K sums, then the kExtra figures above
template <int KT>
__global__ __launch_bounds__(kThreads) void masked_loss_fwd_kernel(LossTable t, const float* __restrict__ gt,
                                                                   const void* __restrict__ mask, int mode, float max_disp,
                                                                   int K, int metric_pred, long long n, int vec,
                                                                   double* __restrict__ partials) {
  __shared__ double red[kThreads / DV_WAVE][KT + kExtra];
  double acc[KT];
#pragma unroll
  for (int k = 0; k < KT; ++k) acc[k] = 0.0;
  double epe = 0.0;
  unsigned cnt = 0, c1 = 0, c3 = 0, c5 = 0, ninf = 0;

  const long long quads = (n + 3) >> 2;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
    const long long i0 = q << 2;
    const bool v = vec && i0 + 4 <= n;
    const Quad g = load_quad(gt, i0, n, v);
    const unsigned sel = select_quad(mask, mode, max_disp, g, i0, n, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (sel & (1u << e)) {
        ++cnt;
        if (isinf(g.v[e])) ++ninf;
      }
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < K) {
        const Quad p = load_quad(t.pred[k], i0, n, v);
        const int kind = t.kind[k];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = p.v[e] - g.v[e];
          acc[k] += (sel & (1u << e)) ? (double)loss_term(d, kind) : 0.0;
          if (k == metric_pred && (sel & (1u << e))) {
            const float a = fabsf(d);
            epe += (double)a;
            c1 += a < 1.f;
            c3 += a < 3.f;
            c5 += a < 5.f;
          }
        }
      }
    }
  }

  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  const double extra[kExtra] = {(double)cnt, epe, (double)c1, (double)c3, (double)c5, (double)ninf};
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    const double s = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = s;
  }
#pragma unroll
  for (int j = 0; j < kExtra; ++j) {
    const double s = wave_sum(extra[j]);
    if (lane == 0) red[wave][KT + j] = s;
  }
  __syncthreads();
  const int S = K + kExtra;
  if ((int)threadIdx.x < S) {
    const int j = (int)threadIdx.x < K ? threadIdx.x : KT + (threadIdx.x - K);
    partials[(size_t)blockIdx.x * S + threadIdx.x] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
  }
}

// One block.  Figure j is summed by one wave: lane l adds blocks l, l + 64, ... in ascending order, then the lanes are
// folded 32, 16, .., 1.  The order depends on the number of blocks only, i.e. on n.
__global__ __launch_bounds__(kThreads) void masked_loss_merge_kernel(const double* __restrict__ partials, int blocks, int K,
                                                                     LossTable t, double* __restrict__ stats,
                                                                     float* __restrict__ loss) {
  __shared__ double tot[kMaxK + kExtra];
  const int lane = threadIdx.x & (DV_WAVE - 1), wave = threadIdx.x / DV_WAVE;
  const int S = K + kExtra;
  for (int j = wave; j < S; j += kThreads / DV_WAVE) {
    double s = 0.0;
    for (int b = lane; b < blocks; b += DV_WAVE) s += partials[(size_t)b * S + j];
    s = wave_sum(s);
    if (lane == 0) tot[j] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double count = tot[K];
    double l = 0.0;
    for (int k = 0; k < K; ++k) {
      stats[k] = tot[k];
      l += t.w[k] * tot[k] / count;                       // count == 0: 0 / 0, the mean of an empty selection
    }
    for (int j = 0; j < kExtra - 1; ++j) stats[K + j] = tot[K + j];
    stats[K + kExtra - 1] = tot[K + kExtra - 1] > 0.0 ? 1.0 : 0.0;
    *loss = (float)l;
  }
}

__global__ __launch_bounds__(kThreads) void masked_loss_bwd_kernel(LossTable t, const float* __restrict__ gt,
                                                                   const void* __restrict__ mask, int mode, float max_disp,
                                                                   int K, long long n, int vec,
                                                                   const double* __restrict__ stats,
                                                                   const float* __restrict__ gout) {
  const double count = stats[K];
  const double inv = count > 0.0 ? (double)gout[0] / count : 0.0;
  const long long quads = (n + 3) >> 2;
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < quads; q += stride) {
    const long long i0 = q << 2;
    const bool v = vec && i0 + 4 <= n;
    const Quad g = load_quad(gt, i0, n, v);
    const unsigned sel = select_quad(mask, mode, max_disp, g, i0, n, v);
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      float* __restrict__ out = t.grad[k];
      if (out == nullptr) continue;
      const float scale = (float)(inv * t.w[k]);
      const int kind = t.kind[k];
      const Quad p = load_quad(t.pred[k], i0, n, v);
      float r[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (sel & (1u << e)) ? scale * loss_slope(p.v[e] - g.v[e], kind) : 0.f;
      if (v) {
        *reinterpret_cast<float4*>(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (i0 + e < n) out[i0 + e] = r[e];
      }
    }
  }
}

int blocks_for(long long n) {
  const long long quads = (n + 3) >> 2;
  const long long b = (quads + kThreads - 1) / kThreads;
  return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

// the checks the two launching entries share; fills the table
int fill_table(LossTable& t, const float* const* preds, float* const* dpreds, const double* weights, const int* kinds,
               const float* gt, const void* mask, int mask_mode, float max_disp, int K, long long n, bool* vec) {
  DV_REQUIRE_PTR(preds);
  DV_REQUIRE_PTR(weights);
  DV_REQUIRE_PTR(kinds);
  DV_REQUIRE_PTR(gt);
  DV_REQUIRE_PTR(mask);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  DV_REQUIRE(K >= 1 && K <= kMaxK, DV_ERR_SHAPE);
  DV_REQUIRE(mask_mode == DV_MASK_U8 || mask_mode == DV_MASK_VALID_F32, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(mask_mode == DV_MASK_U8 || max_disp == max_disp, DV_ERR_UNSUPPORTED);
  bool v = dv_aligned16(gt) && (mask_mode == DV_MASK_U8 ? (((uintptr_t)mask) & 3u) == 0 : dv_aligned16(mask));
  for (int k = 0; k < kMaxK; ++k) {
    t.pred[k] = nullptr;
    t.grad[k] = nullptr;
    t.w[k] = 0.0;
    t.kind[k] = 0;
  }
  for (int k = 0; k < K; ++k) {
    DV_REQUIRE_PTR(preds[k]);
    DV_REQUIRE(kinds[k] == DV_LOSS_L1 || kinds[k] == DV_LOSS_SMOOTH_L1, DV_ERR_UNSUPPORTED);
    t.pred[k] = preds[k];
    t.w[k] = weights[k];
    t.kind[k] = kinds[k];
    v = v && dv_aligned16(preds[k]);
    if (dpreds != nullptr && dpreds[k] != nullptr) {
      t.grad[k] = dpreds[k];
      v = v && dv_aligned16(dpreds[k]);
    }
  }
  *vec = v;
  return DV_OK;
}

template <int KT>
void launch_fwd(const LossTable& t, const float* gt, const void* mask, int mode, float max_disp, int K, int metric_pred,
                long long n, bool vec, double* partials, int blocks, hipStream_t s) {
  hipLaunchKernelGGL(masked_loss_fwd_kernel<KT>, dim3(blocks), dim3(kThreads), 0, s, t, gt, mask, mode, max_disp, K,
                     metric_pred, n, vec ? 1 : 0, partials);
}

}  // namespace

extern "C" size_t dv_masked_loss_workspace_floats(int K, long long n) {
  if (K < 1 || K > kMaxK || n <= 0) return 0;
  return (size_t)2 * blocks_for(n) * (K + kExtra);
}

extern "C" int dv_masked_loss_fwd_f32(const float* const* preds, const double* weights, const int* kinds, const float* gt,
                                      const void* mask, int mask_mode, float max_disp, int K, long long n, int metric_pred,
                                      float* workspace, double* stats, float* loss, dv_stream_t stream) {
  LossTable t;
  bool vec = false;
  const int rc = fill_table(t, preds, nullptr, weights, kinds, gt, mask, mask_mode, max_disp, K, n, &vec);
  if (rc != DV_OK) return rc;
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE_PTR(stats);
  DV_REQUIRE_PTR(loss);
  DV_REQUIRE(metric_pred >= -1 && metric_pred < K, DV_ERR_SHAPE);
  DV_REQUIRE((((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)stats) & 7u) == 0, DV_ERR_ALIGN);
  hipStream_t s = (hipStream_t)stream;
  double* partials = reinterpret_cast<double*>(workspace);
  const int blocks = blocks_for(n);
  if (K <= 1) launch_fwd<1>(t, gt, mask, mask_mode, max_disp, K, metric_pred, n, vec, partials, blocks, s);
  else if (K <= 4) launch_fwd<4>(t, gt, mask, mask_mode, max_disp, K, metric_pred, n, vec, partials, blocks, s);
  else if (K <= 8) launch_fwd<8>(t, gt, mask, mask_mode, max_disp, K, metric_pred, n, vec, partials, blocks, s);
  else if (K <= 16) launch_fwd<16>(t, gt, mask, mask_mode, max_disp, K, metric_pred, n, vec, partials, blocks, s);
  else launch_fwd<kMaxK>(t, gt, mask, mask_mode, max_disp, K, metric_pred, n, vec, partials, blocks, s);
  int e = dv_launch_status();
  if (e != DV_OK) return e;
  hipLaunchKernelGGL(masked_loss_merge_kernel, dim3(1), dim3(kThreads), 0, s, partials, blocks, K, t, stats, loss);
  return dv_launch_status();
}

extern "C" int dv_masked_loss_bwd_f32(const float* const* preds, const double* weights, const int* kinds, const float* gt,
                                      const void* mask, int mask_mode, float max_disp, const double* stats,
                                      const float* gout, float* const* dpreds, int K, long long n, dv_stream_t stream) {
  LossTable t;
  bool vec = false;
  DV_REQUIRE_PTR(dpreds);
  const int rc = fill_table(t, preds, dpreds, weights, kinds, gt, mask, mask_mode, max_disp, K, n, &vec);
  if (rc != DV_OK) return rc;
  DV_REQUIRE_PTR(stats);
  DV_REQUIRE_PTR(gout);
  DV_REQUIRE((((uintptr_t)stats) & 7u) == 0, DV_ERR_ALIGN);
  bool any = false;
  for (int k = 0; k < K; ++k) any = any || t.grad[k] != nullptr;
  DV_REQUIRE(any, DV_ERR_NULL);
  hipLaunchKernelGGL(masked_loss_bwd_kernel, dim3(blocks_for(n)), dim3(kThreads), 0, (hipStream_t)stream, t, gt, mask,
                     mask_mode, max_disp, K, n, vec ? 1 : 0, stats, gout);
  return dv_launch_status();
}
