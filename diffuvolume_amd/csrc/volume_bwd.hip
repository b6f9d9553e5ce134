// Backward of K1 (csrc/gwc_volume.hip) and K2 (csrc/concat_volume.hip): the gradients of the two cost-volume builders
// with respect to their feature maps and, for the scaled concatenation, the scale.
//
//   gwc      vol[b,g,d,y,x]   = (1/cpg) sum_c ref[b,g cpg+c,y,x] tgt[b,g cpg+c,y,x-d]                       (0 for x < d)
//            dref[b,c,y,x]    = (1/cpg) sum_{d<D, d<=x}   dvol[b,g,d,y,x]    tgt[b,c,y,x-d]
//            dtgt[b,c,y,x']   = (1/cpg) sum_{d<D, x'+d<W} dvol[b,g,d,y,x'+d] ref[b,c,y,x'+d]
//   concat   vol[b,c,d,y,x]   = s[b,d,y,x] ref[b,c,y,x],   vol[b,C+c,d,y,x] = s[b,d,y,x] tgt[b,c,y,x-d]    (0 for x < d)
//            dref[b,c,y,x]    = sum_d s dvol[b,c,d,y,x]                                  (d <= x only with zero_left)
//            dtgt[b,c,y,x']   = sum_{d, x'+d<W} s[b,d,y,x'+d] dvol[b,C+c,d,y,x'+d]
//            ds[b,d,y,x]      = sum_c dvol[b,c,d,y,x] ref[b,c,y,x] + [x>=d] sum_c dvol[b,C+c,d,y,x] tgt[b,c,y,x-d]
//
// Both are HBM-bound gathers over dvol, which is 2C/(1 or 2) .. D times larger than anything else they touch.  The row
// kernels read every float of dvol from HBM once, with 16-byte loads along W, into LDS, and every sum over d walks LDS:
//   gwc      one block per (b,g,y): the D x W slab of dvol is staged once and serves the cpg channels of the group for
//            both outputs; an item = (output, channel, quad of 4 x) keeps a sliding 8-float window of the other feature
//            row in registers (one new 16-byte load per 4 disparities), as the forward does.
//   concat   one block per (b,y, chunk of 8 channels): per channel the s-scaled left and right D x W slabs are staged,
//            then summed over d (the right one along the diagonal x = x'+d); the thread that loads dvol[., d, quad]
//            owns ds[d, quad] of its chunk in registers for all channels of the chunk.  With more than one chunk the
//            chunk sums go to a workspace [nchunks][B,D,H,W] and a second kernel adds them in ascending chunk order.
// Every output element is written once by one thread and every sum runs in a fixed order (ascending d; ascending c
// within a chunk, ascending chunks), independent of the grid and of B: no atomics, the same bits on every launch and for
// every batch split.  Staged rows are read as whole aligned quads by consecutive lanes (consecutive 16-byte addresses:
// conflict-free for ds_read_b128); the shift is taken in registers.
// Anything else (W not a multiple of 4, operands off a 16-byte line, cpg outside {4,8,12}, a slab beyond 64 KiB of LDS)
// runs the one-thread-per-output kernels at the bottom: same sums, same order over d.
#include "dv_common.h"
#include "../../include/diffuvolume_hip_volume_train.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 8;                    // channels of each half per block of the concat row kernel
constexpr size_t kLdsCap = 64 * 1024;        // dynamic LDS a block may ask for without further ado

__device__ __forceinline__ float4 ldq(const float* p, int q) { return reinterpret_cast<const float4*>(p)[q]; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// ---------------------------------------------------------------------------------------------------------- gwc, rows
template <int CPG>
__global__ __launch_bounds__(kThreads) void gwc_bwd_rows_kernel(const float* __restrict__ ref,
                                                                 const float* __restrict__ tgt,
                                                                 const float* __restrict__ dvol,
                                                                 float* __restrict__ dref, float* __restrict__ dtgt,
                                                                 int C, int H, int W, int D, int G) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float4* stage = reinterpret_cast<float4*>(smem);        // [Dp][nq], rows D..Dp-1 zero
  const int nq = W >> 2;
  const int eblocks = (D + 3) >> 2;
  const int Dp = 4 * eblocks;
  const int y = blockIdx.x % H;
  const int bg = blockIdx.x / H;                           // b * G + g
  const int g = bg % G;
  const int b = bg / G;
  const size_t plane = (size_t)H * W;
  const float* dv = dvol + ((size_t)bg * D * H + y) * W;   // d = 0; one plane per d

  for (int i = threadIdx.x; i < Dp * nq; i += kThreads) {
    const int d = i / nq, t = i - d * nq;
    stage[i] = d < D ? ldq(dv + (size_t)d * plane, t) : zero4();
  }
  __syncthreads();

  const size_t frow = ((size_t)b * C + (size_t)g * CPG) * plane + (size_t)y * W;   // channel 0 of the group, this row
  const int per = CPG * nq;
  for (int it = threadIdx.x + (dref ? 0 : per); it < (dtgt ? 2 * per : per); it += kThreads) {
    const bool right = it >= per;
    const int rem = right ? it - per : it;
    const int c = rem / nq, t = rem - c * nq;
    const size_t off = frow + (size_t)c * plane;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (!right) {
      // dref[x] += dvol[d][x] * tgt[x-d]: window w[0..7] = tgt[4(t-e-1) .. 4(t-e)+3], element 4+j-r is x-d
      const float* row = tgt + off;
      float4 hi = ldq(row, t);
      for (int e = 0; e < eblocks && e <= t; ++e) {
        const float4 lo = t - e - 1 >= 0 ? ldq(row, t - e - 1) : zero4();
        const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float4 q = stage[(4 * e + r) * nq + t];
          const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(v[j], w[4 + j - r], acc[j]);
        }
        hi = lo;
      }
    } else {
      // dtgt[x'] += dvol[d][x'+d] * ref[x'+d]: x'+d = 4(t+e) + (j+r), both windows start at quad t+e
      const float* row = ref + off;
      float4 lo = ldq(row, t);
      for (int e = 0; e < eblocks && t + e < nq; ++e) {
        const int q0 = t + e;
        const bool more = q0 + 1 < nq;
        const float4 hi = more ? ldq(row, q0 + 1) : zero4();
        const float w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float4 a = stage[(4 * e + r) * nq + q0];
          const float4 bq = more ? stage[(4 * e + r) * nq + q0 + 1] : zero4();
          const float v[8] = {a.x, a.y, a.z, a.w, bq.x, bq.y, bq.z, bq.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = fmaf(v[j + r], w[j + r], acc[j]);
        }
        lo = hi;
      }
    }
    const float4 o = make_float4(acc[0] / (float)CPG, acc[1] / (float)CPG, acc[2] / (float)CPG, acc[3] / (float)CPG);
    reinterpret_cast<float4*>((right ? dtgt : dref) + off)[t] = o;
  }
}

// ------------------------------------------------------------------------------------------------------- gwc, generic
// One thread per element of dref (kind 0) and of dtgt (kind 1).
__global__ void gwc_bwd_generic_kernel(const float* __restrict__ ref, const float* __restrict__ tgt,
                                       const float* __restrict__ dvol, float* __restrict__ dref,
                                       float* __restrict__ dtgt, int C, int H, int W, int D, int G, size_t n) {
  const int cpg = C / G;
  const size_t plane = (size_t)H * W;
  const size_t first = dref ? 0 : n, last = dtgt ? 2 * n : n;
  for (size_t k = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < last; k += (size_t)gridDim.x * blockDim.x) {
    const bool right = k >= n;
    const size_t i = right ? k - n : k;                   // ((b*C + c)*H + y)*W + x
    const int x = (int)(i % W);
    size_t r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const float* dv = dvol + (((size_t)b * G + c / cpg) * D * H + y) * W + x;    // d = 0
    float acc = 0.f;
    if (!right) {
      const int nd = D < x + 1 ? D : x + 1;
      for (int d = 0; d < nd; ++d) acc = fmaf(dv[(size_t)d * plane], tgt[i - d], acc);
      dref[i] = acc / (float)cpg;
    } else {
      const int nd = D < W - x ? D : W - x;
      for (int d = 0; d < nd; ++d) acc = fmaf(dv[(size_t)d * plane + d], ref[i + d], acc);
      dtgt[i] = acc / (float)cpg;
    }
  }
}

// ------------------------------------------------------------------------------------------------------- concat, rows
// ITEMS: (d, quad) pairs of the D x W/4 slab a thread loads per channel -- and whose ds it owns.
template <int ITEMS>
__global__ __launch_bounds__(kThreads) void concat_bwd_rows_kernel(const float* __restrict__ ref,
                                                                    const float* __restrict__ tgt,
                                                                    const float* __restrict__ s,
                                                                    const float* __restrict__ dvol,
                                                                    float* __restrict__ dref, float* __restrict__ dtgt,
                                                                    float* __restrict__ dsout, size_t ds_chunk_stride,
                                                                    int C, int H, int W, int D, int zero_left,
                                                                    int nchunks) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int nq = W >> 2;
  const int eblocks = (D + 3) >> 2;
  const int Dp = 4 * eblocks;
  const int nitems = D * nq;
  float4* stageL = reinterpret_cast<float4*>(smem);        // [D][nq]   s * dvol[c]
  float4* stageR = stageL + (size_t)Dp * nq;               // [Dp][nq]  s * dvol[C+c], rows D..Dp-1 zero

  const unsigned bid = dv_xcd_remap(blockIdx.x, gridDim.x);
  const int chunk = bid % nchunks;
  const int by = bid / nchunks;
  const int y = by % H;
  const int b = by / H;
  const int c0 = chunk * kChunk;
  const int nc = min(kChunk, C - c0);
  const size_t plane = (size_t)H * W;
  const size_t vstride = (size_t)D * plane;                // channel stride of the volume

  for (int i = nitems + threadIdx.x; i < Dp * nq; i += kThreads) stageR[i] = zero4();

  float4 acc[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) acc[k] = zero4();
  const float* srow = s ? s + (size_t)b * D * plane + (size_t)y * W : nullptr;    // d = 0

  for (int c = 0; c < nc; ++c) {
    const float* dl = dvol + ((size_t)b * 2 * C + c0 + c) * vstride + (size_t)y * W;   // d = 0
    const float* dr = dl + (size_t)C * vstride;
    const size_t frow = ((size_t)b * C + c0 + c) * plane + (size_t)y * W;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int i = threadIdx.x + k * kThreads;
      if (i < nitems) {
        const int d = i / nq, t = i - d * nq;
        const float4 L = ldq(dl + (size_t)d * plane, t);
        const float4 R = ldq(dr + (size_t)d * plane, t);
        float4 sl = L, sr = R;
        if (srow) {
          const float4 q = ldq(srow + (size_t)d * plane, t);
          sl = make_float4(q.x * L.x, q.y * L.y, q.z * L.z, q.w * L.w);
          sr = make_float4(q.x * R.x, q.y * R.y, q.z * R.z, q.w * R.w);
        }
        if (zero_left) {
          const int x = 4 * t;
          if (x < d) sl.x = 0.f;
          if (x + 1 < d) sl.y = 0.f;
          if (x + 2 < d) sl.z = 0.f;
          if (x + 3 < d) sl.w = 0.f;
        }
        if (dref) stageL[i] = sl;
        if (dtgt) stageR[i] = sr;
        if (dsout) {
          const float4 rq = ldq(ref + frow, t);
          const float* trow = tgt + frow;
          const int x = 4 * t - d;                          // tgt[x + j], 0 where negative
          const float t0 = x >= 0 ? trow[x] : 0.f, t1 = x + 1 >= 0 ? trow[x + 1] : 0.f;
          const float t2 = x + 2 >= 0 ? trow[x + 2] : 0.f, t3 = x + 3 >= 0 ? trow[x + 3] : 0.f;
          acc[k].x = fmaf(R.x, t0, fmaf(L.x, rq.x, acc[k].x));
          acc[k].y = fmaf(R.y, t1, fmaf(L.y, rq.y, acc[k].y));
          acc[k].z = fmaf(R.z, t2, fmaf(L.z, rq.z, acc[k].z));
          acc[k].w = fmaf(R.w, t3, fmaf(L.w, rq.w, acc[k].w));
        }
      }
    }
    if (!dref && !dtgt) continue;                            // ds alone: nothing is staged
    __syncthreads();
    for (int it = threadIdx.x + (dref ? 0 : nq); it < (dtgt ? 2 * nq : nq); it += kThreads) {
      const bool right = it >= nq;
      const int t = right ? it - nq : it;
      float a[4] = {0.f, 0.f, 0.f, 0.f};
      if (!right) {
        for (int d = 0; d < D; ++d) {
          const float4 q = stageL[d * nq + t];
          a[0] += q.x; a[1] += q.y; a[2] += q.z; a[3] += q.w;
        }
      } else {
        for (int e = 0; e < eblocks && t + e < nq; ++e) {
          const int q0 = t + e;
          const bool more = q0 + 1 < nq;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float4 lo = stageR[(4 * e + r) * nq + q0];
            const float4 hi = more ? stageR[(4 * e + r) * nq + q0 + 1] : zero4();
            const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] += v[j + r];
          }
        }
      }
      reinterpret_cast<float4*>((right ? dtgt : dref) + frow)[t] = make_float4(a[0], a[1], a[2], a[3]);
    }
    __syncthreads();
  }

  if (dsout) {
    float* out = dsout + (size_t)chunk * ds_chunk_stride + (size_t)b * D * plane + (size_t)y * W;   // d = 0
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int i = threadIdx.x + k * kThreads;
      if (i < nitems) {
        const int d = i / nq, t = i - d * nq;
        reinterpret_cast<float4*>(out + (size_t)d * plane)[t] = acc[k];
      }
    }
  }
}

// ds = the chunk sums of the workspace, added in ascending chunk order.
__global__ void concat_bwd_ds_reduce_kernel(const float* __restrict__ ws, float* __restrict__ ds, size_t nquads,
                                            int nchunks) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nquads; i += (size_t)gridDim.x * blockDim.x) {
    float4 a = reinterpret_cast<const float4*>(ws)[i];
    for (int k = 1; k < nchunks; ++k) {
      const float4 p = reinterpret_cast<const float4*>(ws)[(size_t)k * nquads + i];
      a.x += p.x; a.y += p.y; a.z += p.z; a.w += p.w;
    }
    reinterpret_cast<float4*>(ds)[i] = a;
  }
}

// ---------------------------------------------------------------------------------------------------- concat, generic
// One thread per element of dref (kind 0) and of dtgt (kind 1): sums over d.
__global__ void concat_bwd_feat_generic_kernel(const float* __restrict__ s, const float* __restrict__ dvol,
                                               float* __restrict__ dref, float* __restrict__ dtgt, int C, int H, int W,
                                               int D, int zero_left, size_t n) {
  const size_t plane = (size_t)H * W;
  const size_t first = dref ? 0 : n, last = dtgt ? 2 * n : n;
  for (size_t k = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < last; k += (size_t)gridDim.x * blockDim.x) {
    const bool right = k >= n;
    const size_t i = right ? k - n : k;                   // ((b*C + c)*H + y)*W + x
    const int x = (int)(i % W);
    size_t r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const float* dv = dvol + (((size_t)b * 2 * C + (right ? C + c : c)) * D * H + y) * W + x;   // d = 0
    const float* sp = s ? s + ((size_t)b * D * H + y) * W + x : nullptr;                          // d = 0
    float acc = 0.f;
    if (!right) {
      const int nd = (zero_left && x + 1 < D) ? x + 1 : D;
      for (int d = 0; d < nd; ++d) acc += sp ? sp[(size_t)d * plane] * dv[(size_t)d * plane] : dv[(size_t)d * plane];
      dref[i] = acc;
    } else {
      const int nd = D < W - x ? D : W - x;
      for (int d = 0; d < nd; ++d)
        acc += sp ? sp[(size_t)d * plane + d] * dv[(size_t)d * plane + d] : dv[(size_t)d * plane + d];
      dtgt[i] = acc;
    }
  }
}

// One thread per element of ds: sums over c, ascending.
__global__ void concat_bwd_ds_generic_kernel(const float* __restrict__ ref, const float* __restrict__ tgt,
                                             const float* __restrict__ dvol, float* __restrict__ ds, int C, int H,
                                             int W, int D, size_t n) {
  const size_t plane = (size_t)H * W;
  const size_t vstride = (size_t)D * plane;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);                           // i = ((b*D + d)*H + y)*W + x
    size_t r = i / W;
    const int y = (int)(r % H);
    r /= H;
    const int d = (int)(r % D);
    const int b = (int)(r / D);
    const float* dl = dvol + (((size_t)b * 2 * C) * D + d) * plane + (size_t)y * W + x;   // c = 0
    const float* dr = dl + (size_t)C * vstride;
    const size_t f = (size_t)b * C * plane + (size_t)y * W + x;                            // c = 0
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
      acc = fmaf(dl[(size_t)c * vstride], ref[f + (size_t)c * plane], acc);
      if (x >= d) acc = fmaf(dr[(size_t)c * vstride], tgt[f + (size_t)c * plane - d], acc);
    }
    ds[i] = acc;
  }
}

inline int grid_for(size_t n) { return (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384); }

template <int CPG>
int launch_gwc_rows(const float* ref, const float* tgt, const float* dvol, float* dref, float* dtgt, int B, int C,
                    int H, int W, int D, int G, hipStream_t st) {
  const size_t lds = (size_t)4 * ((D + 3) / 4) * W * sizeof(float);
  if (lds > kLdsCap) return DV_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(gwc_bwd_rows_kernel<CPG>, dim3((unsigned)B * G * H), dim3(kThreads), lds, st, ref, tgt, dvol,
                     dref, dtgt, C, H, W, D, G);
  return dv_launch_status();
}

// The concat row kernel applies to a shape (the operands' alignment is a matter of the call).
inline bool concat_rows_shape(int W, int D) {
  if (W % 4) return false;
  const size_t lds = (size_t)2 * 4 * ((D + 3) / 4) * W * sizeof(float);
  return lds <= kLdsCap && (size_t)D * (W / 4) <= (size_t)16 * kThreads;
}

inline int concat_chunks(int C) { return (C + kChunk - 1) / kChunk; }

}  // namespace

extern "C" int dv_gwc_volume_bwd_f32(const float* ref, const float* tgt, const float* dvol, float* dref, float* dtgt,
                                     int B, int C, int H, int W, int D, int G, dv_stream_t stream) {
  DV_REQUIRE_PTR(ref);
  DV_REQUIRE_PTR(tgt);
  DV_REQUIRE_PTR(dvol);
  DV_REQUIRE(dref != nullptr || dtgt != nullptr, DV_ERR_NULL);
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && D > 0 && G > 0, DV_ERR_SHAPE);
  DV_REQUIRE(C % G == 0, DV_ERR_SHAPE);
  DV_REQUIRE((size_t)B * G * H < ((size_t)1 << 31), DV_ERR_UNSUPPORTED);
  hipStream_t st = (hipStream_t)stream;
  const int cpg = C / G;
  const bool fast = (W % 4 == 0) && dv_aligned16(ref) && dv_aligned16(tgt) && dv_aligned16(dvol) &&
                    dv_aligned16(dref) && dv_aligned16(dtgt);
  if (fast) {
    int rc = DV_ERR_UNSUPPORTED;
    if (cpg == 8) rc = launch_gwc_rows<8>(ref, tgt, dvol, dref, dtgt, B, C, H, W, D, G, st);
    else if (cpg == 12) rc = launch_gwc_rows<12>(ref, tgt, dvol, dref, dtgt, B, C, H, W, D, G, st);
    else if (cpg == 4) rc = launch_gwc_rows<4>(ref, tgt, dvol, dref, dtgt, B, C, H, W, D, G, st);
    if (rc != DV_ERR_UNSUPPORTED) return rc;
  }
  const size_t n = (size_t)B * C * H * W;
  const size_t work = (dref ? n : 0) + (dtgt ? n : 0);
  hipLaunchKernelGGL(gwc_bwd_generic_kernel, dim3(grid_for(work)), dim3(256), 0, st, ref, tgt, dvol, dref, dtgt, C, H,
                     W, D, G, n);
  return dv_launch_status();
}

extern "C" size_t dv_concat_volume_bwd_workspace_floats(int B, int C, int H, int W, int D) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0) return 0;
  if (!concat_rows_shape(W, D) || concat_chunks(C) < 2) return 0;
  return (size_t)concat_chunks(C) * B * D * H * W;
}

extern "C" int dv_concat_volume_bwd_f32(const float* ref, const float* tgt, const float* s, const float* dvol,
                                        float* dref, float* dtgt, float* ds, float* workspace, int B, int C, int H,
                                        int W, int D, int zero_left, dv_stream_t stream) {
  DV_REQUIRE_PTR(dvol);
  DV_REQUIRE(dref != nullptr || dtgt != nullptr || ds != nullptr, DV_ERR_NULL);
  if (ds != nullptr) {
    DV_REQUIRE_PTR(s);                                     // ds of the plain concatenation does not exist
    DV_REQUIRE_PTR(ref);
    DV_REQUIRE_PTR(tgt);
  }
  DV_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && D > 0, DV_ERR_SHAPE);
  DV_REQUIRE(!(s != nullptr && zero_left), DV_ERR_UNSUPPORTED);   // dv_concat_prob_volume_f32 has no such forward
  const size_t nws = dv_concat_volume_bwd_workspace_floats(B, C, H, W, D);
  if (ds != nullptr && nws) DV_REQUIRE_PTR(workspace);
  DV_REQUIRE((size_t)B * H * concat_chunks(C) < ((size_t)1 << 31), DV_ERR_UNSUPPORTED);
  hipStream_t st = (hipStream_t)stream;
  const bool fast = concat_rows_shape(W, D) && dv_aligned16(ref) && dv_aligned16(tgt) && dv_aligned16(s) &&
                    dv_aligned16(dvol) && dv_aligned16(dref) && dv_aligned16(dtgt) && dv_aligned16(ds) &&
                    (!(ds && nws) || dv_aligned16(workspace));
  const size_t nds = (size_t)B * D * H * W;
  if (fast) {
    const int nchunks = concat_chunks(C);
    const size_t lds = (size_t)2 * 4 * ((D + 3) / 4) * W * sizeof(float);
    float* dsout = ds ? (nchunks > 1 ? workspace : ds) : nullptr;
    const dim3 grid((unsigned)B * H * nchunks);
    if ((size_t)D * (W / 4) <= (size_t)6 * kThreads)
      hipLaunchKernelGGL(concat_bwd_rows_kernel<6>, grid, dim3(kThreads), lds, st, ref, tgt, s, dvol, dref, dtgt, dsout,
                         nds, C, H, W, D, zero_left, nchunks);
    else
      hipLaunchKernelGGL(concat_bwd_rows_kernel<16>, grid, dim3(kThreads), lds, st, ref, tgt, s, dvol, dref, dtgt,
                         dsout, nds, C, H, W, D, zero_left, nchunks);
    int rc = dv_launch_status();
    if (rc != DV_OK || !ds || nchunks < 2) return rc;
    hipLaunchKernelGGL(concat_bwd_ds_reduce_kernel, dim3(grid_for(nds / 4)), dim3(256), 0, st, workspace, ds, nds / 4,
                       nchunks);
    return dv_launch_status();
  }
  if (dref || dtgt) {
    const size_t n = (size_t)B * C * H * W;
    hipLaunchKernelGGL(concat_bwd_feat_generic_kernel, dim3(grid_for((dref ? n : 0) + (dtgt ? n : 0))), dim3(256), 0, st,
                       s, dvol, dref, dtgt, C, H, W, D, zero_left, n);
    const int rc = dv_launch_status();
    if (rc != DV_OK) return rc;
  }
  if (ds) {
    hipLaunchKernelGGL(concat_bwd_ds_generic_kernel, dim3(grid_for(nds)), dim3(256), 0, st, ref, tgt, dvol, ds, C, H, W,
                       D, nds);
    return dv_launch_status();
  }
  return DV_OK;
}
