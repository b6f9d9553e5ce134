// Weight gradient of the dilation-1 convolutions of IGEV's recurrent update block over a VIRTUAL channel concatenation
// (training: the backward of ConvGRU's convz / convr / convq, KITTI15/core/update.py:26-40, of BasicMotionEncoder,
// update.py:74-94, of DispHead.conv1, update.py:15-24, and of mask_feat_4, update.py:115-117):
//   dW[co, ci, ky, kx] = sum_{b, y, x} g[b, co, y, x] * X[b, ci, y + ky - p, x + kx - p],  X = cat(inputs, dim=1),
//   k in {1, 3}, p = (k-1)/2, stride 1, X zero outside the image; `inputs` as in dv_conv2d_cat_f32 (1..4 tensors).
// An implicit GEMM M = Cout, N = Cin*k^2, K = B*H*W on the exact-fp32 matrix instruction v_mfma_f32_16x16x4_f32.
//
// Against csrc/conv2d_wgrad.hip (built for refinenet3's dilated layers, kept as it is):
//   * the block tile is 64 co x 64 ci: each of the four waves owns 32 x 32 (2 x 2 MFMA tiles x k^2 taps = 144 accumulator
//     registers for k = 3); a g fragment feeds 2 * k^2 MFMAs and an x fragment two;
//   * dilation 1 lets all three tap rows share ONE halo tile of x, (TY+2) x (TX+2) per channel, instead of three bands
//     (136 floats per channel and brick instead of 480);
//   * the staging is double-buffered through registers: the global loads of brick n+1 are issued before the MFMAs of
//     brick n and stored to LDS after them, so their latency is covered by the same block's arithmetic (one LDS buffer of
//     58 KB).  144 accumulators + 50 staging registers + the fragments of an unrolled brick do not fit 256 registers
//     (the compiler spilled 220-280 of them under __launch_bounds__(256, 2)), so a block has a CU to itself: one wave
//     per SIMD with the full 512-register file, 36 independent MFMAs per step keep the pipe busy without a second wave;
//   * every thread's share of a brick is fixed (compile-time LDS offsets, no division in the staging loop): per iteration
//     a 32-lane half-wave loads one image row of 32 floats (one 128-byte line when the plane allows it).
// The K dimension (bricks of TY x TX = 2 x 32 output positions, all batch items in one sequence) is split over blocks;
// each split writes its partial [Cout][Cin][k^2] into the caller's workspace, a second kernel sums the splits in split
// order.  No atomics: the bits depend on the shape only.  (The split plan counts the bricks of the whole batch, so a
// batch and its halves are NOT summed in the same order.)
// Non-finite values: the positions of a brick outside the image are staged as g = 0 (and x = 0) and multiplied like any
// other, so a NaN OR an Inf in x next to the bottom / right edge of a plane that is no multiple of the brick meets a
// 0 of g: 0 * Inf = NaN in dw where the exact sum has no such product (csrc/conv2d_wgrad.hip has the same property).
// It stays in the rows of dw that belong to that input channel.
//
// Also here, for the same training route: the ConvGRU gate arithmetic (forward-for-training and backward, elementwise
// float4 kernels) and the weight gradient of the 7x7 single-input-channel convd1.
//
// LDS bank map (ds_read_b32, conflicts inside a 32-lane half): lane l reads channel l & 15 at output position l >> 4;
// per-channel strides are 2 mod 32 and the two positions of a half are adjacent dwords: conflict-free for every tap.
#include "dv_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int WC_CO = 64, WC_CI = 64, WC_THREADS = 256;
constexpr int WC_TY = 2, WC_TX = 32;                     // output brick
constexpr int WC_TARGET_BLOCKS = 256;                    // one block per CU on 256 CUs, one round
constexpr long long WC_MAX_WS_FLOATS = 12ll << 20;       // workspace bound: 48 MB
constexpr int WC_MAX_INPUTS = 4;

constexpr int wc_pad_2mod32(int n) { return n + (((2 - n % 32) % 32) + 32) % 32; }

template <int KS_>
struct WcGeo {
  static constexpr int KS = KS_, KT = KS * KS, HALO = (KS - 1) / 2;
  static constexpr int HR = WC_TY + KS - 1, HC = WC_TX + KS - 1;        // halo tile of x per channel
  static constexpr int XS = wc_pad_2mod32(HR * HC);                     // per-channel stride of the x tile
  static constexpr int GS = wc_pad_2mod32(WC_TY * WC_TX);               // per-channel stride of the g tile
  static constexpr int NX = WC_CI * HR / 8;                             // interior loads per thread (8 rows per pass)
  static constexpr int NE = KS == 1 ? 0 : 2;                            // halo-column loads per thread
  static constexpr int NG = WC_CO * WC_TY / 8;                          // g loads per thread
  static_assert(8 % HR == 0, "a pass of 8 rows holds whole channels");
  static_assert(KS == 1 || WC_CI * HR == WC_THREADS, "one halo row per thread");
  static_assert((WC_CI * XS + WC_CO * GS) * 4 <= 64 * 1024, "static LDS");
};

struct WcArgs {
  const float* src[WC_MAX_INPUTS];   // [B, c_i, H, W]
  int coff[WC_MAX_INPUTS + 1];       // first channel of source i in the concatenation; coff[n..4] = Cin
  const float* g;                    // [B, Cout, H, W]
  float* ws;                         // [splits, Cout, Cin, KT]
  int B, Cin, H, W, Cout;
  int nby, nbx, splits;
  long long nbricks;
};

// plane of channel ci (< Cin) of the concatenation, batch item b
__device__ __forceinline__ const float* wc_plane(const WcArgs& a, int ci, int b, size_t plane) {
  const float* p = a.src[0];
  int lo = 0, hi = a.coff[1];
  if (ci >= a.coff[1]) { p = a.src[1]; lo = a.coff[1]; hi = a.coff[2]; }
  if (ci >= a.coff[2]) { p = a.src[2]; lo = a.coff[2]; hi = a.coff[3]; }
  if (ci >= a.coff[3]) { p = a.src[3]; lo = a.coff[3]; hi = a.coff[4]; }
  return p + ((size_t)b * (hi - lo) + (ci - lo)) * plane;
}

template <class G>
struct WcRegs {
  float x[G::NX];
  float e[G::NE == 0 ? 1 : G::NE];
  float g[G::NG];
};

// the calling thread's share of brick `br`, from global memory into registers (zeros outside the image / the channels)
template <class G>
__device__ __forceinline__ void wc_load(const WcArgs& a, long long br, int co0, int ci0, int tid, WcRegs<G>& r) {
  long long q = br;
  const int bx = (int)(q % a.nbx); q /= a.nbx;
  const int by = (int)(q % a.nby); q /= a.nby;
  const int b = (int)q;
  const int oy0 = by * WC_TY, ox0 = bx * WC_TX;
  const size_t plane = (size_t)a.H * a.W;
  const int col = tid & 31, rw = tid >> 5;               // 8 rows of 32 columns per pass
  {
    const int hr = rw % G::HR, cb = __builtin_amdgcn_readfirstlane(rw / G::HR);
    const int iy = oy0 + hr - G::HALO, ix = ox0 + col;
    const bool in = iy >= 0 && iy < a.H && ix < a.W;
    const unsigned off = (unsigned)((in ? iy : 0) * a.W + (in ? ix : 0));     // (H*W < 2^30: checked by the entry)
#pragma unroll
    for (int j = 0; j < G::NX; ++j) {
      const int ci = ci0 + cb + j * (8 / G::HR);
      float v = 0.f;
      if (in && ci < a.Cin) v = wc_plane(a, ci, b, plane)[off];
      r.x[j] = v;
    }
  }
  if constexpr (G::NE != 0) {                            // columns ox0 - 1 and ox0 + TX of halo row `tid`
    const int hr = tid % G::HR, c = tid / G::HR;
    const int iy = oy0 + hr - G::HALO, ci = ci0 + c;
    const bool rin = iy >= 0 && iy < a.H && ci < a.Cin;
    const float* p = wc_plane(a, rin ? ci : 0, b, plane) + (size_t)(rin ? iy : 0) * a.W;
    r.e[0] = (rin && ox0 >= 1) ? p[ox0 - 1] : 0.f;
    r.e[G::NE - 1] = (rin && ox0 + WC_TX < a.W) ? p[ox0 + WC_TX] : 0.f;
  }
  {
    const int py = rw % WC_TY, cb = __builtin_amdgcn_readfirstlane(rw / WC_TY);
    const int oy = oy0 + py, ox = ox0 + col;
    const bool in = oy < a.H && ox < a.W;
    const unsigned off = (unsigned)((in ? oy : 0) * a.W + (in ? ox : 0));
#pragma unroll
    for (int j = 0; j < G::NG; ++j) {
      const int co = co0 + cb + j * (8 / WC_TY);
      float v = 0.f;
      if (in && co < a.Cout) v = (a.g + ((size_t)b * a.Cout + co) * plane)[off];
      r.g[j] = v;
    }
  }
}

template <class G>
__device__ __forceinline__ void wc_store(float* xs, float* gs, int tid, const WcRegs<G>& r) {
  const int col = tid & 31, rw = tid >> 5;
  {
    float* p = xs + (rw / G::HR) * G::XS + (rw % G::HR) * G::HC + G::HALO + col;
#pragma unroll
    for (int j = 0; j < G::NX; ++j) p[j * (8 / G::HR) * G::XS] = r.x[j];
  }
  if constexpr (G::NE != 0) {
    float* p = xs + (tid / G::HR) * G::XS + (tid % G::HR) * G::HC;
    p[0] = r.e[0];
    p[G::HC - 1] = r.e[G::NE - 1];
  }
  {
    float* p = gs + (rw / WC_TY) * G::GS + (rw % WC_TY) * WC_TX + col;
#pragma unroll
    for (int j = 0; j < G::NG; ++j) p[j * (8 / WC_TY) * G::GS] = r.g[j];
  }
}

template <class G>
__global__ __launch_bounds__(WC_THREADS, 1) void conv2d_wgrad_cat_kernel(WcArgs a) {
  __shared__ float xs[WC_CI * G::XS];
  __shared__ float gs[WC_CO * G::GS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int co0 = blockIdx.x * WC_CO, ci0 = blockIdx.y * WC_CI, split = blockIdx.z;
  const int cow = wave & 1, ciw = wave >> 1;             // the wave's 32 co x 32 ci quarter
  const int li = lane & 15, lk = lane >> 4;

  f32x4 acc[4][G::KT];                                   // [2 co tiles x 2 ci tiles][taps]
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int t = 0; t < G::KT; ++t) acc[m][t] = f32x4{0.f, 0.f, 0.f, 0.f};

  const long long b0 = a.nbricks * split / a.splits, b1 = a.nbricks * (split + 1) / a.splits;
  const float* xrd = xs + (ciw * 32 + li) * G::XS + lk;
  const float* grd = gs + (cow * 32 + li) * G::GS + lk;

  WcRegs<G> regs;
  if (b0 < b1) wc_load<G>(a, b0, co0, ci0, tid, regs);
  for (long long br = b0; br < b1; ++br) {
    __syncthreads();                                     // the previous brick's reads are done
    wc_store<G>(xs, gs, tid, regs);
    __syncthreads();
    if (br + 1 < b1) wc_load<G>(a, br + 1, co0, ci0, tid, regs);     // in flight during the MFMAs below

#pragma unroll
    for (int py = 0; py < WC_TY; ++py) {
#pragma unroll
      for (int sx = 0; sx < WC_TX / 4; ++sx) {
        const int p = py * WC_TX + sx * 4;               // (+ lk: folded into grd / xrd)
        const float a0 = grd[p], a1 = grd[16 * G::GS + p];
#pragma unroll
        for (int ky = 0; ky < G::KS; ++ky) {
#pragma unroll
          for (int kx = 0; kx < G::KS; ++kx) {
            const int o = (py + ky) * G::HC + sx * 4 + kx;
            const float x0 = xrd[o], x1 = xrd[16 * G::XS + o];
            const int t = ky * G::KS + kx;
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, x0, acc[0][t], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, x1, acc[1][t], 0, 0, 0);
            acc[2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, x0, acc[2][t], 0, 0, 0);
            acc[3][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, x1, acc[3][t], 0, 0, 0);
          }
        }
      }
    }
  }

  // D layout: col = lane & 15 (ci), row = 4 * (lane >> 4) + r (co)
  float* out = a.ws + (size_t)split * a.Cout * a.Cin * G::KT;
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const int ci = ci0 + ciw * 32 + (m & 1) * 16 + li;
    if (ci >= a.Cin) continue;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int co = co0 + cow * 32 + (m >> 1) * 16 + 4 * lk + rr;
      if (co >= a.Cout) continue;
      float* o = out + ((size_t)co * a.Cin + ci) * G::KT;
#pragma unroll
      for (int t = 0; t < G::KT; ++t) o[t] = acc[m][t][rr];
    }
  }
}

struct WcPlan {
  int nby, nbx, splits;
  long long nbricks;
};

WcPlan wc_plan(int B, int Cin, int H, int W, int Cout, int k) {
  WcPlan p;
  p.nby = (H + WC_TY - 1) / WC_TY;
  p.nbx = (W + WC_TX - 1) / WC_TX;
  p.nbricks = (long long)B * p.nby * p.nbx;
  // split K so that the grid fills the device once (a block has a CU to itself: a second, partial round would cost a
  // whole one), within the workspace bound, at least two bricks per split
  const long long mn = (long long)((Cout + WC_CO - 1) / WC_CO) * ((Cin + WC_CI - 1) / WC_CI);
  long long s = WC_TARGET_BLOCKS / mn;
  const long long cap = WC_MAX_WS_FLOATS / ((long long)Cout * Cin * k * k);
  if (s > cap) s = cap;
  if (s > p.nbricks / 2) s = p.nbricks / 2;
  if (s < 1) s = 1;
  p.splits = (int)s;
  return p;
}

// sum of the channel counts, or 0 when the description of the sources is unusable
long long wc_cin(const int* channels, int n_inputs) {
  if (channels == nullptr || n_inputs < 1 || n_inputs > WC_MAX_INPUTS) return 0;
  long long c = 0;
  for (int i = 0; i < n_inputs; ++i) {
    if (channels[i] <= 0) return 0;
    c += channels[i];
  }
  return c > 0x3fffffff ? 0 : c;
}

bool wc_valid(long long cin, int B, int H, int W, int Cout, int k) {
  return (k == 1 || k == 3) && cin > 0 && B > 0 && H > 0 && W > 0 && Cout > 0 && (long long)H * W < (1ll << 30) &&
         (long long)Cout * cin * k * k <= WC_MAX_WS_FLOATS;
}

template <class G>
int wc_launch(const WcArgs& a, float* dw, hipStream_t s) {
  dim3 grid((unsigned)((a.Cout + WC_CO - 1) / WC_CO), (unsigned)((a.Cin + WC_CI - 1) / WC_CI), (unsigned)a.splits);
  hipLaunchKernelGGL(conv2d_wgrad_cat_kernel<G>, grid, dim3(WC_THREADS), 0, s, a);
  const int rc = dv_launch_status();
  if (rc != DV_OK) return rc;
  dv_splitk_sum(a.ws, dw, (long long)a.Cout * a.Cin * G::KT, a.splits, s);
  return dv_launch_status();
}

// ---- ConvGRU gate arithmetic for training (update.py:36-39) --------------------------------------------------------
// float4 bodies on 16-byte aligned pointers, scalar tails; the host entry falls back to the scalar body for views that
// are not 16-byte aligned.
template <int V>
__global__ __launch_bounds__(256) void gru_mul_kernel(const float* __restrict__ r, const float* __restrict__ h,
                                                      float* __restrict__ rh, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = V == 4 ? n / 4 : 0;
  for (size_t i = i0; i < nv; i += stride) {
    const float4 a = ((const float4*)r)[i], b = ((const float4*)h)[i];
    ((float4*)rh)[i] = make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
  }
  for (size_t i = nv * 4 + i0; i < n; i += stride) rh[i] = r[i] * h[i];
}

// (1 - z) h + z q in the form of the inference epilogue (csrc/conv2d.hip: blend_h + blend_z * (v - blend_h)), so that the
// training forward and the eval forward round the hidden state alike
__device__ __forceinline__ float gru_blend1(float z, float q, float h) { return h + z * (q - h); }

template <int V>
__global__ __launch_bounds__(256) void gru_blend_kernel(const float* __restrict__ z, const float* __restrict__ q,
                                                        const float* __restrict__ h, float* __restrict__ out, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = V == 4 ? n / 4 : 0;
  for (size_t i = i0; i < nv; i += stride) {
    const float4 a = ((const float4*)z)[i], b = ((const float4*)q)[i], c = ((const float4*)h)[i];
    ((float4*)out)[i] = make_float4(gru_blend1(a.x, b.x, c.x), gru_blend1(a.y, b.y, c.y), gru_blend1(a.z, b.z, c.z),
                                    gru_blend1(a.w, b.w, c.w));
  }
  for (size_t i = nv * 4 + i0; i < n; i += stride) out[i] = gru_blend1(z[i], q[i], h[i]);
}

// from dh', z, q, h:  dq_pre = dh' z (1 - q^2),  dz_pre = dh' (q - h) z (1 - z),  dh = dh' (1 - z)
__device__ __forceinline__ void gru_bwd_blend1(float d, float z, float q, float h, float& dq, float& dz, float& dh) {
  dq = d * z * (1.0f - q * q);
  dz = d * (q - h) * z * (1.0f - z);
  dh = d * (1.0f - z);
}

template <int V>
__global__ __launch_bounds__(256) void gru_bwd_blend_kernel(const float* __restrict__ dhn, const float* __restrict__ z,
                                                            const float* __restrict__ q, const float* __restrict__ h,
                                                            float* __restrict__ dq, float* __restrict__ dz,
                                                            float* __restrict__ dh, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = V == 4 ? n / 4 : 0;
  for (size_t i = i0; i < nv; i += stride) {
    const float4 d = ((const float4*)dhn)[i], a = ((const float4*)z)[i], b = ((const float4*)q)[i],
                 c = ((const float4*)h)[i];
    float4 oq, oz, oh;
    gru_bwd_blend1(d.x, a.x, b.x, c.x, oq.x, oz.x, oh.x);
    gru_bwd_blend1(d.y, a.y, b.y, c.y, oq.y, oz.y, oh.y);
    gru_bwd_blend1(d.z, a.z, b.z, c.z, oq.z, oz.z, oh.z);
    gru_bwd_blend1(d.w, a.w, b.w, c.w, oq.w, oz.w, oh.w);
    ((float4*)dq)[i] = oq;
    ((float4*)dz)[i] = oz;
    ((float4*)dh)[i] = oh;
  }
  for (size_t i = nv * 4 + i0; i < n; i += stride) gru_bwd_blend1(dhn[i], z[i], q[i], h[i], dq[i], dz[i], dh[i]);
}

// from d(rh), r, h:  dr_pre = d(rh) h r (1 - r),  dh += d(rh) r
__device__ __forceinline__ void gru_bwd_reset1(float d, float r, float h, float& dr, float& dh) {
  dr = d * h * r * (1.0f - r);
  dh += d * r;
}

template <int V>
__global__ __launch_bounds__(256) void gru_bwd_reset_kernel(const float* __restrict__ drh, const float* __restrict__ r,
                                                            const float* __restrict__ h, float* __restrict__ dr,
                                                            float* __restrict__ dh, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nv = V == 4 ? n / 4 : 0;
  for (size_t i = i0; i < nv; i += stride) {
    const float4 d = ((const float4*)drh)[i], a = ((const float4*)r)[i], c = ((const float4*)h)[i];
    float4 o, acc = ((float4*)dh)[i];
    gru_bwd_reset1(d.x, a.x, c.x, o.x, acc.x);
    gru_bwd_reset1(d.y, a.y, c.y, o.y, acc.y);
    gru_bwd_reset1(d.z, a.z, c.z, o.z, acc.z);
    gru_bwd_reset1(d.w, a.w, c.w, o.w, acc.w);
    ((float4*)dr)[i] = o;
    ((float4*)dh)[i] = acc;
  }
  for (size_t i = nv * 4 + i0; i < n; i += stride) gru_bwd_reset1(drh[i], r[i], h[i], dr[i], dh[i]);
}

// ---- weight gradient of a single-input-channel k x k convolution (BasicMotionEncoder.convd1, 7x7, update.py:78) -----
// dw[co, ky, kx] = sum_{b,y,x} g[b,co,y,x] * x[b,0,y+ky-p,x+kx-p].  One block per (co, ky): every thread adds its
// positions (a fixed stride) into k accumulators, then a fixed-order tree over the block.  No atomics.
template <int K>
__global__ __launch_bounds__(256) void conv2d_1in_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                               float* __restrict__ dw, int B, int H, int W, int Cout) {
  __shared__ float red[K][256];
  const int co = blockIdx.x, ky = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)H * W, total = (size_t)B * plane;
  float acc[K];
#pragma unroll
  for (int kx = 0; kx < K; ++kx) acc[kx] = 0.f;
  for (size_t i = tid; i < total; i += 256) {
    const int b = (int)(i / plane), p = (int)(i % plane), y = p / W, xx = p % W;
    const int iy = y + ky - K / 2;
    if (iy < 0 || iy >= H) continue;
    const float gv = g[((size_t)b * Cout + co) * plane + p];
    const float* row = x + (size_t)b * plane + (size_t)iy * W;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
      const int ix = xx + kx - K / 2;
      if (ix >= 0 && ix < W) acc[kx] = fmaf(gv, row[ix], acc[kx]);
    }
  }
#pragma unroll
  for (int kx = 0; kx < K; ++kx) red[kx][tid] = acc[kx];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int kx = 0; kx < K; ++kx) red[kx][tid] += red[kx][tid + s];
    __syncthreads();
  }
  if (tid < K) dw[((size_t)co * K + ky) * K + tid] = red[tid][0];
}

unsigned gru_grid(size_t n) {
  const size_t nb = (n / 4 + 255) / 256 + 1;
  return (unsigned)(nb < 4096 ? nb : 4096);
}

}  // namespace

extern "C" size_t dv_conv2d_wgrad_cat_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout,
                                                       int k) {
  const long long cin = wc_cin(channels, n_inputs);
  if (!wc_valid(cin, B, H, W, Cout, k)) return 0;
  const WcPlan p = wc_plan(B, (int)cin, H, W, Cout, k);
  return (size_t)p.splits * Cout * cin * k * k;
}

extern "C" int dv_conv2d_wgrad_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* g,
                                       float* dw, float* workspace, int B, int H, int W, int Cout, int k,
                                       dv_stream_t stream) {
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(inputs);
  DV_REQUIRE_PTR(channels);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE_PTR(workspace);
  DV_REQUIRE(n_inputs >= 1 && n_inputs <= WC_MAX_INPUTS, DV_ERR_SHAPE);
  const long long cin = wc_cin(channels, n_inputs);
  DV_REQUIRE(wc_valid(cin, B, H, W, Cout, k), DV_ERR_SHAPE);
  for (int i = 0; i < n_inputs; ++i) DV_REQUIRE_PTR(inputs[i]);
  const WcPlan p = wc_plan(B, (int)cin, H, W, Cout, k);
  WcArgs a;
  int off = 0;
  for (int i = 0; i < WC_MAX_INPUTS; ++i) {
    a.src[i] = inputs[i < n_inputs ? i : 0];
    a.coff[i] = i < n_inputs ? off : (int)cin;
    if (i < n_inputs) off += channels[i];
  }
  a.coff[WC_MAX_INPUTS] = (int)cin;
  a.g = g; a.ws = workspace;
  a.B = B; a.Cin = (int)cin; a.H = H; a.W = W; a.Cout = Cout;
  a.nby = p.nby; a.nbx = p.nbx; a.splits = p.splits; a.nbricks = p.nbricks;
  hipStream_t s = (hipStream_t)stream;
  return k == 1 ? wc_launch<WcGeo<1>>(a, dw, s) : wc_launch<WcGeo<3>>(a, dw, s);
}

extern "C" int dv_gru_reset_mul_f32(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(rh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dv_aligned16(r) && dv_aligned16(h) && dv_aligned16(rh))
    hipLaunchKernelGGL(gru_mul_kernel<4>, dim3(gru_grid(n)), dim3(256), 0, s, r, h, rh, n);
  else
    hipLaunchKernelGGL(gru_mul_kernel<1>, dim3(gru_grid(n)), dim3(256), 0, s, r, h, rh, n);
  return dv_launch_status();
}

extern "C" int dv_gru_blend_f32(const float* z, const float* q, const float* h, float* out, size_t n,
                                dv_stream_t stream) {
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dv_aligned16(z) && dv_aligned16(q) && dv_aligned16(h) && dv_aligned16(out))
    hipLaunchKernelGGL(gru_blend_kernel<4>, dim3(gru_grid(n)), dim3(256), 0, s, z, q, h, out, n);
  else
    hipLaunchKernelGGL(gru_blend_kernel<1>, dim3(gru_grid(n)), dim3(256), 0, s, z, q, h, out, n);
  return dv_launch_status();
}

extern "C" int dv_gru_gates_bwd_blend_f32(const float* dh_new, const float* z, const float* q, const float* h,
                                          float* dq_pre, float* dz_pre, float* dh, size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(dh_new);
  DV_REQUIRE_PTR(z);
  DV_REQUIRE_PTR(q);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(dq_pre);
  DV_REQUIRE_PTR(dz_pre);
  DV_REQUIRE_PTR(dh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dv_aligned16(dh_new) && dv_aligned16(z) && dv_aligned16(q) && dv_aligned16(h) && dv_aligned16(dq_pre) &&
      dv_aligned16(dz_pre) && dv_aligned16(dh))
    hipLaunchKernelGGL(gru_bwd_blend_kernel<4>, dim3(gru_grid(n)), dim3(256), 0, s, dh_new, z, q, h, dq_pre, dz_pre, dh, n);
  else
    hipLaunchKernelGGL(gru_bwd_blend_kernel<1>, dim3(gru_grid(n)), dim3(256), 0, s, dh_new, z, q, h, dq_pre, dz_pre, dh, n);
  return dv_launch_status();
}

extern "C" int dv_gru_gates_bwd_reset_f32(const float* drh, const float* r, const float* h, float* dr_pre, float* dh,
                                          size_t n, dv_stream_t stream) {
  DV_REQUIRE_PTR(drh);
  DV_REQUIRE_PTR(r);
  DV_REQUIRE_PTR(h);
  DV_REQUIRE_PTR(dr_pre);
  DV_REQUIRE_PTR(dh);
  DV_REQUIRE(n > 0, DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  if (dv_aligned16(drh) && dv_aligned16(r) && dv_aligned16(h) && dv_aligned16(dr_pre) && dv_aligned16(dh))
    hipLaunchKernelGGL(gru_bwd_reset_kernel<4>, dim3(gru_grid(n)), dim3(256), 0, s, drh, r, h, dr_pre, dh, n);
  else
    hipLaunchKernelGGL(gru_bwd_reset_kernel<1>, dim3(gru_grid(n)), dim3(256), 0, s, drh, r, h, dr_pre, dh, n);
  return dv_launch_status();
}

extern "C" int dv_conv2d_1in_wgrad_f32(const float* x, const float* g, float* dw, int B, int H, int W, int Cout, int k,
                                       dv_stream_t stream) {
  DV_REQUIRE(k == 7, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(g);
  DV_REQUIRE_PTR(dw);
  DV_REQUIRE(B > 0 && H > 0 && W > 0 && Cout > 0 && Cout <= 65535 && (long long)H * W < (1ll << 30), DV_ERR_SHAPE);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(conv2d_1in_wgrad_kernel<7>, dim3((unsigned)Cout, 7), dim3(256), 0, s, x, g, dw, B, H, W, Cout);
  return dv_launch_status();
}
