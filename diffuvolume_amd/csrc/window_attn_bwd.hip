// Backward of K6 (csrc/window_attn.hip): the 4x4x4 window multi-head self-attention of the hourglass bottleneck in training.
// What autograd computes for attention_block.forward (SceneFlow/models/submodule.py:398-429, applied by the hourglass of
// SceneFlow/models/acv_ddim.py:56-93) with respect to x, qkv_3d.weight / .bias and final1x1.weight / .bias.
//
// Stage 1, one block of 4 waves per window (the forward's XCD-aware window order).  The window's tokens X and the output
// gradient dY live in registers as MFMA A fragments (zero at padded tokens); heads are taken two at a time like the
// forward.  Per group of two heads:
//   QKV = X Wg^T + b  -> q_s          (the forward's GEMM)         dOm = dY Wp[:, 16g..16g+15]  -> do_s
//   per head, a wave owning 16 queries: S^T = K Q^T, the forward's max / exp / sum (dv_exp_le0) -> P = e / sum;
//     O = (e V) / sum (the forward's statement; kept for dWp), dP^T = V dO^T, Dq = rowsum(P dP) (= rowsum(dO O)),
//     dS = 8^-0.5 P (dP - Dq), dQ = dS K -- all in the forward's transposed layout, nothing leaves the wave;
//   dV = P^T dO and dK = dS^T Q sum over the queries of all four waves: P and dS go through LDS (p_s, ds_s, 20 KiB each)
//     and the wave that owns keys 16w..16w+15 forms its rows with the 64 queries in ascending MFMA steps;
//   dX += dQKV_g Wg  accumulated in registers over the groups (a wave reads only the dQKV rows it wrote itself).
// Padded tokens are real keys: their rows of dK / dV exist and enter the bias gradient (the sum over the window's 64 rows
// of dQKV, one partial per window), but are neither stored (X = 0 there: no dWqkv) nor given a dX.
// Stage 1 writes dx, and channel-major into the workspace Om [B,128,D,H,W] and dQKV [B,384,D,H,W] at unpadded tokens.
// Stage 2: dWqkv = sum_tokens dQKV^T X and dWp = sum_tokens dY^T Om as split-K GEMMs over the tokens on the fp32 MFMA with
// the splits summed in split order (dv_conv3d_wgrad_f32 at k = 1 computes the same products, but its 32 x 32 tiles reach
// 0.08 of the MFMA peak at these sizes); dbqkv adds the per-window partials, dbp the elements of dY, both in a fixed
// order in double.  No atomics anywhere; every output element is written once.
#include "dv_common.h"

namespace {

constexpr int C = 128, HEADS = 16, HD = 8, TOK = 64, F3 = 3 * C;
constexpr int LDW = 130;                        // w_s[row][k], as the forward
constexpr int GH2 = 2, GF2 = 3 * GH2 * HD;      // 48 qkv features per group
constexpr int GC = GH2 * HD;                    // 16 merged channels per group
constexpr int LDQ2 = 52;                        // q_s / dq_s [tok][q 16 | k 16 | v 16]
constexpr int WROWS = 48;
constexpr int LDP = 18;                         // wp_s[co][16 channels of the group]
constexpr int LDT = 17;                         // do_s[tok][16 channels]
constexpr int LDS_P = 80;                       // p_s / ds_s [query][key]: == 16 (mod 32), the two k-rows of a half differ by 16 banks
constexpr int W2 = WROWS * LDW, Q2 = TOK * LDQ2, P2 = C * LDP, T2 = TOK * LDT, S2 = TOK * LDS_P;
constexpr int SMEM_FLOATS = W2 + 2 * Q2 + P2 + T2 + 2 * S2;
constexpr int NWQ = WROWS * 32 / 256, NPQ = C * 4 / 256;
static_assert(SMEM_FLOATS * 4 <= 160 * 1024, "one block per CU");
static_assert(LDS_P % 4 == 0, "16-byte rows of p_s / ds_s");

struct BwdArgs {
  const float* x;
  const float* qkv_w;   // [384][128]
  const float* qkv_b;   // [384]
  const float* proj_w;  // [128][128]
  const float* dout;
  float* dx;            // or nullptr
  float* om;            // workspace [B][128][vol] or nullptr
  float* dqkv;          // workspace [B][384][vol] or nullptr
  float* dbias;         // workspace [windows][384] or nullptr
  int B, D, H, W, nd, nh, nw;
  int mask_on;
  int vec_dx, vec_ws;
};

// 4 values of one channel along w at (row gy, columns w0..w0+3): one 16-byte store or guarded element stores
__device__ __forceinline__ void store4(float* dst, bool vec, int w0, int W, float a, float b, float c, float d) {
  if (vec) {
    *reinterpret_cast<float4*>(dst) = make_float4(a, b, c, d);
  } else {
    if (w0 + 0 < W) dst[0] = a;
    if (w0 + 1 < W) dst[1] = b;
    if (w0 + 2 < W) dst[2] = c;
    if (w0 + 3 < W) dst[3] = d;
  }
}

__global__ __launch_bounds__(256, 1) void window_attn_bwd_kernel(BwdArgs a) {
  __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];
  float* w_s = smem;
  float* q_s = w_s + W2;
  float* dq_s = q_s + Q2;
  float* wp_s = dq_s + Q2;
  float* do_s = wp_s + P2;
  float* p_s = do_s + T2;
  float* ds_s = p_s + S2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;

  const unsigned win = dv_xcd_remap(blockIdx.x, gridDim.x);
  unsigned t = win;
  const int ww = t % a.nw; t /= a.nw;
  const int wh = t % a.nh; t /= a.nh;
  const int wd = t % a.nd;
  const int b = t / a.nd;
  const int d0 = wd * 4, h0 = wh * 4, w0 = ww * 4;
  const size_t plane = (size_t)a.H * a.W, vol = (size_t)a.D * plane;

  float4 wq[NWQ], wpq[NPQ];
  auto fetch_w = [&](int g) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NWQ; ++i) {
      const int e = tid + 256 * i, r = e >> 5, q = e & 31;              // r = row 0..47 = which*16 + feature
      const int which = r >> 4, f = r & 15;
      wq[i] = reinterpret_cast<const float4*>(a.qkv_w + (size_t)(which * C + g * GC + f) * C)[q];
    }
#pragma unroll
    for (int i = 0; i < NPQ; ++i) {
      const int e = tid + 256 * i, co = e >> 2, q = e & 3;              // projection weights [co][16g + 4q .. +3]
      wpq[i] = reinterpret_cast<const float4*>(a.proj_w + (size_t)co * C + g * GC)[q];
    }
  };
  auto store_w = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NWQ; ++i) {
      const int e = tid + 256 * i, r = e >> 5, q = e & 31;
      float2* d = reinterpret_cast<float2*>(w_s + r * LDW + 4 * q);
      d[0] = make_float2(wq[i].x, wq[i].y);
      d[1] = make_float2(wq[i].z, wq[i].w);
    }
#pragma unroll
    for (int i = 0; i < NPQ; ++i) {
      const int e = tid + 256 * i, co = e >> 2, q = e & 3;
      float2* d = reinterpret_cast<float2*>(wp_s + co * LDP + 4 * q);
      d[0] = make_float2(wpq[i].x, wpq[i].y);
      d[1] = make_float2(wpq[i].z, wpq[i].w);
    }
  };
  fetch_w(0);

  // A fragments of this wave's 16 tokens (ld = wave, lh = j >> 2, lw = j & 3): channel ks*4 + kq, of x and of dY
  float xa[C / 4], ya[C / 4];
  {
    const int gy = h0 + (j >> 2), gx = w0 + (j & 3);
    const bool in = gy < a.H && gx < a.W;
    const size_t off = (size_t)b * C * vol + (size_t)(d0 + wave) * plane + (size_t)(in ? gy : 0) * a.W + (in ? gx : 0) +
                       (size_t)kq * vol;
    const float* sx = a.x + off;
    const float* sy = a.dout + off;
#pragma unroll
    for (int ks = 0; ks < C / 4; ++ks) {
      xa[ks] = in ? sx[(size_t)ks * 4 * vol] : 0.f;
      ya[ks] = in ? sy[(size_t)ks * 4 * vol] : 0.f;
    }
  }

  f32x4 dxacc[C / 16];                                 // dX accumulators: 16 tokens x 128 channels
#pragma unroll
  for (int n = 0; n < C / 16; ++n) dxacc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // where this lane's (token row 4*kq + r, r = 0..3 = lw) results go in a channel-major [.., D, H, W] tensor
  const int gy_out = h0 + kq;
  const bool row_in = gy_out < a.H;
  const size_t pos_out = (size_t)(d0 + wave) * plane + (size_t)gy_out * a.W + w0;
  const float scale = 0.35355339059327379f;  // 8^-0.5

  for (int g = 0; g < HEADS / GH2; ++g) {
    __syncthreads();                                   // the previous group is done with every LDS tile
    store_w();
    __syncthreads();
    if (g + 1 < HEADS / GH2) fetch_w(g + 1);
    {   // GEMM1 (the forward's): q_s[tok][f] = x[tok][:] . Wg[f][:] + b
      f32x4 acc[GF2 / 16];
#pragma unroll
      for (int n = 0; n < GF2 / 16; ++n) acc[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float* bp = w_s + j * LDW + kq;
#pragma unroll
      for (int ks = 0; ks < C / 4; ++ks)
#pragma unroll
        for (int n = 0; n < GF2 / 16; ++n)
          acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks], bp[n * 16 * LDW + ks * 4], acc[n], 0, 0, 0);
#pragma unroll
      for (int n = 0; n < GF2 / 16; ++n) {
        const int f = n * 16 + j;
        const float bias = a.qkv_b[n * C + g * GC + j];
#pragma unroll
        for (int r = 0; r < 4; ++r) q_s[(wave * 16 + 4 * kq + r) * LDQ2 + f] = acc[n][r] + bias;
      }
    }
    {   // dOm of the group: do_s[tok][c] = sum_co dY[tok][co] Wp[co][16g + c]
      f32x4 d0acc = {0.f, 0.f, 0.f, 0.f}, d1acc = {0.f, 0.f, 0.f, 0.f};
      const float* bp = wp_s + kq * LDP + j;           // B: row co = 4ks + kq, column c = j
#pragma unroll
      for (int ks = 0; ks < C / 4; ks += 2) {
        d0acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[ks], bp[ks * 4 * LDP], d0acc, 0, 0, 0);
        d1acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[ks + 1], bp[(ks + 1) * 4 * LDP], d1acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) do_s[(wave * 16 + 4 * kq + r) * LDT + j] = d0acc[r] + d1acc[r];
    }
    __syncthreads();
#pragma unroll 1
    for (int hd = 0; hd < GH2; ++hd) {
      const int hoff = hd * HD;
      const int qrow = (wave * 16 + j) * LDQ2;
      {   // this wave's 16 queries: lane (query j, k-group kq) holds the keys 16*kt + 4*kq + i
        f32x4 sc[4], dp[4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          sc[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
          dp[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
          const float* kp = q_s + (kt * 16 + j) * LDQ2 + GC + hoff + kq;             // A: key row j, dim 4s + kq
          const float* vp = q_s + (kt * 16 + j) * LDQ2 + 2 * GC + hoff + kq;         // A: value row j, dim 4s + kq
          const float* qp = q_s + qrow + hoff + kq;                                  // B: query column j
          const float* gp = do_s + (wave * 16 + j) * LDT + hoff + kq;                // B: dO of query j
#pragma unroll
          for (int s2 = 0; s2 < HD / 4; ++s2) {
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[4 * s2], qp[4 * s2], sc[kt], 0, 0, 0);
            dp[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[4 * s2], gp[4 * s2], dp[kt], 0, 0, 0);
          }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            float v = sc[kt][i] * scale;
            if (a.mask_on) {
              const int k = kt * 16 + 4 * kq + i, q = wave * 16 + j;
              const bool k_pad = (h0 + ((k >> 2) & 3) >= a.H) || (w0 + (k & 3) >= a.W);
              const bool qp_ = (h0 + ((q >> 2) & 3) >= a.H) || (w0 + (q & 3) >= a.W);
              if (k_pad != qp_) v += -1000.0f;
            }
            sc[kt][i] = v;
            mx = fmaxf(mx, v);
          }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        float sum = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[kt][i] = dv_exp_le0(sc[kt][i] - mx);
            sum += sc[kt][i];
          }
        sum += __shfl_xor(sum, 16);
        sum += __shfl_xor(sum, 32);
        if (a.om != nullptr) {   // O = (e V) / sum, the forward's statement, for dWp
          f32x4 o = {0.f, 0.f, 0.f, 0.f};
          const float* vp = q_s + 2 * GC + hoff + (j & 7);
#pragma unroll
          for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float bv = vp[(kt * 16 + 4 * kq + i) * LDQ2];
              o = __builtin_amdgcn_mfma_f32_16x16x4f32(sc[kt][i], bv, o, 0, 0, 0);
            }
          float ov[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) ov[i] = o[i] / __shfl(sum, 4 * kq + i);
          if (j < HD && row_in)
            store4(a.om + ((size_t)b * C + g * GC + hoff + j) * vol + pos_out, a.vec_ws, w0, a.W, ov[0], ov[1], ov[2], ov[3]);
        }
        // P, Dq = rowsum(P dP), dS = scale P (dP - Dq)
        float dq_row = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[kt][i] = sc[kt][i] / sum;
            dq_row = fmaf(sc[kt][i], dp[kt][i], dq_row);
          }
        dq_row += __shfl_xor(dq_row, 16);
        dq_row += __shfl_xor(dq_row, 32);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) dp[kt][i] = scale * (sc[kt][i] * (dp[kt][i] - dq_row));
        // P and dS of the head -> LDS, [query][key]
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const int o = (wave * 16 + j) * LDS_P + kt * 16 + 4 * kq;
          *reinterpret_cast<float4*>(p_s + o) = make_float4(sc[kt][0], sc[kt][1], sc[kt][2], sc[kt][3]);
          *reinterpret_cast<float4*>(ds_s + o) = make_float4(dp[kt][0], dp[kt][1], dp[kt][2], dp[kt][3]);
        }
        // dQ = dS K: M = this wave's queries, N = the head's 8 dims (columns 8..15 idle), K = keys
        f32x4 dq = {0.f, 0.f, 0.f, 0.f};
        const float* kp = q_s + GC + hoff + (j & 7);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float bv = kp[(kt * 16 + 4 * kq + i) * LDQ2];
            dq = __builtin_amdgcn_mfma_f32_16x16x4f32(dp[kt][i], bv, dq, 0, 0, 0);
          }
        if (j < HD) {
#pragma unroll
          for (int i = 0; i < 4; ++i) dq_s[(wave * 16 + 4 * kq + i) * LDQ2 + hoff + j] = dq[i];
          if (a.dqkv != nullptr && row_in)
            store4(a.dqkv + ((size_t)b * F3 + g * GC + hoff + j) * vol + pos_out, a.vec_ws, w0, a.W, dq[0], dq[1], dq[2],
                   dq[3]);
        }
      }
      __syncthreads();                                 // p_s / ds_s of all 64 queries are in place
      {   // this wave's 16 keys (16*wave + ..): dV = P^T dO, dK = dS^T Q over the 64 queries, 4 per MFMA step in ascending order
        f32x4 dv = {0.f, 0.f, 0.f, 0.f}, dk = {0.f, 0.f, 0.f, 0.f};
        const float* pp = p_s + kq * LDS_P + wave * 16 + j;            // A: key j, query 4s + kq
        const float* sp = ds_s + kq * LDS_P + wave * 16 + j;
        const float* gp = do_s + kq * LDT + hoff + (j & 7);            // B: dO[query 4s + kq][dim j]
        const float* qp = q_s + kq * LDQ2 + hoff + (j & 7);            // B: Q[query 4s + kq][dim j]
#pragma unroll
        for (int s = 0; s < TOK / 4; ++s) {
          dv = __builtin_amdgcn_mfma_f32_16x16x4f32(pp[4 * s * LDS_P], gp[4 * s * LDT], dv, 0, 0, 0);
          dk = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[4 * s * LDS_P], qp[4 * s * LDQ2], dk, 0, 0, 0);
        }
        if (j < HD) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            dq_s[(wave * 16 + 4 * kq + r) * LDQ2 + GC + hoff + j] = dk[r];
            dq_s[(wave * 16 + 4 * kq + r) * LDQ2 + 2 * GC + hoff + j] = dv[r];
          }
          if (a.dqkv != nullptr && row_in) {
            store4(a.dqkv + ((size_t)b * F3 + C + g * GC + hoff + j) * vol + pos_out, a.vec_ws, w0, a.W, dk[0], dk[1],
                   dk[2], dk[3]);
            store4(a.dqkv + ((size_t)b * F3 + 2 * C + g * GC + hoff + j) * vol + pos_out, a.vec_ws, w0, a.W, dv[0], dv[1],
                   dv[2], dv[3]);
          }
        }
      }
      __syncthreads();                                 // p_s / ds_s may be overwritten; dq_s of this head is complete
    }
    if (a.dbias != nullptr && tid < GF2) {   // the window's bias partial: the 64 rows of dQKV in ascending order (padded rows too)
      float s = dq_s[tid];
#pragma unroll 8
      for (int r = 1; r < TOK; ++r) s += dq_s[r * LDQ2 + tid];
      a.dbias[(size_t)win * F3 + (tid >> 4) * C + g * GC + (tid & 15)] = s;
    }
    if (a.dx != nullptr) {   // dX += dQKV_g Wg: A = this wave's own rows of dq_s, B = w_s[feature][channel]
      const float* ap = dq_s + (wave * 16 + j) * LDQ2 + kq;
      const float* bp = w_s + kq * LDW + j;
#pragma unroll
      for (int s = 0; s < GF2 / 4; ++s) {
        const float av = ap[4 * s];
#pragma unroll
        for (int n = 0; n < C / 16; ++n)
          dxacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bp[4 * s * LDW + n * 16], dxacc[n], 0, 0, 0);
      }
    }
  }

  if (a.dx != nullptr && row_in) {
#pragma unroll
    for (int n = 0; n < C / 16; ++n)
      store4(a.dx + ((size_t)b * C + n * 16 + j) * vol + pos_out, a.vec_dx, w0, a.W, dxacc[n][0], dxacc[n][1], dxacc[n][2],
             dxacc[n][3]);
  }
}

// Stage 2: dW[m][n] = sum over tokens A[b][m][s] B[b][n][s] for channel-major operands (A = dQKV [B,384,S] with B = x, or
// A = dY with B = Om; S = D*H*W), n < 128.  Split-K over chunks of 32 tokens (a chunk lies inside one batch item): a block
// owns 128 rows m x 128 columns n and a contiguous range of chunks, four waves of 64 x 64 each (16 accumulators); both
// tiles are staged [row][32 tokens] with the next chunk's global loads in flight during the MFMA steps.  Every split writes
// its partial [M][128]; dv_splitk_sum adds the splits in split order.  Row stride 34 == 2 (mod 32): the banks
// 2j + kq of a half-wave are distinct.
constexpr int GT = 128, GK = 32, LDG = GK + 2;
constexpr int GQ = GT * GK / 4 / 256;             // float4 per thread and tile: 4
constexpr int Z_QKV = 64, Z_PROJ = 128;           // splits at most: 3 x 64 and 1 x 128 blocks

struct GemmArgs {
  const float* a;       // [B][M][S]
  const float* b;       // [B][128][S]
  float* part;          // [Z][M][128]
  int M, Z, vec;
  long long S, cpi, T;  // tokens per item, chunks per item, chunks in all
};

__global__ __launch_bounds__(256, 2) void attn_wgrad_kernel(GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float as[GT * LDG];
  __shared__ __attribute__((aligned(16))) float bs[GT * LDG];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;
  const int mt = blockIdx.x, z = blockIdx.y;
  const int wm = wave & 1, wn = wave >> 1;

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto ld4 = [&](const float* p, long long s) __attribute__((always_inline)) {
    if (g.vec) return s < g.S ? *reinterpret_cast<const float4*>(p + s) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 v;
    v.x = s + 0 < g.S ? p[s + 0] : 0.f;
    v.y = s + 1 < g.S ? p[s + 1] : 0.f;
    v.z = s + 2 < g.S ? p[s + 2] : 0.f;
    v.w = s + 3 < g.S ? p[s + 3] : 0.f;
    return v;
  };
  float4 ra[GQ], rb[GQ];
  auto fetch = [&](long long c) __attribute__((always_inline)) {
    const long long b = c / g.cpi, s0 = (c % g.cpi) * GK;
    const float* ap = g.a + ((size_t)b * g.M + (size_t)mt * GT) * (size_t)g.S;
    const float* bp = g.b + (size_t)b * GT * (size_t)g.S;
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
      const int e = tid + 256 * i, r = e >> 3, q = e & 7;
      ra[i] = ld4(ap + (size_t)r * g.S, s0 + 4 * q);
      rb[i] = ld4(bp + (size_t)r * g.S, s0 + 4 * q);
    }
  };
  auto store = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < GQ; ++i) {
      const int e = tid + 256 * i, r = e >> 3, q = e & 7;
      float2* da = reinterpret_cast<float2*>(as + r * LDG + 4 * q);
      da[0] = make_float2(ra[i].x, ra[i].y);
      da[1] = make_float2(ra[i].z, ra[i].w);
      float2* db = reinterpret_cast<float2*>(bs + r * LDG + 4 * q);
      db[0] = make_float2(rb[i].x, rb[i].y);
      db[1] = make_float2(rb[i].z, rb[i].w);
    }
  };

  const long long c0 = g.T * z / g.Z, c1 = g.T * (z + 1) / g.Z;
  if (c0 < c1) fetch(c0);
  for (long long c = c0; c < c1; ++c) {
    __syncthreads();                                   // the previous chunk's reads are done
    store();
    __syncthreads();
    if (c + 1 < c1) fetch(c + 1);
    const float* ap = as + (64 * wm + j) * LDG + kq;
    const float* bp = bs + (64 * wn + j) * LDG + kq;
#pragma unroll
    for (int ks = 0; ks < GK / 4; ++ks) {
      float av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        av[i] = ap[i * 16 * LDG + 4 * ks];
        bv[i] = bp[i * 16 * LDG + 4 * ks];
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi], bv[ni], acc[mi][ni], 0, 0, 0);
    }
  }
  // D layout: row m = 4 * kq + r, column n = j
  float* out = g.part + ((size_t)z * g.M + (size_t)mt * GT) * GT;
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(size_t)(64 * wm + 16 * mi + 4 * kq + r) * GT + 64 * wn + 16 * ni + j] = acc[mi][ni][r];
}

void launch_wgrad(const float* a, const float* b, float* part, float* dw, int M, int zmax, int B, long long S,
                  hipStream_t st) {
  GemmArgs g;
  g.a = a; g.b = b; g.part = part; g.M = M; g.S = S;
  g.cpi = (S + GK - 1) / GK;
  g.T = (long long)B * g.cpi;
  g.Z = (int)(g.T < zmax ? g.T : zmax);
  g.vec = (S % 4 == 0) && dv_aligned16(a) && dv_aligned16(b);
  hipLaunchKernelGGL(attn_wgrad_kernel, dim3((unsigned)(M / GT), (unsigned)g.Z), dim3(256), 0, st, g);
  dv_splitk_sum(part, dw, (long long)M * GT, g.Z, st);
}

size_t wgrad_splits(int B, long long S, int zmax) {
  const long long T = (long long)B * ((S + GK - 1) / GK);
  return (size_t)(T < zmax ? T : zmax);
}

// dbqkv[f] = sum over the windows of their partials: one wave per feature, lane l takes windows l, l + 64, ... in ascending
// order, then the lanes by halving shuffles, in double.
__global__ __launch_bounds__(DV_WAVE) void attn_bwd_bias_kernel(const float* __restrict__ part, float* __restrict__ dqkv_b,
                                                                long long nwin) {
  const int f = blockIdx.x, lane = threadIdx.x;
  double s = 0.0;
  for (long long p = lane; p < nwin; p += DV_WAVE) s += (double)part[(size_t)p * F3 + f];
#pragma unroll
  for (int off = DV_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, DV_WAVE);
  if (lane == 0) dqkv_b[f] = (float)s;
}

// dbp[co] = sum over b and positions of dY: one block per channel; a thread takes positions tid, tid + 256, ... of every
// batch item in ascending order, then the lanes by halving shuffles and the four waves in ascending order, in double.
__global__ __launch_bounds__(256) void attn_bwd_dbp_kernel(const float* __restrict__ dout, float* __restrict__ dproj_b, int B,
                                                           long long vol) {
  __shared__ double red[4];
  const int co = blockIdx.x, tid = threadIdx.x;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* src = dout + ((size_t)b * C + co) * (size_t)vol;
    for (long long p = tid; p < vol; p += 256) s += (double)src[p];
  }
#pragma unroll
  for (int off = DV_WAVE / 2; off > 0; off >>= 1) s += __shfl_down(s, off, DV_WAVE);
  if ((tid & (DV_WAVE - 1)) == 0) red[tid / DV_WAVE] = s;
  __syncthreads();
  if (tid == 0) dproj_b[co] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

struct BwdWs {
  size_t om, dqkv, dbias, wg_qkv, wg_proj, total;   // offsets in floats
};

bool bwd_workspace(int B, int Cc, int D, int H, int W, int heads, BwdWs* out) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || D % 4 != 0 || Cc != C || heads != HEADS) return false;
  const size_t vol = (size_t)D * H * W;
  const size_t nwin = (size_t)B * (D / 4) * ((H + 3) / 4) * ((W + 3) / 4);
  const size_t wq = wgrad_splits(B, (long long)vol, Z_QKV) * F3 * C;
  const size_t wp = wgrad_splits(B, (long long)vol, Z_PROJ) * C * C;
  BwdWs w;
  w.om = 0;
  w.dqkv = w.om + (size_t)B * C * vol;
  w.dbias = w.dqkv + (size_t)B * F3 * vol;
  w.wg_qkv = w.dbias + nwin * F3;
  w.wg_proj = w.wg_qkv + wq;
  w.total = w.wg_proj + wp;
  *out = w;
  return true;
}

}  // namespace

extern "C" size_t dv_window_attn3d_bwd_workspace_floats(int B, int Cc, int D, int H, int W, int heads) {
  BwdWs w;
  return bwd_workspace(B, Cc, D, H, W, heads, &w) ? w.total : 0;
}

extern "C" int dv_window_attn3d_bwd_f32(const float* x, const float* qkv_w, const float* qkv_b, const float* proj_w,
                                        const float* dout, float* dx, float* dqkv_w, float* dqkv_b, float* dproj_w,
                                        float* dproj_b, float* workspace, int B, int Cc, int D, int H, int W, int heads,
                                        dv_stream_t stream) {
  DV_REQUIRE_PTR(x);
  DV_REQUIRE_PTR(qkv_w);
  DV_REQUIRE_PTR(qkv_b);
  DV_REQUIRE_PTR(proj_w);
  DV_REQUIRE_PTR(dout);
  DV_REQUIRE(dx != nullptr || dqkv_w != nullptr || dqkv_b != nullptr || dproj_w != nullptr || dproj_b != nullptr,
             DV_ERR_NULL);
  DV_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, DV_ERR_SHAPE);
  DV_REQUIRE(Cc == C && heads == HEADS, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(D % 4 == 0, DV_ERR_SHAPE);
  DV_REQUIRE(dv_aligned16(qkv_w) && dv_aligned16(proj_w), DV_ERR_ALIGN);
  const bool need_ws = dqkv_w != nullptr || dqkv_b != nullptr || dproj_w != nullptr;    // dproj_b reads dout alone
  DV_REQUIRE(workspace != nullptr || !need_ws, DV_ERR_NULL);
  BwdWs w;
  const long long blocks = (long long)B * (D / 4) * ((H + 3) / 4) * ((W + 3) / 4);
  DV_REQUIRE(blocks <= 0x7fffffffLL && bwd_workspace(B, Cc, D, H, W, heads, &w), DV_ERR_SHAPE);
  hipStream_t st = (hipStream_t)stream;
  if (dx != nullptr || need_ws) {
    BwdArgs a;
    a.x = x; a.qkv_w = qkv_w; a.qkv_b = qkv_b; a.proj_w = proj_w; a.dout = dout; a.dx = dx;
    a.om = dproj_w != nullptr ? workspace + w.om : nullptr;
    a.dqkv = dqkv_w != nullptr ? workspace + w.dqkv : nullptr;
    a.dbias = dqkv_b != nullptr ? workspace + w.dbias : nullptr;
    a.B = B; a.D = D; a.H = H; a.W = W;
    a.nd = D / 4; a.nh = (H + 3) / 4; a.nw = (W + 3) / 4;
    a.mask_on = (H % 4 != 0) && (W % 4 != 0);
    a.vec_dx = (W % 4 == 0) && dv_aligned16(dx);
    a.vec_ws = (W % 4 == 0) && dv_aligned16(workspace);
    hipLaunchKernelGGL(window_attn_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    const int rc = dv_launch_status();
    if (rc != DV_OK) return rc;
  }
  const long long S = (long long)D * H * W;
  if (dqkv_w != nullptr) launch_wgrad(workspace + w.dqkv, x, workspace + w.wg_qkv, dqkv_w, F3, Z_QKV, B, S, st);
  if (dproj_w != nullptr) launch_wgrad(dout, workspace + w.om, workspace + w.wg_proj, dproj_w, C, Z_PROJ, B, S, st);
  if (dqkv_b != nullptr)
    hipLaunchKernelGGL(attn_bwd_bias_kernel, dim3(F3), dim3(DV_WAVE), 0, st, workspace + w.dbias, dqkv_b, blocks);
  if (dproj_b != nullptr)
    hipLaunchKernelGGL(attn_bwd_dbp_kernel, dim3(C), dim3(256), 0, st, dout, dproj_b, B, (long long)D * H * W);
  return dv_launch_status();
}
