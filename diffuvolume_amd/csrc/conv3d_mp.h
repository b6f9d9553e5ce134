// The 3x3x3 stride-1 aggregation convolution of mixed-precision training, forward and input gradient, written once for
// the two 16-bit element types of csrc/mp_elem.h (train precisions "f16" and "bf16"):
//   y = conv(r(x), r(w)) (+ bias),   r = T::round: r16 at MpF16 (round to nearest even fp16, subnormals kept, beyond
//   65504: Inf), rb16 at MpBf16 (round to nearest even bfloat16 by the hardware conversion while the operand is staged;
//   NaN stays NaN; a finite float32 above about 3.3895e38 rounds to Inf; operands below 2^-126 may be flushed to zero).
// x, w and y are float32 tensors; both operands are rounded while they are staged, the products (exact in fp32 unless
// they leave the fp32 exponent range) accumulate in fp32 on T::mfma (v_mfma_f32_16x16x32_f16 / _bf16) and y is written
// UNROUNDED.  An operand beyond the element type's range becomes Inf and reaches every output whose window holds it: at
// fp16 the signal torch.amp.GradScaler skips a step on; at bf16 the range is float32's and there is no such signal.
// This header holds the kernel, the staging and the launch helper; csrc/conv3d_f16.hip and csrc/conv3d_bf16.hip each hold
// one instantiation and its extern "C" entry.
//
// The kernel is csrc/conv3d_f16x3.hip with one 16-bit image instead of its hi | lo pair: one MFMA per step instead of
// three, no pre-scaling, no overflow flag, no epilogue beyond a per-channel bias.  Same GEMM view -- M = 16 consecutive
// x of a (z, y) row, N = 16 cout, K-block (32) = 4 taps x 8 input channels: lane (i = lane & 15, kq = lane >> 4) supplies
// the 8 channels of voxel i at tap slot 4 kb + kq as ONE ds_read_b128 from the channels-last LDS image
// [position][8 elements] -- and the same tap pairing (27 taps + 1 dummy with zero weights; the two taps sharing a 16-lane
// LDS group sit a multiple of 16 positions apart, row stride RW = 56: 13 of the 14 pairs are bank-conflict free).
// The dummy slot repeats tap (2,1,2) with zero weights: an Inf there is multiplied by 0, but the real tap 26 has already
// put the same voxel into the same output, so no output turns non-finite that the exact sum keeps finite.
//
// Weights: the module's RAW float32 tensor [Cout,Cin,3,3,3], gathered and rounded per chunk of 8 input channels while
// the chunk is staged (one chunk ahead, in registers, as the activations).  There is no packed image: the training route
// repacked on every call, so a pack launch and its buffer are saved.  `flip` reads the tensor [Cin,Cout,3,3,3] of the
// layer whose input gradient is wanted as w.flip(2,3,4).transpose(0,1).
// Summation order of one output: chunks of 8 channels in ascending order, inside a chunk the 7 K-blocks in order, the
// 32 products of a K-block inside the matrix instruction.  It does not depend on the batch, the grid or the alignment.
#pragma once
#include "mp_elem.h"

namespace {

constexpr int TD = 2, TH = 4, MTX = 3, NT = 2, KC = 8;
constexpr int TW = MTX * 16;
constexpr int IZ = TD + 2, IY = TH + 2, IX = TW + 2;
constexpr int RW = (IX + 7) / 8 * 8;                 // 56: IY*RW and 2*RW are multiples of 16 positions
constexpr int NPOS = IZ * IY * RW;                   // LDS positions (16 B each)
constexpr int NREAL = IZ * IY * IX;                  // positions that carry data
constexpr int KB = 7;                                // k-blocks of 4 tap slots
constexpr int COUT = NT * 16;
constexpr int W_H8 = KB * 4 * COUT;                  // 8-element vectors of weights per chunk
constexpr int ROWS = TD * TH, RPW = ROWS / 4, MT = RPW * MTX;
static_assert((IY * RW) % 16 == 0 && (2 * RW) % 16 == 0, "tap pairing needs 16-position multiples");
static_assert((NPOS + W_H8) * 16 <= 80 * 1024, "two blocks per CU");

// tap slot -> (dz,dy,dx) as 9 dz + 3 dy + dx; slot 27 repeats a tap with zero weights
__host__ __device__ constexpr int slot_tap(int s) {
  // pairs: 9 x [(0,dy,dx),(1,dy,dx)], 3 x [(2,0,dx),(2,2,dx)], [(2,1,0),(2,1,1)], [(2,1,2), dummy]
  if (s < 18) { const int p = s >> 1, dz = s & 1; return (dz * 3 + p / 3) * 3 + p % 3; }
  if (s < 24) { const int p = (s - 18) >> 1, dy = ((s - 18) & 1) * 2; return (2 * 3 + dy) * 3 + p; }
  if (s == 24) return (2 * 3 + 1) * 3 + 0;
  if (s == 25) return (2 * 3 + 1) * 3 + 1;
  return (2 * 3 + 1) * 3 + 2;  // 26 real, 27 dummy
}
__host__ __device__ constexpr int tap_off(int tap) { return ((tap / 9) * IY + (tap / 3) % 3) * RW + tap % 3; }

struct Args {
  const float* in;
  const float* w;        // [Cout][Cin][27], or [Cin][Cout][27] with flip
  const float* bias;
  float* out;
  int B, Cin, D, H, W, Cout;
  int ntx, nty, ntz, nco;
  int flip, vec_store;
};

template <class T>
__global__ __launch_bounds__(256, 2) void conv3d_mp_kernel(Args a) {
  typedef typename T::v8 h8;
  __shared__ __attribute__((aligned(16))) h8 smem[NPOS + W_H8];
  h8* in_s = smem;                 // [pos]
  h8* w_s = smem + NPOS;           // [kb][kq][cout]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 15, kq = lane >> 4;

  unsigned t = dv_xcd_remap(blockIdx.x, gridDim.x);
  const int tx = t % a.ntx; t /= a.ntx;
  const int ty = t % a.nty; t /= a.nty;
  const int tz = t % a.ntz; t /= a.ntz;
  const int tc = t % a.nco;
  const int b = t / a.nco;
  const int x0 = tx * TW, y0 = ty * TH, z0 = tz * TD, co0 = tc * COUT;

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // this wave's rows are (2*wave, 2*wave+1) of the brick and never straddle a z slab (TH even), so
  // every M-tile is a compile-time offset from one base position
  static_assert(RPW == 2 && TH % 2 == 0, "row layout assumed by the A addressing");
  const int abase0 = (((wave * RPW) / TH) * IY + (wave * RPW) % TH) * RW + j;
  int toff[KB];     // position offset of this lane's tap in every k-block
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const int o0 = tap_off(slot_tap(4 * kb)), o1 = tap_off(slot_tap(4 * kb + 1));
    const int o2 = tap_off(slot_tap(4 * kb + 2)), o3 = tap_off(slot_tap(4 * kb + 3));
    toff[kb] = kq == 0 ? o0 : (kq == 1 ? o1 : (kq == 2 ? o2 : o3));
  }
  const int bbase = kq * COUT + j;

  const size_t plane = (size_t)a.H * a.W, vol = (size_t)a.D * plane;
  const float* inb = a.in + (size_t)b * a.Cin * vol;

  // staging plan: thread owns NS brick positions (all 8 channels of each) and NWQ weight vectors (8 channels of one
  // (tap slot, cout) each)
  constexpr int NS = (NREAL + 255) / 256;
  constexpr int NWQ = (W_H8 + 255) / 256;
  unsigned sob[NS];                 // byte offset inside one channel volume (2^31 outside: the buffer load returns 0)
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int r = tid + 256 * i;
    const int zz = r / (IY * IX), r2 = r - zz * (IY * IX);
    const int yy = r2 / IX, xx = r2 - yy * IX;
    const int z = z0 - 1 + zz, y = y0 - 1 + yy, x = x0 - 1 + xx;
    const bool ok = r < NREAL && (unsigned)z < (unsigned)a.D && (unsigned)y < (unsigned)a.H &&
                    (unsigned)x < (unsigned)a.W;
    const unsigned sp = ok ? (unsigned)((z * a.H + y) * a.W + x) : 0u;
    sob[i] = ok ? sp * 4u : 0x80000000u;
  }
  constexpr unsigned NOW = 0xffffffffu;                    // no weight behind this vector: dummy slot, cout tail
  unsigned wob[NWQ];                // float index of the vector's channel 0; the channel stride is wstr
  const unsigned wstr = a.flip ? (unsigned)a.Cout * 27u : 27u;
#pragma unroll
  for (int q = 0; q < NWQ; ++q) {
    const int e = tid + 256 * q;                           // -> (kb*4+kq, cout)
    const int sl = e / COUT, co = co0 + e % COUT;
    const bool ok = e < W_H8 && sl < 27 && co < a.Cout;
    const unsigned tap = (unsigned)slot_tap(sl < 27 ? sl : 26);
    wob[q] = !ok ? NOW : (a.flip ? (unsigned)co * 27u + 26u - tap : (unsigned)co * (unsigned)a.Cin * 27u + tap);
  }
  const int vol_bytes = (int)(vol * sizeof(float));   // < 2^31 (checked by the host)
  float vin[NS][KC];
  float vw[NWQ][KC];
  auto fetch = [&](int c0) {
#pragma unroll
    for (int cl = 0; cl < KC; ++cl) {
      // buffer loads (one descriptor per channel, scalar): zero padding and channel tail from the range check
      const bool cok = (c0 + cl) < a.Cin;
      const uint64_t ba = reinterpret_cast<uint64_t>(inb + (size_t)(cok ? c0 + cl : 0) * vol);
      const uint64_t bu = (uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)ba) |
                          ((uint64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(ba >> 32)) << 32);
      const auto rs = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(bu), 0,
                                                        __builtin_amdgcn_readfirstlane(cok ? vol_bytes : 0), 0x00020000);
#pragma unroll
      for (int i = 0; i < NS; ++i)
        vin[i][cl] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs, (int)sob[i], 0, 0));
#pragma unroll
      for (int q = 0; q < NWQ; ++q)
        vw[q][cl] = (wob[q] != NOW && cok) ? a.w[wob[q] + (unsigned)(c0 + cl) * wstr] : 0.f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
      const int r = tid + 256 * i;
      if (r >= NREAL) continue;
      const int zz = r / (IY * IX), r2 = r - zz * (IY * IX);
      const int lpos = (zz * IY + r2 / IX) * RW + r2 % IX;
      h8 v;
#pragma unroll
      for (int cl = 0; cl < KC; ++cl) v[cl] = T::round(vin[i][cl]);
      in_s[lpos] = v;
    }
#pragma unroll
    for (int q = 0; q < NWQ; ++q) {
      const int e = tid + 256 * q;
      if (e >= W_H8) continue;
      h8 v;
#pragma unroll
      for (int cl = 0; cl < KC; ++cl) v[cl] = T::round(vw[q][cl]);
      w_s[e] = v;
    }
  };

  fetch(0);
  for (int c0 = 0; c0 < a.Cin; c0 += KC) {
    __syncthreads();
    commit();
    __syncthreads();
    if (c0 + KC < a.Cin) fetch(c0 + KC);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      h8 bw[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) bw[n] = w_s[bbase + kb * 4 * COUT + n * 16];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const h8 av = in_s[abase0 + (m / MTX) * RW + (m % MTX) * 16 + toff[kb]];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = T::mfma(av, bw[n], acc[m][n]);
      }
    }
  }

  // epilogue: the bias, 16-byte stores along x where the caller's pointer and W allow them
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int co = co0 + n * 16 + j;
    if (co >= a.Cout) continue;
    const float bi = a.bias ? a.bias[co] : 0.f;
    const size_t cbase = ((size_t)b * a.Cout + co) * vol;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int rr = wave * RPW + m / MTX, xt = m % MTX;
      const int zo = z0 + rr / TH, yo = y0 + rr % TH, xo = x0 + xt * 16 + 4 * kq;
      if (zo >= a.D || yo >= a.H || xo >= a.W) continue;
      const size_t o = cbase + (size_t)zo * plane + (size_t)yo * a.W + xo;
      const float v[4] = {acc[m][n][0] + bi, acc[m][n][1] + bi, acc[m][n][2] + bi, acc[m][n][3] + bi};
      if (a.vec_store) {
        *reinterpret_cast<float4*>(a.out + o) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (xo + r < a.W) a.out[o + r] = v[r];
      }
    }
  }
}

// the checks and the launch of an entry (dv_conv3d_k3s1_f16_f32 / dv_conv3d_k3s1_bf16_f32)
template <class T>
int conv3d_mp_launch(const float* in, const float* w, const float* bias, float* out, int B, int Cin, int D, int H, int W,
                     int Cout, int k, int transpose_flip, dv_stream_t stream) {
  DV_REQUIRE(k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE_PTR(in);
  DV_REQUIRE_PTR(w);
  DV_REQUIRE_PTR(out);
  DV_REQUIRE(B > 0 && Cin > 0 && D > 0 && H > 0 && W > 0 && Cout > 0, DV_ERR_SHAPE);
  DV_REQUIRE(Cout >= 2, DV_ERR_UNSUPPORTED);                                       // the heads keep their float32 kernel
  DV_REQUIRE((unsigned long long)D * H * W * sizeof(float) <= 0x7fffffffull, DV_ERR_SHAPE);   // 31-bit byte offsets in a channel
  DV_REQUIRE((unsigned long long)Cout * Cin * 27 <= 0x7fffffffull, DV_ERR_SHAPE);  // 32-bit weight indices
  Args a;
  a.in = in; a.w = w; a.bias = bias; a.out = out;
  a.B = B; a.Cin = Cin; a.D = D; a.H = H; a.W = W; a.Cout = Cout;
  a.ntx = (W + TW - 1) / TW; a.nty = (H + TH - 1) / TH; a.ntz = (D + TD - 1) / TD; a.nco = (Cout + COUT - 1) / COUT;
  a.flip = transpose_flip != 0;
  a.vec_store = (W % 4 == 0) && dv_aligned16(out);
  const long long blocks = (long long)B * a.nco * a.ntz * a.nty * a.ntx;
  if (blocks <= 0 || blocks > 0x7fffffffLL) return DV_ERR_SHAPE;
  hipLaunchKernelGGL(conv3d_mp_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
  return dv_launch_status();
}

}  // namespace
