// K13: the 2-D convolutions of IGEV's update block in 16-bit mixed precision (KITTI15/core/update.py:26-142 run inside
// `autocast(enabled=self.args.mixed_precision)`, igev_stereo_ddim.py:242-246; in training train_stereo.py:146-173), as a
// direct implicit GEMM on the 16x16x32 matrix instruction, written once for the two element types of csrc/mp_elem.h:
// MpF16 (fp16 autocast, train precision "f16", v_mfma_f32_16x16x32_f16) and MpBf16 (train precision "bf16",
// v_mfma_f32_16x16x32_bf16).  This header holds the body of the kernel, the K-split reduce, the weight packer, the
// checks and the launch; csrc/conv2d_f16.hip and csrc/conv2d_bf16.hip each hold the kernels of one instantiation and
// its extern "C" entries.
//
// Rounding contract (what autocast does to nn.Conv2d and the elementwise ops after it), r = T::round (r16: round to
// nearest even fp16, beyond 65504 Inf; rb16: round to nearest even bfloat16 by the hardware conversion, NaN stays NaN, a
// finite float32 above about 3.3895e38 rounds to Inf, operands below 2^-126 may be flushed to zero): input, weight and
// bias are rounded, the products accumulate in fp32, the convolution's output is rounded; every elementwise op of the
// fused epilogue rounds its result again (`cvt f32->16 bit->f32`):
//   v = r(acc + r(bias));  v = r(v + residual);  v = r(act(v));  v = r(v * mul);
//   GRU blend (update.py:39, `(1-z)*h + z*q`):  v = r(r(r(1 - z) * h) + r(z * v)).
// Storage stays fp32 (16-bit-exact values): sources are read as fp32 and rounded while they are staged, so a pooled or
// interpolated tensor gets the value the reference's 16-bit pool / interpolation would have stored.  No Winograd: its
// transforms in 16 bits would add error the reference does not have.
//
// GEMM view: M = 16 consecutive x of an output row, N = 16 output channels, K = 32 input channels of one tap.  A block
// owns 4 rows x 64 columns x (NT * 16) output channels, one row per wave (4 M tiles x NT N tiles, 4*NT accumulators).
// Per chunk of 32 input channels the haloed brick (4 + k - 1) x (64 + k - 1) is staged channels-last in LDS as 16-bit
// elements ([pixel][48 halves]: a 16-lane ds_read_b128 group is bank-conflict free at that stride) and the chunk's packed
// weights ([tap][n tile][lane][8 halves], the B fragment layout) are copied next to it.  The next chunk's global loads
// are issued before the current chunk's MFMAs (register prefetch); two blocks per CU.  Sources are the same virtual
// concatenation of up to four tensors as dv_conv2d_cat_f32 (channel counts need not be multiples of the chunk).  "Half"
// is one 16-bit element of either type: the layouts, the sizes and the launch choice do not depend on the type.
//
// Pair launch: one weight set of Cout1 + Cout2 channels (ConvGRU's convz | convr), channels < Cout1 go to the first
// output with its residual / mul, the others to the second.  K-split: `kslices` blocks share an output tile, each sums a
// contiguous range of chunks into scratch; a second kernel adds the slices in a fixed order and applies the epilogue.
#pragma once
#include "mp_elem.h"

namespace {

constexpr int TH = 4, TW = 64, MT = TW / 16, KC = 32, CS = 48;

template <class T>
__device__ __forceinline__ float mp_r(float v) { return (float)T::round(v); }

struct MpConvArgs {
  const float* src[4];
  int cbeg[5];             // prefix sums of the source channel counts; cbeg[nsrc] = Cin
  int nsrc;
  const void* wpk;         // [chunk][tap][n16][lane 64][8] elements of the instantiation's type
  const float* bias;       // [Ctot] or null
  const float* res[2];     // per output head: [B,C_g,H,W] or null
  const float* mul[2];
  float* out[2];
  const float* blend_z;    // head 0 only: v = (1-z)*h + z*v
  const float* blend_h;
  float* scratch;          // K-split partials [ks][B,Ctot,H,W]
  int ks;
  int B, H, W, Cin, C1, Ctot, n16, nchunks, ntx, nty, nnb;
  int act;
};

template <int KS>
struct Geo {
  static constexpr int P = KS / 2, LH = TH + KS - 1, LW = TW + KS - 1;
  static constexpr int ITEMS = 4 * LH * LW;                  // 8-channel groups of the brick
  static constexpr int IPT = (ITEMS + 255) / 256;            // per thread
  static constexpr int IN_H = LH * LW * CS;                  // halves
};

// One output value through the rounding chain of the contract.  co in [0, Ctot); i = offset inside the head's tensor.
template <class T>
__device__ __forceinline__ void epilogue_store(const MpConvArgs& a, int head, size_t i, float bias, float v) {
  const float* res = head ? a.res[1] : a.res[0];
  const float* mul = head ? a.mul[1] : a.mul[0];
  float* out = head ? a.out[1] : a.out[0];
  v = mp_r<T>(v + bias);
  if (res) v = mp_r<T>(v + res[i]);
  switch (a.act) {
    case DV_ACT_RELU: v = fmaxf(v, 0.0f); break;                 // exact on 16-bit values
    case DV_ACT_SIGMOID: v = mp_r<T>(dv_sigmoid(v)); break;
    case DV_ACT_TANH: v = mp_r<T>(dv_tanh(v)); break;
    default: break;
  }
  if (mul) v = mp_r<T>(v * mul[i]);
  if (head == 0 && a.blend_z) {
    const float z = a.blend_z[i], h = a.blend_h[i];
    v = mp_r<T>(mp_r<T>(mp_r<T>(1.0f - z) * h) + mp_r<T>(z * v));
  }
  out[i] = v;
}

// the source holding global channel c: its base pointer, first channel and channel count (selects, not an indexed
// kernel-argument array: a dynamic index would copy the struct to scratch)
struct SrcRef {
  const float* p;
  int c0, cs;
};
__device__ __forceinline__ SrcRef src_of(const MpConvArgs& a, int c) {
  SrcRef r{a.src[0], 0, a.cbeg[1]};
  if (a.nsrc > 1 && c >= a.cbeg[1]) r = SrcRef{a.src[1], a.cbeg[1], a.cbeg[2] - a.cbeg[1]};
  if (a.nsrc > 2 && c >= a.cbeg[2]) r = SrcRef{a.src[2], a.cbeg[2], a.cbeg[3] - a.cbeg[2]};
  if (a.nsrc > 3 && c >= a.cbeg[3]) r = SrcRef{a.src[3], a.cbeg[3], a.cbeg[4] - a.cbeg[3]};
  return r;
}

// channel c of batch item b at (y, x), or 0 past Cin
__device__ __forceinline__ float src_at(const MpConvArgs& a, int b, int c, int y, int x) {
  if (c >= a.Cin) return 0.0f;
  const SrcRef r = src_of(a, c);
  return r.p[(((size_t)b * r.cs + (c - r.c0)) * a.H + y) * a.W + x];
}

// the body of the convolution kernel: a __global__ function of 256 threads, __launch_bounds__(256, 2), calls it with
// its argument (the instantiation files name their kernels)
template <class T, int KS, int NT>
__device__ __forceinline__ void conv2d_mp_body(const MpConvArgs& a) {
  using G = Geo<KS>;
  typedef typename T::elem elem;
  typedef typename T::v8 h8;
  __shared__ __attribute__((aligned(16))) elem in_s[G::IN_H];
  __shared__ __attribute__((aligned(16))) elem w_s[KS * KS * NT * 64 * 8];
  const elem* wpk = static_cast<const elem*>(a.wpk);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned t = blockIdx.x;
  const int nb = t % a.nnb; t /= a.nnb;
  const int tx = t % a.ntx; t /= a.ntx;
  const int ty = t % a.nty; t /= a.nty;
  const int b = t % a.B;
  const int slice = t / a.B;
  const int x0 = tx * TW, y0 = ty * TH;
  const int c_lo = slice * a.nchunks / a.ks, c_hi = (slice + 1) * a.nchunks / a.ks;

  float pre[G::IPT][8];
  auto fetch = [&](int ck) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < G::IPT; ++j) {
      const int i = tid + 256 * j;
      const int g = i / (G::LH * G::LW), rem = i - g * (G::LH * G::LW);
      const int ly = rem / G::LW, lx = rem - ly * G::LW;
      const int y = y0 - G::P + ly, x = x0 - G::P + lx;
      const int c = ck * KC + g * 8;
      const bool in_img = i < G::ITEMS && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
      const SrcRef r = src_of(a, c);
      if (in_img && c + 8 <= r.c0 + r.cs) {          // the 8 channels lie in one source: one base, plane strides
        const size_t hw = (size_t)a.H * a.W;
        const float* p = r.p + ((size_t)b * r.cs + (c - r.c0)) * hw + (size_t)y * a.W + x;
#pragma unroll
        for (int e = 0; e < 8; ++e) pre[j][e] = p[e * hw];
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) pre[j][e] = in_img ? src_at(a, b, c + e, y, x) : 0.0f;
      }
    }
  };
  auto commit = [&](int ck) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < G::IPT; ++j) {
      const int i = tid + 256 * j;
      if (i < G::ITEMS) {
        const int g = i / (G::LH * G::LW), rem = i - g * (G::LH * G::LW);
        h8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = T::round(pre[j][e]);            // round to nearest even
        *reinterpret_cast<h8*>(in_s + rem * CS + g * 8) = v;
      }
    }
    // weights of this chunk and n block: KS*KS taps x NT n tiles x 1 KiB, contiguous per tap
    constexpr int UNITS = KS * KS * NT * 64;
    for (int u = tid; u < UNITS; u += 256) {
      const int tap = u / (NT * 64), r = u - tap * (NT * 64);
      const size_t gsrc = (((size_t)ck * KS * KS + tap) * a.n16 + (size_t)nb * NT) * 512 + (size_t)r * 8;
      *reinterpret_cast<h8*>(w_s + u * 8) = *reinterpret_cast<const h8*>(wpk + gsrc);
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (c_lo < c_hi) fetch(c_lo);
  for (int ck = c_lo; ck < c_hi; ++ck) {
    __syncthreads();                       // the previous chunk's fragments are read
    commit(ck);
    __syncthreads();
    if (ck + 1 < c_hi) fetch(ck + 1);      // in flight during this chunk's MFMAs
#pragma unroll
    for (int tap = 0; tap < KS * KS; ++tap) {
      const int ky = tap / KS, kx = tap % KS;
      h8 af[MT], bf[NT];
#pragma unroll
      for (int m = 0; m < MT; ++m)
        af[m] = *reinterpret_cast<const h8*>(in_s + ((wave + ky) * G::LW + 16 * m + (lane & 15) + kx) * CS + 8 * (lane >> 4));
#pragma unroll
      for (int n = 0; n < NT; ++n) bf[n] = *reinterpret_cast<const h8*>(w_s + ((tap * NT + n) * 64 + lane) * 8);
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = T::mfma(af[m], bf[n], acc[m][n]);
    }
  }

  // ---- epilogue: lane holds output channel (lane & 15) of each N tile, x = 16m + 4(lane >> 4) + r ----
  const int y = y0 + wave;
  if (y >= a.H) return;
  const size_t hw = (size_t)a.H * a.W;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int co = (nb * NT + n) * 16 + (lane & 15);
    if (co >= a.Ctot) continue;
    const int head = co >= a.C1 ? 1 : 0;
    const int ch = head ? co - a.C1 : co, C = head ? a.Ctot - a.C1 : a.C1;
    const float bias = a.bias ? mp_r<T>(a.bias[co]) : 0.0f;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int x = x0 + 16 * m + 4 * (lane >> 4) + r;
        if (x >= a.W) continue;
        if (a.ks > 1) {
          a.scratch[(((size_t)slice * a.B + b) * a.Ctot + co) * hw + (size_t)y * a.W + x] = acc[m][n][r];
        } else {
          epilogue_store<T>(a, head, ((size_t)b * C + ch) * hw + (size_t)y * a.W + x, bias, acc[m][n][r]);
        }
      }
    }
  }
}

// fixed-order sum of the K-split partials + the epilogue: the body of a __global__ function of 256 threads
template <class T>
__device__ __forceinline__ void conv2d_mp_ksplit_epilogue_body(const MpConvArgs& a) {
  const size_t hw = (size_t)a.H * a.W, total = (size_t)a.B * a.Ctot * hw;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float v = a.scratch[i];
  for (int s = 1; s < a.ks; ++s) v += a.scratch[(size_t)s * total + i];
  const size_t p = i % hw;
  const int co = (int)((i / hw) % (size_t)a.Ctot);
  const int b = (int)(i / (hw * a.Ctot));
  const int head = co >= a.C1 ? 1 : 0;
  const int ch = head ? co - a.C1 : co, C = head ? a.Ctot - a.C1 : a.C1;
  epilogue_store<T>(a, head, ((size_t)b * C + ch) * hw + p, a.bias ? mp_r<T>(a.bias[co]) : 0.0f, v);
}

// element i of the packed weight image: the body of the packing kernel
template <class T>
__device__ __forceinline__ void conv2d_mp_pack_body(const float* __restrict__ w, typename T::elem* __restrict__ wpk,
                                                    int Cin, int Cout, int kk, int n16, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
  size_t t = i >> 9;
  const int nt = (int)(t % n16); t /= n16;
  const int tap = (int)(t % kk);
  const int ck = (int)(t / kk);
  const int co = nt * 16 + (lane & 15), ci = ck * KC + 8 * (lane >> 4) + j;
  wpk[i] = T::round((co < Cout && ci < Cin) ? w[((size_t)co * Cin + ci) * kk + tap] : 0.0f);
}

inline int nt_of(int Ctot) { return Ctot > 32 ? 4 : 1; }
inline int n16_of(int Ctot) { return (Ctot + 63) / 64 * 4; }     // padded so that NT = 4 blocks stay inside

// 16-bit elements of the packed image; 0 for a shape the packer refuses
inline size_t conv2d_mp_packed_elems(int Cin, int Cout, int k) {
  if (Cin <= 0 || Cout <= 0 || (k != 1 && k != 3)) return 0;
  return (size_t)((Cin + KC - 1) / KC) * k * k * n16_of(Cout) * 512;
}

inline int auto_kslices(int Cin, int H, int W, int Ctot, int k) {
  const int nt = nt_of(Ctot);
  const long long blocks = (long long)((H + TH - 1) / TH) * ((W + TW - 1) / TW) * ((Ctot + 16 * nt - 1) / (16 * nt));
  const int nchunks = (Cin + KC - 1) / KC;
  if (k != 3 || blocks >= 128) return 1;
  int ks = (int)((128 + blocks - 1) / blocks);
  if (ks > 8) ks = 8;
  while (ks > 1 && nchunks / ks < 2) --ks;
  return ks;
}

// The checks and the launches.  K names the instantiation's kernels: K::conv<KS, NT>(grid, stream, args),
// K::ksplit_epilogue(grid, stream, args) and K::pack(grid, stream, w, wpacked, Cin, Cout, kk, n16, total).
template <class K>
int conv2d_mp_run(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked, const float* bias,
                  const float* res1, const float* mul1, const float* blend_z, const float* blend_h, float* out1,
                  const float* res2, const float* mul2, float* out2, float* scratch, int ks, int B, int H, int W, int C1,
                  int C2, int k, int act, hipStream_t stream) {
  DV_REQUIRE_PTR(inputs);
  DV_REQUIRE_PTR(channels);
  DV_REQUIRE_PTR(wpacked);
  DV_REQUIRE_PTR(out1);
  DV_REQUIRE(n_inputs >= 1 && n_inputs <= 4, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(B > 0 && H > 0 && W > 0 && C1 > 0 && C2 >= 0, DV_ERR_SHAPE);
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  DV_REQUIRE(act == DV_ACT_NONE || act == DV_ACT_RELU || act == DV_ACT_SIGMOID || act == DV_ACT_TANH,
             DV_ERR_UNSUPPORTED);
  DV_REQUIRE((blend_z == nullptr) == (blend_h == nullptr), DV_ERR_NULL);
  DV_REQUIRE(C2 == 0 || out2 != nullptr, DV_ERR_NULL);
  DV_REQUIRE(ks >= 1 && ks <= 8 && (ks == 1 || scratch != nullptr), DV_ERR_UNSUPPORTED);
  MpConvArgs a = {};
  int cin = 0;
  a.cbeg[0] = 0;
  for (int i = 0; i < n_inputs; ++i) {
    DV_REQUIRE_PTR(inputs[i]);
    DV_REQUIRE(channels[i] > 0, DV_ERR_SHAPE);
    a.src[i] = inputs[i];
    cin += channels[i];
    a.cbeg[i + 1] = cin;
  }
  for (int i = n_inputs; i < 4; ++i) a.cbeg[i + 1] = cin;
  a.nsrc = n_inputs;
  a.wpk = wpacked;
  a.bias = bias;
  a.res[0] = res1; a.mul[0] = mul1; a.out[0] = out1;
  a.res[1] = res2; a.mul[1] = mul2; a.out[1] = out2;
  a.blend_z = blend_z; a.blend_h = blend_h;
  a.scratch = scratch; a.ks = ks;
  a.B = B; a.H = H; a.W = W; a.Cin = cin; a.C1 = C1; a.Ctot = C1 + C2;
  const int nt = nt_of(a.Ctot);
  a.n16 = n16_of(a.Ctot);
  a.nchunks = (cin + KC - 1) / KC;
  DV_REQUIRE(ks <= a.nchunks, DV_ERR_UNSUPPORTED);
  a.ntx = (W + TW - 1) / TW;
  a.nty = (H + TH - 1) / TH;
  a.nnb = (a.Ctot + 16 * nt - 1) / (16 * nt);
  a.act = act;
  const long long blocks = (long long)a.nnb * a.ntx * a.nty * B * ks;
  DV_REQUIRE(blocks <= 0x7fffffffLL, DV_ERR_SHAPE);
  const dim3 grid((unsigned)blocks);
  if (k == 3) {
    if (nt == 4) K::template conv<3, 4>(grid, stream, a);
    else K::template conv<3, 1>(grid, stream, a);
  } else {
    if (nt == 4) K::template conv<1, 4>(grid, stream, a);
    else K::template conv<1, 1>(grid, stream, a);
  }
  int rc = dv_launch_status();
  if (rc != DV_OK || ks == 1) return rc;
  const size_t total = (size_t)B * a.Ctot * H * W;
  K::ksplit_epilogue(dim3((unsigned)((total + 255) / 256)), stream, a);
  return dv_launch_status();
}

template <class K>
int conv2d_mp_pack(const float* w, void* wpacked, int Cin, int Cout, int k, dv_stream_t stream) {
  DV_REQUIRE_PTR(w);
  DV_REQUIRE_PTR(wpacked);
  DV_REQUIRE(Cin > 0 && Cout > 0, DV_ERR_SHAPE);
  DV_REQUIRE(k == 1 || k == 3, DV_ERR_UNSUPPORTED);
  const size_t total = conv2d_mp_packed_elems(Cin, Cout, k);
  K::pack(dim3((unsigned)((total + 255) / 256)), (hipStream_t)stream, w, wpacked, Cin, Cout, k * k, n16_of(Cout), total);
  return dv_launch_status();
}

// the four launching forms of a table
template <class K>
int conv2d_mp_cat(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked, const float* bias,
                  const float* residual, const float* mul, const float* blend_z, const float* blend_h, float* out,
                  float* scratch, int kslices, int B, int H, int W, int Cout, int k, int act, dv_stream_t stream) {
  return conv2d_mp_run<K>(inputs, channels, n_inputs, wpacked, bias, residual, mul, blend_z, blend_h, out, nullptr,
                          nullptr, nullptr, scratch, kslices, B, H, W, Cout, 0, k, act, (hipStream_t)stream);
}

template <class K>
int conv2d_mp_cat_pair(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                       const float* bias, const float* residual1, const float* mul1, float* out1, const float* residual2,
                       const float* mul2, float* out2, float* scratch, int kslices, int B, int H, int W, int Cout1,
                       int Cout2, int act, dv_stream_t stream) {
  DV_REQUIRE(Cout2 > 0, DV_ERR_SHAPE);
  return conv2d_mp_run<K>(inputs, channels, n_inputs, wpacked, bias, residual1, mul1, nullptr, nullptr, out1, residual2,
                          mul2, out2, scratch, kslices, B, H, W, Cout1, Cout2, 3, act, (hipStream_t)stream);
}

}  // namespace
