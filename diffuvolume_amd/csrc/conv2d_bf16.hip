// K13 at bf16: the 2-D convolutions of IGEV's update block at train precision "bf16" (KITTI15/core/update.py:26-142,
// the training loop of train_stereo.py:146-173 under `torch.autocast("cuda", dtype=torch.bfloat16)`) on
// v_mfma_f32_16x16x32_bf16: operands, the convolution result and every epilogue result rounded by rb16 (round to nearest
// even bfloat16 by v_cvt_pk_bf16_f32; NaN stays NaN, a finite float32 above about 3.3895e38 rounds to Inf, operands below
// 2^-126 may be flushed to zero).  Everything else is csrc/conv2d_mp.h's, written once for fp16 and bf16; this file is the
// bf16 instantiation and its entries.  The packed image has dv_conv2d_f16_packed_bytes bytes and the K-split choice is
// dv_conv2d_f16_auto_kslices: neither depends on the element type.
#include "conv2d_mp.h"

namespace {

template <int KS, int NT>
__global__ __launch_bounds__(256, 2) void conv2d_bf16_kernel(MpConvArgs a) {
  conv2d_mp_body<MpBf16, KS, NT>(a);
}

__global__ __launch_bounds__(256) void conv2d_bf16_ksplit_epilogue_kernel(MpConvArgs a) {
  conv2d_mp_ksplit_epilogue_body<MpBf16>(a);
}

__global__ void pack_bf16_kernel(const float* __restrict__ w, MpBf16::elem* __restrict__ wpk, int Cin, int Cout, int kk,
                                 int n16, size_t total) {
  conv2d_mp_pack_body<MpBf16>(w, wpk, Cin, Cout, kk, n16, total);
}

struct Kernels {
  template <int KS, int NT>
  static void conv(dim3 grid, hipStream_t s, const MpConvArgs& a) {
    hipLaunchKernelGGL((conv2d_bf16_kernel<KS, NT>), grid, dim3(256), 0, s, a);
  }
  static void ksplit_epilogue(dim3 grid, hipStream_t s, const MpConvArgs& a) {
    hipLaunchKernelGGL(conv2d_bf16_ksplit_epilogue_kernel, grid, dim3(256), 0, s, a);
  }
  static void pack(dim3 grid, hipStream_t s, const float* w, void* wpacked, int Cin, int Cout, int kk, int n16,
                   size_t total) {
    hipLaunchKernelGGL(pack_bf16_kernel, grid, dim3(256), 0, s, w, static_cast<MpBf16::elem*>(wpacked), Cin, Cout, kk, n16,
                       total);
  }
};

}  // namespace

#include "../../include/diffuvolume_hip_amp2d_bf16.h"

extern "C" int dv_conv2d_bf16_pack_weights(const float* w, void* wpacked, int Cin, int Cout, int k, dv_stream_t stream) {
  return conv2d_mp_pack<Kernels>(w, wpacked, Cin, Cout, k, stream);
}

extern "C" int dv_conv2d_bf16_cat(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                                 const float* bias, const float* residual, const float* mul, const float* blend_z,
                                 const float* blend_h, float* out, int B, int H, int W, int Cout, int k, int act,
                                 dv_stream_t stream) {
  return conv2d_mp_cat<Kernels>(inputs, channels, n_inputs, wpacked, bias, residual, mul, blend_z, blend_h, out, nullptr,
                                1, B, H, W, Cout, k, act, stream);
}

extern "C" int dv_conv2d_bf16_cat_ksplit(const float* const* inputs, const int* channels, int n_inputs,
                                        const void* wpacked, const float* bias, const float* residual, const float* mul,
                                        const float* blend_z, const float* blend_h, float* out, float* scratch,
                                        int kslices, int B, int H, int W, int Cout, int k, int act, dv_stream_t stream) {
  return conv2d_mp_cat<Kernels>(inputs, channels, n_inputs, wpacked, bias, residual, mul, blend_z, blend_h, out, scratch,
                                kslices, B, H, W, Cout, k, act, stream);
}

extern "C" int dv_conv2d_bf16_cat_pair(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                                      const float* bias, const float* residual1, const float* mul1, float* out1,
                                      const float* residual2, const float* mul2, float* out2, int B, int H, int W,
                                      int Cout1, int Cout2, int act, dv_stream_t stream) {
  return conv2d_mp_cat_pair<Kernels>(inputs, channels, n_inputs, wpacked, bias, residual1, mul1, out1, residual2, mul2,
                                     out2, nullptr, 1, B, H, W, Cout1, Cout2, act, stream);
}

extern "C" int dv_conv2d_bf16_cat_pair_ksplit(const float* const* inputs, const int* channels, int n_inputs,
                                             const void* wpacked, const float* bias, const float* residual1,
                                             const float* mul1, float* out1, const float* residual2, const float* mul2,
                                             float* out2, float* scratch, int kslices, int B, int H, int W, int Cout1,
                                             int Cout2, int act, dv_stream_t stream) {
  return conv2d_mp_cat_pair<Kernels>(inputs, channels, n_inputs, wpacked, bias, residual1, mul1, out1, residual2, mul2,
                                     out2, scratch, kslices, B, H, W, Cout1, Cout2, act, stream);
}
