/* diffuvolume_hip.h -- C ABI of libdiffuvolume_hip.so (MI355X / gfx950 only).
 *
 * The reference (iSEE-Laboratory/DiffuVolume) has no FFI layer: its hot path is
 * Python calling ATen.  This header is the boundary a maintainer binds instead
 * (ctypes stub in INTEGRATION.md).  Each entry point names the reference code it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to a dense, contiguous row-major tensor in
 *    the reference's own layout (NCHW / NCDHW); outputs are caller-allocated;
 *  - nothing here allocates, frees, synchronises or keeps global mutable state;
 *    calls are re-entrant and are enqueued on `stream` of the current device.  The one exception to "no global
 *    state" are the test hooks dv_conv3d_set_s2_tile, dv_conv3d_set_c1z, dv_deconv3d_set_impl and
 *    dv_deconv3d_pl_set_max_blocks: process-wide atomics meant for tests, not to be toggled while another thread launches;
 *  - stream contract: every launch and memset of an entry goes to `stream`, and no entry blocks the host;
 *  - alignment: a tensor operand needs only the alignment of its element type (4 bytes for float, 8 for double) unless
 *    the entry says otherwise below.  16-byte aligned operands on rows of whole quads (W or H*W a multiple of 4) select
 *    the vector loads / stores; any other placement takes the element-wise bodies and gives the same values to within
 *    the entry's rounding.  Packed weights (`wpacked`, whatever packer made them) must be 16-byte aligned: the entries
 *    that check it return DV_ERR_ALIGN.  A refused call launches nothing and writes nothing;
 *  - return value: 0 = ok, <0 = DV_ERR_* (bad argument), >0 = hipError_t.
 */
#ifndef DIFFUVOLUME_HIP_H
#define DIFFUVOLUME_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* dv_stream_t; /* hipStream_t */

#define DV_OK 0
#define DV_ERR_NULL (-1)        /* required pointer is NULL */
#define DV_ERR_SHAPE (-2)       /* dimension <= 0 or inconsistent */
#define DV_ERR_UNSUPPORTED (-3) /* shape/option outside what the kernels implement */
#define DV_ERR_ALIGN (-4)       /* pointer not 16-byte aligned */

#define DV_ACT_NONE 0
#define DV_ACT_RELU 1      /* SceneFlow / ACVNet */
#define DV_ACT_MISH 2      /* KITTI12 / PCWNet: x*tanh(softplus(x)) */
#define DV_ACT_LEAKY 3     /* KITTI15 / IGEV: LeakyReLU(0.01) */
#define DV_ACT_SIGMOID 4   /* ConvGRU gates (KITTI15/core/update.py:36-37); dv_conv2d_* only */
#define DV_ACT_TANH 5      /* ConvGRU candidate state (update.py:38); dv_conv2d_* only */

int dv_version(void);
const char* dv_error_string(int code);

/* ---- cost-volume builders ------------------------------------------------
 * build_gwc_volume: SceneFlow/models/submodule.py:228-238 (+ groupwise_correlation
 * :209-215); identical in KITTI12 :109-119 and KITTI15 :159-169.
 * ref,tgt [B,C,H,W] -> out [B,G,D,H,W];  out[b,g,d,y,x] = mean_c ref*tgt(x-d), 0 for x<d. */
int dv_gwc_volume_f32(const float* ref, const float* tgt, float* out,
                      int B, int C, int H, int W, int D, int G, dv_stream_t stream);

/* build_concat_volume: SceneFlow/models/submodule.py:180-191 (zero_left=0, = KITTI15
 * :206-217) and KITTI12/models/submodule.py:86-97 (zero_left=1).
 * ref,tgt [B,C,H,W] -> out [B,2C,D,H,W]. */
int dv_concat_volume_f32(const float* ref, const float* tgt, float* out,
                         int B, int C, int H, int W, int D, int zero_left, dv_stream_t stream);

/* F.softmax(att_weights, dim=2) * build_concat_volume(...): SceneFlow/models/acv_ddim.py:388-390
 * fused.  att [B,1,D,H,W] logits -> out [B,2C,D,H,W]. */
int dv_concat_attn_volume_f32(const float* ref, const float* tgt, const float* att, float* out,
                              int B, int C, int H, int W, int D, dv_stream_t stream);
/* The same product from the softmax already taken (p [B,D,H,W] of dv_softmax_d_f32; identical bits): what
 * AttentionConcatVolume.tensor() runs when something other than the rank-1 layer wants the tensor of acv_ddim.py:390. */
int dv_concat_prob_volume_f32(const float* ref, const float* tgt, const float* p, float* out,
                              int B, int C, int H, int W, int D, dv_stream_t stream);

/* ---- the first aggregation layer of a DiffuVolume step on its factored input --------------------------------
 * SceneFlow/models/acv_ddim.py:254-262 feeds `volume * noise` to dres0[0] (convbn_3d(64,32,3,1,1) + ReLU, :200-203)
 * with volume = softmax(att, dim=2) * build_concat_volume(L, R) (:388-390) and noise a per-voxel scalar: the input is
 * s(b,d,y,x) * [L(y,x) ; R(y,x-d)], so the 3x3x3 convolution is sum_tap s(.) * (GL[tap] + GR[tap](x-d)) with GL / GR
 * the 1x1 convolutions of L / R with the layer's weights, built once per stereo pair (csrc/rank1_filter.hip).
 * dv_softmax_d_f32: att [B,D,HW] logits -> p [B,D,HW] = softmax over D (the arithmetic of dv_concat_attn_volume_f32).
 * dv_mul_f32: out = x * y elementwise (s = p * n01).
 * dv_conv3d_rank1_filter_f32: s [B,D,H,W], gl / gr [B,27*Cout,H,W] (channel = tap*Cout + co, tap = (kd*3+ky)*3+kx)
 *   -> out [B,Cout,D,H,W] = act(scale * conv + bias); D <= 48. */
/* The tables themselves: a 1x1 convolution from few input channels (Cin <= 32: the concat features) to many output
 * channels (27 * Cout of the layer), no BatchNorm / activation: in [B,Cin,HW] -> out [B,Cout,HW] = W [Cout,Cin] . in.
 * A pure HBM write stream (csrc/pointwise_expand.hip).  Weights are packed once (dv_pointwise_expand_packed_floats floats). */
size_t dv_pointwise_expand_packed_floats(int Cin, int Cout);
int dv_pointwise_expand_pack_weights_f32(const float* w, float* wpacked, int Cin, int Cout, dv_stream_t stream);
int dv_pointwise_expand_f32(const float* in, const float* wpacked, float* out, int B, int Cin, int HW, int Cout,
                            dv_stream_t stream);
int dv_softmax_d_f32(const float* att, float* p, int B, int D, int HW, dv_stream_t stream);
int dv_mul_f32(const float* x, const float* y, float* out, size_t n, dv_stream_t stream);
int dv_conv3d_rank1_filter_f32(const float* s, const float* gl, const float* gr, const float* ch_scale,
                               const float* ch_bias, float* out, int B, int D, int H, int W, int Cout, int act,
                               dv_stream_t stream);

/* ---- time-shifted noise -> [0,1] volume filter ----------------------------
 * DynamicHead add (SceneFlow/models/head.py:74-77) + clamp + rescale
 * (acv_ddim.py:256-258).  x_t [B,C,HW], shift [B,C] (fp32, the MLP output),
 * n01 = (clamp(x_t+shift,-1,1)+1)/2 in the state dtype; n01_f32 = (float)n01
 * is what multiplies the volume (acv_ddim.py:260).  The f32 flavour is the
 * first DDIM step (state still fp32), f64 the later ones. */
int dv_noise_prepare_f32(const float* x_t, const float* shift, float* n01,
                         int B, int C, int HW, dv_stream_t stream);
int dv_noise_prepare_f64(const double* x_t, const float* shift, double* n01, float* n01_f32,
                         int B, int C, int HW, dv_stream_t stream);

/* ---- 3-D aggregation convolutions ------------------------------------------
 * convbn_3d (+ReLU/Mish/LeakyReLU): SceneFlow/models/submodule.py:94-97 and its
 * uses acv_ddim.py:60-70,:82-83,:200-222.  Cubic kernel k in {1,3}, pad (k-1)/2,
 * stride in {1,2}; implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32).
 *   y = act( conv(in * in_scale) * ch_scale[co] + ch_bias[co] + residual )
 * in [B,Cin,D,H,W]; in_scale [B,D,H,W] or NULL (the `volume * noise.unsqueeze(1)`
 * prologue of acv_ddim.py:260); ch_scale/ch_bias [Cout] or NULL (eval-mode BN
 * folded by the caller); residual [B,Cout,Do,Ho,Wo] or NULL; out same shape.
 * `wpacked` comes from dv_conv3d_pack_weights_f32. */
size_t dv_conv3d_packed_floats(int Cin, int Cout, int k);
int dv_conv3d_pack_weights_f32(const float* w /*[Cout,Cin,k,k,k]*/, float* wpacked,
                               int Cin, int Cout, int k, dv_stream_t stream);
int dv_conv3d_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                  const float* in_scale, const float* residual, float* out,
                  int B, int Cin, int D, int H, int W, int Cout, int k, int stride, int act,
                  dv_stream_t stream);

/* Test hook: pins the tiling of the DIRECT stride-2 kernel (0 = the launcher's own choice from the size of one batch item,
 * 1 = 2 x 4 x 32 output tiles, 2 = 2 x 2 x 32); both tilings give the same bits.  Process-wide; returns DV_OK. */
int dv_conv3d_set_s2_tile(int mode);
/* Test hook, process-wide: the z-marching form of the single-output-channel head (conv3d_c1z_kernel) takes volumes of at
 * least `min_tiles` 16 x 64 tiles per batch item (0 = the default, 64); `segment` pins the planes per block (0 = the
 * launcher's choice from the block count; 3, 6 or 12 -- every segment length gives the same bits). */
int dv_conv3d_set_c1z(int min_tiles, int segment);

/* The same 3x3x3 stride-1 layer (Cout <= 32) on the fp16 matrix instruction with every fp32 operand
 * carried as hi+lo fp16 pairs: x*w ~= hi*hi' + hi*lo' + lo*hi', fp32 accumulate (csrc/conv3d_f16x3.hip).
 * Split error 2^-22 per operand, below the fp32 accumulation rounding, for |in * in_scale| >= 0.5; below that an
 * absolute 2^-23 per activation (the lo half is an fp16 subnormal).  Opt-in (DV_CONV_PRECISION=f16x3).
 * Activations must stay below 2.6e5 in magnitude (fp16 range after the 2^-2 pre-scale): if one does not,
 * or is NaN, *overflow_flag (device int, may be NULL) is set to 1 and the output is not to be trusted. */
size_t dv_conv3d_f16x3_packed_bytes(int Cin, int Cout);
int dv_conv3d_f16x3_pack_weights(const float* w /*[Cout,Cin,3,3,3]*/, void* wpacked, int Cin, int Cout,
                                 dv_stream_t stream);
int dv_conv3d_f16x3_f32(const float* in, const void* wpacked, const float* ch_scale, const float* ch_bias,
                        const float* in_scale, const float* residual, float* out, int* overflow_flag,
                        int B, int Cin, int D, int H, int W, int Cout, int act, dv_stream_t stream);

/* The same 3x3x3 stride-1 layer with the two in-plane taps computed by the Winograd minimal-filtering transform
 * F(2x2,3x3) (depth taps direct): 2.25x fewer multiplies, still on v_mfma_f32_16x16x4_f32 with fp32 operands and
 * accumulation (csrc/conv3d_wino.hip).  The transforms only add / subtract (the 1/2 factors are folded into the
 * packed weights), so results differ from dv_conv3d_f32 by fp32 rounding of a few extra additions per product.
 * Same arguments and epilogue as dv_conv3d_f32 (k = 3, stride = 1); `wpacked` from dv_conv3d_wino_pack_weights_f32. */
size_t dv_conv3d_wino_packed_floats(int Cin, int Cout);
int dv_conv3d_wino_pack_weights_f32(const float* w /*[Cout,Cin,3,3,3]*/, float* wpacked, int Cin, int Cout,
                                    dv_stream_t stream);
int dv_conv3d_wino_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                       const float* in_scale, const float* residual, float* out,
                       int B, int Cin, int D, int H, int W, int Cout, int act, dv_stream_t stream);

/* The same layer with ALL THREE taps by minimal filtering, F(2x2x2,3x3x3) (csrc/conv3d_wino3.hip): 8 instead of 12
 * multiplies per output and input channel, the depth positions of the transform on the four waves of a block (they meet in
 * LDS after the channel loop).  fp32 operands and accumulation on v_mfma_f32_16x16x4_f32; the transforms only add /
 * subtract, measured error no larger than the in-plane form's (tools/probes/wino_f222_numerics.py).  No filter prologue
 * (a call with `in_scale` takes dv_conv3d_wino_f32).  dv_conv3d_wino3_supported: 1 when four channel volumes of the
 * input fit 31-bit byte offsets.  `in` must be 16-byte aligned (its rows are staged as quads): DV_ERR_ALIGN otherwise;
 * `out` / `residual` may have any float alignment. */
size_t dv_conv3d_wino3_packed_floats(int Cin, int Cout);
int dv_conv3d_wino3_supported(int Cin, int Cout, int D, int H, int W);
int dv_conv3d_wino3_pack_weights_f32(const float* w /*[Cout,Cin,3,3,3]*/, float* wpacked, int Cin, int Cout,
                                     dv_stream_t stream);
int dv_conv3d_wino3_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                        const float* residual, float* out, int B, int Cin, int D, int H, int W, int Cout, int act,
                        dv_stream_t stream);

/* The 3x3x3 STRIDE-2 layer (hourglass conv1 / conv3: acv_ddim.py:60,:66; pwcnet_ddim.py:137-147) in its polyphase
 * minimal-filtering form (csrc/conv3d_s2pp.hip): per in-plane axis the odd input phase sees a 2-tap filter, done as
 * F(2,2), the even phase one tap -- 25 instead of 36 multiplies per 2x2 outputs, depth taps direct, still on
 * v_mfma_f32_16x16x4_f32 with fp32 operands and accumulation.  The transforms only subtract (weights are summed once
 * by the pack), so results differ from dv_conv3d_f32(stride = 2) by fp32 rounding of one extra subtraction per operand.
 *   y = act( conv_s2(in) * ch_scale[co] + ch_bias[co] + residual )
 * 64 output channels per block and rows that travel as 16-byte quads: dv_conv3d_s2pp_supported says whether a layer
 * qualifies (Cout a multiple of 64, W a multiple of 4, D*H*W*4 <= 2^30), dv_conv3d_s2pp_f32 returns DV_ERR_UNSUPPORTED
 * otherwise.  `in` must be 16-byte aligned: DV_ERR_ALIGN otherwise; `out` / `residual` may have any float alignment.
 * Persistent launch: one persistent block per CU, two tiles at a time.
 * `wpacked` from dv_conv3d_s2pp_pack_weights_f32. */
int dv_conv3d_s2pp_supported(int Cin, int Cout, int D, int H, int W);
size_t dv_conv3d_s2pp_packed_floats(int Cin, int Cout);
int dv_conv3d_s2pp_pack_weights_f32(const float* w /*[Cout,Cin,3,3,3]*/, float* wpacked, int Cin, int Cout,
                                    dv_stream_t stream);
int dv_conv3d_s2pp_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                       const float* residual, float* out,
                       int B, int Cin, int D, int H, int W, int Cout, int act, dv_stream_t stream);

/* nn.ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1, bias=False) + BN
 * + skip add + activation: acv_ddim.py:74-80 and :91-92.  w [Cin,Cout,3,3,3].
 * in [B,Cin,D,H,W] -> out [B,Cout,2D,2H,2W]. */
size_t dv_deconv3d_packed_floats(int Cin, int Cout);
int dv_deconv3d_pack_weights_f32(const float* w /*[Cin,Cout,3,3,3]*/, float* wpacked,
                                 int Cin, int Cout, dv_stream_t stream);
int dv_deconv3d_k3s2_f32(const float* in, const float* wpacked, const float* ch_scale,
                         const float* ch_bias, const float* residual, float* out,
                         int B, int Cin, int D, int H, int W, int Cout, int act, dv_stream_t stream);

/* The k3 flavour has two launch shapes behind dv_deconv3d_k3s2_f32 / dv_deconv3d_k3s2_redir_f32 (same packed weights, same
 * arithmetic per output up to the order in which the fused skip channels join the sum): one-tile blocks
 * (csrc/deconv3d.hip) and one persistent block per CU with loader waves (csrc/deconv3d_pl.hip).
 * dv_deconv3d_pl_supported: 1 if the persistent kernel takes the shape (Cskip = 0: no fused skip convolution) -- whole
 * 8-channel input chunks, 32-channel output blocks, W % 4 == 0, Cskip % 4 == 0 and Cskip / 4 <= Cin / 8, 32-bit byte offsets
 * inside a batch item; the entry points also want 16-byte aligned tensors for it.  The choice never looks at the batch size.
 * dv_deconv3d_set_impl (test hook, process-wide): 0 = the launcher picks, 1 = one-tile blocks, 2 = persistent where supported. */
int dv_deconv3d_pl_supported(int Cin, int Cout, int D, int H, int W, int Cskip);
int dv_deconv3d_set_impl(int mode);
/* Test hook, process-wide: the persistent kernel launches at most n blocks (0 = one per CU), so that small volumes exercise
 * long per-block tile lists; results do not depend on it. */
int dv_deconv3d_pl_set_max_blocks(int n);

/* nn.ConvTranspose3d(kernel 4, stride 2, padding 1, bias=False) [+BN +LeakyReLU]: the IGEV hourglass's
 * conv3_up / conv2_up / conv1_up (KITTI15/core/igev_stereo_ddim.py:44-51, BasicConv deconv core/submodule.py:9-35).
 * w [Cin,Cout,4,4,4]; in [B,Cin,D,H,W] -> out [B,Cout,2D,2H,2W]; same fused epilogue as the k3 flavour. */
size_t dv_deconv3d_k4_packed_floats(int Cin, int Cout);
int dv_deconv3d_k4_pack_weights_f32(const float* w /*[Cin,Cout,4,4,4]*/, float* wpacked,
                                    int Cin, int Cout, dv_stream_t stream);
int dv_deconv3d_k4s2_f32(const float* in, const float* wpacked, const float* ch_scale,
                         const float* ch_bias, const float* residual, float* out,
                         int B, int Cin, int D, int H, int W, int Cout, int act, dv_stream_t stream);

/* ---- 2-D refinement stack (KITTI12 per-step disparity refinement) ------------------------------------
 * convbn (KITTI12/models/submodule.py:21-24: Conv2d(k, stride 1, padding = dilation, bias=False) + BatchNorm2d)
 * [+ Mish] and BasicBlock's `out += x` (:192-215), as used by refinenet_version3 (pwcnet_ddim.py:251-306):
 *   out = act( conv2d(in, w; dilation) * ch_scale + ch_bias + residual ),  k = 3 (dilation 1..16) or 1.
 * in [B,Cin,H,W], w [Cout,Cin,k,k], out / residual [B,Cout,H,W].  Weights are packed once per layer. */
size_t dv_conv2d_packed_floats(int Cin, int Cout, int k, int dilation);
int dv_conv2d_pack_weights_f32(const float* w, float* wpacked, int Cin, int Cout, int k, int dilation,
                               dv_stream_t stream);
int dv_conv2d_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                  const float* residual, float* out, int B, int Cin, int H, int W, int Cout, int k,
                  int dilation, int act, dv_stream_t stream);

/* The same convolution with the ConvGRU gate arithmetic of KITTI15/core/update.py:26-40 in its epilogue:
 *   v = act( conv2d(in, w) * ch_scale + ch_bias + residual );
 *   if (mul)      v = v * mul;                                   r * h            (update.py:38, the `r*h` operand)
 *   if (blend_z)  v = blend_h + blend_z * (v - blend_h);         (1-z)*h + z*q    (update.py:39)
 * mul / blend_z / blend_h are [B,Cout,H,W] or NULL; act may also be DV_ACT_SIGMOID / DV_ACT_TANH. */
int dv_conv2d_gated_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                        const float* residual, const float* mul, const float* blend_z, const float* blend_h,
                        float* out, int B, int Cin, int H, int W, int Cout, int k, int dilation, int act,
                        dv_stream_t stream);

/* The gated convolution over a VIRTUAL channel concatenation: `conv(torch.cat(inputs, dim=1))` without the copy
 * (ConvGRU.forward, KITTI15/core/update.py:33-38: hx = cat[h, x...], cat[r*h, x...]).  `inputs` / `channels` are HOST
 * arrays of n_inputs (1..4) device pointers [B,channels[i],H,W] and their channel counts; the weights are those
 * of the full convolution (Cin = sum of channels), packed as usual. */
int dv_conv2d_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                      const float* ch_scale, const float* ch_bias, const float* residual, const float* mul,
                      const float* blend_z, const float* blend_h, float* out, int B, int H, int W, int Cout,
                      int k, int dilation, int act, dv_stream_t stream);

/* K-split form of dv_conv2d_cat_f32 for launches too small to fill the chip (a single IGEV pair at 1/8 and 1/16
 * resolution: KITTI15/core/update.py:33-40 at 48x156 / 24x78 pixels): `kslices` blocks share an output tile, each
 * sums a contiguous range of the input-channel chunks into scratch[kslices][B,Cout,H,W]; a second small kernel adds
 * the slices in a fixed order (deterministic) and applies the same fused epilogue.  kslices must be the value
 * dv_conv2d_auto_kslices returns for this shape (1 = use dv_conv2d_cat_f32); scratch is caller-allocated.  The factor is a
 * function of ONE batch item (`B` is ignored since round 5): it fixes the summation order, and a shard of a batch must
 * reproduce the batch's bits. */
int dv_conv2d_auto_kslices(int B, int Cin, int H, int W, int Cout, int k, int dilation);
int dv_conv2d_cat_ksplit_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                             const float* ch_scale, const float* ch_bias, const float* residual, const float* mul,
                             const float* blend_z, const float* blend_h, float* out, float* scratch, int kslices,
                             int B, int H, int W, int Cout, int k, int dilation, int act, dv_stream_t stream);

/* Stride-2 flavour (the down-sampling layers of the 2-D feature CNNs: SceneFlow/models/acv_ddim.py:19-21, :28 --
 * convbn(k 3, stride 2, pad 1) and the 1x1 stride-2 `downsample`): out [B,Cout,(H-1)/2+1,(W-1)/2+1], dilation 1,
 * residual (if any) has the output's shape.  Same packed weights as dv_conv2d_f32 with dilation 1. */
int dv_conv2d_s2_f32(const float* in, const float* wpacked, const float* ch_scale, const float* ch_bias,
                     const float* residual, float* out, int B, int Cin, int H, int W, int Cout, int k, int act,
                     dv_stream_t stream);

/* The 3x3, dilation-1, stride-1 case of dv_conv2d_cat_f32 in the Winograd F(2x2,3x3) form (csrc/conv2d_wino.hip): 2.25x
 * fewer multiplies on the same fp32 MFMA instruction, same epilogue (scale/bias, residual, activation, `mul`, GRU
 * blend) and the same virtual channel concatenation of up to four inputs; results equal dv_conv2d_cat_f32 up to fp32
 * rounding.  `wpacked` from dv_conv2d_wino_pack_weights_f32 (its own layout). */
size_t dv_conv2d_wino_packed_floats(int Cin, int Cout);
int dv_conv2d_wino_pack_weights_f32(const float* w /*[Cout,Cin,3,3]*/, float* wpacked, int Cin, int Cout,
                                    dv_stream_t stream);
int dv_conv2d_wino_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                           const float* ch_scale, const float* ch_bias, const float* residual, const float* mul,
                           const float* blend_z, const float* blend_h, float* out, int B, int H, int W, int Cout,
                           int act, dv_stream_t stream);
/* Two 3x3 convolutions of the SAME input in one launch: ConvGRU's z and r gates (KITTI15/core/update.py:33-35,
 * `convz(hx)` and `convr(hx)`).  `wpacked` / `ch_scale` / `ch_bias` hold the Cout1 + Cout2 output channels back to back
 * (pack the concatenated weight; Cout1 % 32 == 0); channels < Cout1 go to out1 [B,Cout1,H,W] with residual1 / mul1,
 * the others to out2 [B,Cout2,H,W] with residual2 / mul2:  out_g = act(conv_g * scale + bias + residual_g) * mul_g.
 * out2 / residual2 / mul2 must be 16-byte aligned (DV_ERR_ALIGN otherwise); out1 / residual1 / mul1 need not be. */
int dv_conv2d_wino_cat_pair_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                                const float* ch_scale, const float* ch_bias, const float* residual1, const float* mul1,
                                float* out1, const float* residual2, const float* mul2, float* out2, int B, int H,
                                int W, int Cout1, int Cout2, int act, dv_stream_t stream);
/* The same with dilation 1..16 (the refinement network's dilated layers, KITTI12/models/submodule.py:251-306, and the
 * dilated blocks of the 2-D feature CNNs): a dilation-d 3x3 convolution is d*d independent dilation-1 convolutions on the
 * sub-sampled images, so each block runs the Winograd kernel on a 16x16 tile of one sub-image.  Same packed weights. */
int dv_conv2d_wino_dil_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                               const float* ch_scale, const float* ch_bias, const float* residual, const float* mul,
                               const float* blend_z, const float* blend_h, float* out, int B, int H, int W, int Cout,
                               int dilation, int act, dv_stream_t stream);

/* Input assembly of that refinement (KITTI12/models/pwcnet_ddim.py:486-502), fused:
 *   frw = warp(right, disp)  (models/submodule.py:137-176, incl. its align_corners mismatch and >= 0.999 mask),
 *   cv  = build_corrleation_volume(left, frw, maxshift, 1)  (:121-135, incl. its negative-shift slicing),
 *   out = cat(left - frw, left, Mish(du_a * disp + du_b), disp, cv)   [B, 3C + 1 + 2*maxshift + 1, H, W].
 * left/right [B,C,H,W] (C <= 32), disp [B,H,W]; du_a/du_b [C] = `dispupsample` (1x1 conv + BN) folded;
 * maxshift must be 24. */
int dv_refine_inputs_f32(const float* left, const float* right, const float* disp, const float* du_a,
                         const float* du_b, float* out, int B, int C, int H, int W, int maxshift,
                         dv_stream_t stream);

/* K-split forms of the two Winograd entries above, for launches that leave most of the chip empty (IGEV's ConvGRU at 1/16
 * resolution: 80 / 40 blocks per pair): `kslices` = dv_conv2d_wino_auto_kslices(Cin, H, W, Cout, dilation) blocks share an
 * output tile, each sums a contiguous range of the input-channel chunks into scratch [kslices][B,Cout,H,W] (Cout = Cout1 + Cout2
 * for the pair), and a second kernel adds the slices in slice order (deterministic) and applies the epilogue.  The factor
 * depends on ONE batch item only, so a shard of a batch reproduces the batch's bits.  kslices == 1: use the entries above. */
int dv_conv2d_wino_auto_kslices(int Cin, int H, int W, int Cout, int dilation);
int dv_conv2d_wino_cat_ksplit_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                                  const float* ch_scale, const float* ch_bias, const float* residual, const float* mul,
                                  const float* blend_z, const float* blend_h, float* out, float* scratch, int kslices, int B,
                                  int H, int W, int Cout, int dilation, int act, dv_stream_t stream);
int dv_conv2d_wino_cat_pair_ksplit_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                                       const float* ch_scale, const float* ch_bias, const float* residual1, const float* mul1,
                                       float* out1, const float* residual2, const float* mul2, float* out2, float* scratch,
                                       int kslices, int B, int H, int W, int Cout1, int Cout2, int act, dv_stream_t stream);

/* Space-to-batch for the dilated layers of refinenet_version3 (KITTI12/models/pwcnet_ddim.py:251-306), csrc/refine_inputs.hip.
 * dv_space_to_batch2_f32: [N,C,h,w] -> [4N,C,h/2,w/2]; sub-image (y & 1, x & 1) of item n becomes item 4n + 2(y & 1) + (x & 1)
 *   (h, w even; `in` 8-byte aligned, DV_ERR_ALIGN otherwise).  A 3x3 convolution with dilation 2d on the input is one with dilation d on the output.
 * dv_batch_to_space_f32: the inverse of `levels` such steps at once: in [B * 4^levels, C, H >> levels, W >> levels] -> out [B,C,H,W]. */
int dv_space_to_batch2_f32(const float* in, float* out, int N, int C, int h, int w, dv_stream_t stream);
/* dv_conv2d_wino_cat_f32 (dilation 1, no residual / mul / blend) with its output stored through dv_space_to_batch2_f32's
 * mapping: out [4B,Cout,H/2,W/2] (H, W even).  The layer in front of a dilation doubling writes what the next layer reads. */
int dv_conv2d_wino_s2b_f32(const float* const* inputs, const int* channels, int n_inputs, const float* wpacked,
                           const float* ch_scale, const float* ch_bias, float* out, int B, int H, int W, int Cout,
                           int act, dv_stream_t stream);
int dv_batch_to_space_f32(const float* in, float* out, int B, int C, int H, int W, int levels, dv_stream_t stream);

/* FeatureAtt.forward's broadcast product (KITTI15/core/submodule.py:234-239):
 * out[b,c,d,y,x] = sigmoid(logit[b,c,y,x]) * cv[b,c,d,y,x]; out may alias cv. */
int dv_feature_gate_f32(const float* cv /*[B,C,D,H,W]*/, const float* logit /*[B,C,H,W]*/, float* out,
                        int B, int C, int D, int H, int W, dv_stream_t stream);

/* Backward of dv_feature_gate_f32 (training of FeatureAtt, KITTI15/core/submodule.py:234-239; six gates per forward,
 * igev_stereo_ddim.py:62-88, :380): with s = sigmoid(logit) recomputed and g = d loss / d out [B,C,D,H,W]
 *   dcv[b,c,d,y,x] = g * s[b,c,y,x]        dlogit[b,c,y,x] = s (1 - s) * sum_d g[b,c,d,y,x] * cv[b,c,d,y,x]
 * g and cv are read once each; the d sum runs in ascending order inside one thread.  A plane too small to fill the chip
 * splits D into contiguous ranges over blocks: partials go to `workspace` (dv_feature_gate_bwd_workspace_floats
 * floats; 0 = no split, workspace may be NULL) and are added in split order.  No atomics: the same bits on every launch. */
size_t dv_feature_gate_bwd_workspace_floats(int B, int C, int D, int H, int W);
int dv_feature_gate_bwd_f32(const float* cv /*[B,C,D,H,W]*/, const float* logit /*[B,C,H,W]*/, const float* g,
                            float* dcv, float* dlogit, float* workspace, int B, int C, int D, int H, int W,
                            dv_stream_t stream);

/* The hourglass tail `F.relu(conv6(x) + redir1(skip))` (SceneFlow/models/acv_ddim.py:81-86, :91-92; KITTI12
 * pwcnet_ddim.py:236-248 with Mish) in ONE launch: the 1x1x1 `redir` convolution of the skip tensor is folded into
 * the transposed convolution as extra K-steps.
 *   out = act( deconv3d_k3s2(in, w) + redir_w . skip + ch_bias )
 * Both BatchNorm scales must already be folded into `w` (before dv_deconv3d_pack_weights_f32) and `redir_w`
 * ([Cout][Cskip] row-major, device), their shifts summed into ch_bias.  skip [B,Cskip,2D,2H,2W].
 * Needs W % 2 == 0, a 16-byte aligned `skip` (its quads must not straddle a row end) and ceil(Cskip/8) <= ceil(Cin/8);
 * otherwise DV_ERR_UNSUPPORTED (run the two layers apart). */
int dv_deconv3d_k3s2_redir_f32(const float* in, const float* wpacked, const float* ch_bias, const float* skip,
                               const float* redir_w, float* out, int B, int Cin, int D, int H, int W, int Cout,
                               int Cskip, int act, dv_stream_t stream);

/* The attention branch's depth-wise stencils on the gwc volume (SceneFlow/models/acv_ddim.py:181-188, :377-381):
 * out = cat_g( Conv3d_(1,3,3),dil_g( Conv3d_(1,3,3)(gwc) ) ), both per channel (groups = channels), zero padded.
 * gwc/out [B,G,D,H,W]; w1 = `patch` weights [G][9]; w2 = the matching `patch_l1/l2/l3` weights [G][9];
 * dilation [G] (int32, 1..3).  All pointers on the device. */
int dv_patch_volume_f32(const float* gwc, const float* w1, const float* w2, const int* dilation, float* out,
                        int B, int G, int D, int H, int W, dv_stream_t stream);
/* The same pass with the dilation given as host-side runs of consecutive groups (run r: groups run_g0[r] ..
 * run_g0[r] + run_ng[r] - 1 at dilation run_dil[r]; the runs tile 0..G-1 in order): the 16-byte fast path needs the
 * dilation at launch time.  `dilation_dev` (device, [G]) serves the element-wise kernel when W % 4 != 0. */
int dv_patch_volume_runs_f32(const float* gwc, const float* w1, const float* w2, const int* dilation_dev, float* out,
                             int B, int G, int D, int H, int W, int nruns, const int* run_g0, const int* run_ng,
                             const int* run_dil, dv_stream_t stream);

/* attention_block.forward: SceneFlow/models/submodule.py:398-429 -- 4x4x4 window
 * multi-head self-attention (heads x C/heads), qkv Linear(C,3C)+bias, softmax,
 * final 1x1x1 Conv3d(C,C)+bias.  x [B,C,D,H,W] -> out same shape.  D must be a
 * multiple of 4; H,W not multiples of 4 are zero-padded with the reference's
 * -1000 mask rule.  C == 128, heads == 16 in every reference use.  qkv_w / proj_w must be 16-byte aligned
 * (DV_ERR_ALIGN otherwise); x / out and the two bias vectors need not be. */
int dv_window_attn3d_f32(const float* x, const float* qkv_w /*[3C,C]*/, const float* qkv_b /*[3C]*/,
                         const float* proj_w /*[C,C]*/, const float* proj_b /*[C]*/, float* out,
                         int B, int C, int D, int H, int W, int heads, dv_stream_t stream);

/* ---- regression tail ---------------------------------------------------------
 * F.upsample(trilinear, x4) + F.softmax(dim=1) + disparity_regression
 * (acv_ddim.py:267-270, submodule.py:173-177) and the uncertainty
 * sum_k |disp-k| p_k (acv_ddim.py:325-329), fused: the [B,4D,4h,4w] volumes are
 * never materialised.  cost [B,D,h,w] -> disp [B,4h,4w], unc [B,4h,4w] (or NULL).
 * align_corners: 0 = SceneFlow, 1 = KITTI12 (pwcnet_ddim.py:480). */
int dv_upsample_softmax_regress_f32(const float* cost, float* disp, float* unc,
                                    int B, int D, int h, int w, int align_corners, dv_stream_t stream);

/* Uncertainty about an externally supplied disparity (KITTI12: the 2-D-refined `disp_finetune`,
 * pwcnet_ddim.py:548-552): unc = sum_k |disp - k| * softmax(trilinear(cost))_k.
 * cost [B,D,h,w], disp [B,4h,4w] (input) -> unc [B,4h,4w]. */
int dv_upsample_softmax_uncertainty_f32(const float* cost, const float* disp, float* unc,
                                        int B, int D, int h, int w, int align_corners, dv_stream_t stream);

/* disparity_regression on a materialised probability volume (submodule.py:173-177):
 * prob [B,D,H,W] -> disp [B,H,W]. */
int dv_disparity_regression_f32(const float* prob, float* disp, int B, int D, int H, int W,
                                dv_stream_t stream);

/* F.softmax(dim=1) + disparity_regression at the volume's own resolution (IGEV init_disp,
 * KITTI15/core/igev_stereo_ddim.py:382-383): cost [B,D,H,W] -> disp [B,H,W]. */
int dv_softmax_regress_f32(const float* cost, float* disp, int B, int D, int H, int W, dv_stream_t stream);

/* two-hot encoding of a quarter-resolution disparity (acv_ddim.py:403-419):
 * disp_q [B,h*w] -> x [B,nbins,h*w] = 2*twohot-1.
 * disp_q is expected in [0, nbins).  Outside it the reference raises (scatter index out of range); this entry does
 * not look and writes what its arithmetic gives: every element finite and in [-1,1], all -1 for disp_q >= nbins
 * (tests/test_gpu_ddim_kernels.py pins that). */
int dv_encode_two_hot_f32(const float* disp_q, float* x, int B, int nbins, int hw, dv_stream_t stream);

/* One DDIM state update, everything after the regression of one step
 * (acv_ddim.py:272-294 and :318-362):
 *   x_start  = 2*twohot(bilinear_down4(clamp(disp,0,4*nbins-1))/4) - 1          (fp32 out)
 *   pred_eps = (sqrt_recip*n01 - x_start) / sqrt_recipm1                          (fp64)
 *   keep     = bilinear_down4( |disp-used|<dif_thr & unc<unc_thr );  mask = clamp(mask+keep,0,1)
 *   x_next   = last ? x_start : (mask==0 ? fill : x_start*sqrt_alpha_next + c*pred_eps + sigma*eps)
 *   ens     += cof * disp
 * n01_f32 / n01_f64: exactly one is non-NULL (state dtype of this step).
 * eps_f32 / eps_f64: exactly one non-NULL unless last (randn_like(img) follows img's dtype).
 * disp,unc,used,ens [B,4h,4w]; mask [B,h,w] in/out; fill,x_next,pred_eps fp64 [B,nbins,h,w];
 * pred_eps and ens may be NULL (not wanted).
 * Rounding points (the reference's dtype promotions, acv_ddim.py:356): x_start * sqrt_alpha_next is a float32
 * tensor times a 0-dim float64 scalar and is rounded to float32, with sqrt_alpha_next itself rounded to float32
 * first; sigma * eps_f32 likewise is (float)sigma * eps rounded to float32 (with eps_f64 it is a float64 product);
 * c * pred_eps, pred_eps itself and the two additions are float64.  x_start and mask are bit-exact statements
 * (every multiplication on their way is by 0.5 or 2).  x_next and pred_eps are compared with the reference at the
 * level of float64 ulps and not bit for bit: the library is built with -ffp-contract=on, so a float64 a*b+c may be
 * one fused operation here and two roundings in torch (tests/ddim_statement.py, tests/test_gpu_ddim_kernels.py). */
typedef struct dv_ddim_coef {
  double sqrt_recip_alpha;   /* sqrt(1/abar_t)     acv_ddim.py:156 */
  double sqrt_recipm1_alpha; /* sqrt(1/abar_t - 1) acv_ddim.py:157 */
  double sqrt_alpha_next;    /* sqrt(abar_next)    acv_ddim.py:356 */
  double c;                  /* sqrt(1-abar_next-sigma^2) acv_ddim.py:352 */
  double sigma;              /* acv_ddim.py:351 */
  float dif_thr;             /* 1  (acv_ddim.py:323) */
  float unc_thr;             /* 3  (acv_ddim.py:330) */
  float cof;                 /* ensemble weight of this step's disparity (acv_ddim.py:367) */
  int last;                  /* time_next < 0 (acv_ddim.py:344-346) */
  float clamp_max;           /* clamp of disp before the /4 downsample: 4*nbins-1 (ACV/PCW), nbins-1 (IGEV :265) */
  float ens_dif_thr;         /* >0: ensemble takes |disp-used|<thr ? disp : used (IGEV :323-327); 0: disp */
} dv_ddim_coef;

/* unc may be NULL (IGEV renewal mask tests the disparity only); coords0 [B,h,w] is NULL except for IGEV,
 * where the two-hot position is clamp(coords0 + disp_q, 0, nbins-1) (igev_stereo_ddim.py:268-272). */
int dv_ddim_step(const float* disp, const float* unc, const float* used, const float* coords0,
                 const float* n01_f32, const double* n01_f64,
                 const float* eps_f32, const double* eps_f64, const double* fill,
                 float* mask, float* x_start, double* pred_eps, double* x_next, float* ens,
                 int B, int nbins, int h, int w, const dv_ddim_coef* coef, dv_stream_t stream);

/* ---- IGEV: convex upsampling of the quarter-resolution disparity ------------------------
 * IGEVStereo_ddim.upsample_disp (KITTI15/core/igev_stereo_ddim.py:209-217) = F.softmax(spx_pred, 1) followed by
 * context_upsample (core/submodule.py:241-253):
 *   out[b,Y,X] = sum_{k=3ky+kx} p_k[b,Y,X] * scale * disp_low[b, (Y>>2)+ky-1, (X>>2)+kx-1]   (zeros outside)
 * disp_low [B,h,w]; weights [B,9,4h,4w] (logits when apply_softmax != 0, else probabilities); out [B,4h,4w];
 * scale = 4 in the reference (`disp*4.`).  weights / out must be 16-byte aligned (DV_ERR_ALIGN otherwise). */
int dv_context_upsample_f32(const float* disp_low, const float* weights, float* out, int B, int h, int w,
                            float scale, int apply_softmax, dv_stream_t stream);

/* Backward of the above for training (the reference differentiates `upsample_disp` at every GRU iteration:
 * igev_stereo_ddim.py:203-211 called from the train loop :441-457, and context_upsample core/submodule.py:241-253 on
 * `init_disp` :462).  grad_out [B,4h,4w]; with nb_k = scale * disp_low[(Y>>2)+ky-1, (X>>2)+kx-1] and p the softmax
 * recomputed from the logits with the forward's expression (probabilities are never saved):
 *   d_weights[b,k,Y,X] = p_k (g nb_k - sum_j p_j g nb_j)      (apply_softmax == 0: g nb_k)
 *   d_disp[b,y,x]      = scale * sum_k s_k[b, y-ky+1, x-kx+1],  s_k[cell] = sum over the cell's 16 pixels of g p_k
 * d_weights [B,9,4h,4w] or d_disp [B,h,w] may be NULL (not both): that gradient is not computed.  cell_sums: scratch of
 * B*9*h*w floats (the s_k), required when d_disp is given.  A gather in both passes -- no scatter, no atomics, fixed
 * summation order: the same bits on every launch.  weights / grad_out / d_weights must be 16-byte aligned
 * (DV_ERR_ALIGN otherwise). */
int dv_context_upsample_bwd_f32(const float* disp_low, const float* weights, const float* grad_out, float* d_weights,
                                float* d_disp, float* cell_sums, int B, int h, int w, float scale, int apply_softmax,
                                dv_stream_t stream);

/* ---- IGEV: the small per-iteration operators around the ConvGRUs (KITTI15/core/update.py) ----
 * dv_conv2d_1in_f32: nn.Conv2d(1, Cout, k, padding=k/2) + bias + activation on a single-channel image (the motion
 *   encoder's 7x7 `convd1` on the disparity, update.py:86,:92).  in [B,1,H,W]; w [Cout,1,k,k] (k = 3, 5, 7); out [B,Cout,H,W].
 * dv_resize_bilinear_ac_f32: F.interpolate(x, (H,W), mode='bilinear', align_corners=True) (`interp`, update.py:100-102),
 *   PyTorch's source-index arithmetic.  in [BC,h,w] -> out [BC,H,W].
 * dv_avg_pool3s2_f32: F.avg_pool2d(x, 3, stride=2, padding=1) with the padded zeros counted (`pool2x`, update.py:96-97).
 *   in [BC,H,W] -> out [BC,(H-1)/2+1,(W-1)/2+1]. */
int dv_conv2d_1in_f32(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cout,
                      int k, int act, dv_stream_t stream);
/* dv_conv2d_1in_f16: dv_conv2d_1in_f32 under fp16 autocast (`convd1` with mixed_precision, update.py:86,:92 inside
 *   igev_stereo_ddim.py:242-246's autocast region): input, weights and bias rounded to fp16, fp32 accumulation, the
 *   convolution's output rounded to fp16 before the activation (sigmoid / tanh results rounded again).  fp32 storage. */
int dv_conv2d_1in_f16(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, int Cout,
                      int k, int act, dv_stream_t stream);
int dv_resize_bilinear_ac_f32(const float* in, float* out, int BC, int h, int w, int H, int W, dv_stream_t stream);
int dv_avg_pool3s2_f32(const float* in, float* out, int BC, int H, int W, dv_stream_t stream);

/* ---- IGEV's update block under fp16 autocast (csrc/conv2d_f16.hip): every 3x3 / 1x1 convolution of
 * BasicMultiUpdateBlock with `mixed_precision=True` (KITTI15/core/update.py:26-142, run inside
 * `autocast(enabled=self.args.mixed_precision)` at igev_stereo_ddim.py:242-246) as a direct implicit GEMM on
 * v_mfma_f32_16x16x32_f16.  Input, weight and bias are rounded to fp16, products accumulate in fp32, the output is
 * rounded to fp16, and every epilogue op rounds its result to fp16 again (what autocast's fp16 tensors do):
 *   v = r(conv + r(bias)); v = r(v + residual); v = r(act(v)); v = r(v * mul); blend: v = r(r(r(1-z)*h) + r(z*v)).
 * Storage is fp32 (fp16-exact values).  k in {1, 3}, dilation 1, stride 1, "same" padding; act NONE / RELU / SIGMOID /
 * TANH.  `inputs` / `channels` are HOST arrays of n_inputs (1..4) sources read as one virtual channel concatenation
 * (as dv_conv2d_cat_f32; any channel split).  residual / mul / blend_z / blend_h are [B,Cout,H,W] or NULL.
 * dv_conv2d_f16_packed_bytes / dv_conv2d_f16_pack_weights: w [Cout,Cin,k,k] fp32 -> the kernel's fp16 image
 *   (caller-allocated, packed_bytes bytes).
 * dv_conv2d_f16_cat_pair: two 3x3 convolutions of the same input (ConvGRU's convz | convr, update.py:33-35) in one
 *   launch: the weights of Cout1 + Cout2 channels packed back to back; channels < Cout1 go to out1 with residual1 /
 *   mul1, the others to out2 with residual2 / mul2.
 * dv_conv2d_f16_auto_kslices: the K-split factor for a launch of this shape (a function of ONE batch item: a shard of a
 *   batch reproduces the batch's bits); > 1 means use the _ksplit forms with scratch of kslices * B * (Cout1 + Cout2)
 *   * H * W floats.  The slices are summed in a fixed order (deterministic).
 * dv_conv2d_f16_packed_bytes and dv_conv2d_f16_auto_kslices serve BOTH 16-bit element types: the bf16 entries of
 *   diffuvolume_hip_amp2d_bf16.h (csrc/conv2d_bf16.hip, the same kernel body in csrc/conv2d_mp.h) pack an image of the
 *   same size and take the same launch choice -- neither depends on the element type, so they have no bf16 twins. */
size_t dv_conv2d_f16_packed_bytes(int Cin, int Cout, int k);
int dv_conv2d_f16_pack_weights(const float* w, void* wpacked, int Cin, int Cout, int k, dv_stream_t stream);
int dv_conv2d_f16_auto_kslices(int Cin, int H, int W, int Cout, int k);
int dv_conv2d_f16_cat(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                      const float* bias, const float* residual, const float* mul, const float* blend_z,
                      const float* blend_h, float* out, int B, int H, int W, int Cout, int k, int act,
                      dv_stream_t stream);
int dv_conv2d_f16_cat_ksplit(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                             const float* bias, const float* residual, const float* mul, const float* blend_z,
                             const float* blend_h, float* out, float* scratch, int kslices, int B, int H, int W,
                             int Cout, int k, int act, dv_stream_t stream);
int dv_conv2d_f16_cat_pair(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                           const float* bias, const float* residual1, const float* mul1, float* out1,
                           const float* residual2, const float* mul2, float* out2, int B, int H, int W, int Cout1,
                           int Cout2, int act, dv_stream_t stream);
int dv_conv2d_f16_cat_pair_ksplit(const float* const* inputs, const int* channels, int n_inputs, const void* wpacked,
                                  const float* bias, const float* residual1, const float* mul1, float* out1,
                                  const float* residual2, const float* mul2, float* out2, float* scratch, int kslices,
                                  int B, int H, int W, int Cout1, int Cout2, int act, dv_stream_t stream);

/* IGEV's once-per-pair 2-D front without MIOpen (csrc/igev_front.hip).
 * dv_conv2d_fewin_f32: nn.Conv2d(Cin <= 4, Cout, k in {3,5,7}, stride in {1,2}, padding=k/2) [+ bias] [+ folded eval
 *   BatchNorm: y * ch_scale + ch_shift, both or neither] + activation -- the 7x7 stride-2 stem of the context encoder
 *   (KITTI15/core/extractor.py:197) and the RGB stems; w [Cout,Cin,k,k]; out [B,Cout,(H-1)/stride+1,(W-1)/stride+1].
 * dv_instance_norm_act_f32: nn.InstanceNorm2d (affine=False) + activation over BC planes of HW floats
 *   (core/submodule.py:79-107, igev_stereo_ddim.py:100-117); in-place allowed (out == in). */
int dv_conv2d_fewin_f32(const float* in, const float* w, const float* bias, const float* ch_scale, const float* ch_shift,
                        float* out, int B, int Cin, int H, int W, int Cout, int k, int stride, int act,
                        dv_stream_t stream);
int dv_instance_norm_act_f32(const float* in, float* out, int BC, int HW, float eps, int act, dv_stream_t stream);

/* ---- IGEV: all-pairs correlation along the epipolar line + its level-1 pooling --------
 * Combined_Geo_Encoding_Volume.corr (KITTI15/core/geometry_ddim.py:72-80: einsum 'aijk,aijh->ajkh') and the
 * avg_pool2d([1,2]) of the pyramid (:28-30), once per stereo pair:
 *   corr0[b,y,x1,x2] = sum_c fmap1[b,c,y,x1] * fmap2[b,c,y,x2];   corr1[b,y,x1,x] = (corr0[..,2x] + corr0[..,2x+1]) / 2
 * fmap1 [B,C,H,W1], fmap2 [B,C,H,W2] (C <= 256); corr0 [B,H,W1,W2]; corr1 [B,H,W1,W2/2] (floor). */
int dv_allpairs_corr_f32(const float* fmap1, const float* fmap2, float* corr0, float* corr1, int B, int C, int H,
                         int W1, int W2, dv_stream_t stream);
/* Backward of the above for training (the reference differentiates the einsum of geometry_ddim.py:72-80 through the
 * lookup of every GRU iteration, igev_stereo_ddim.py:441-443).  dcorr0 [B,H,W1,W2] is the TOTAL gradient of corr0: corr1
 * is only its avg_pool (:28-30) and dv_geo_filter_lookup_bwd_f32 folds that level in.
 *   dfmap1[b,c,y,x1] = sum_x2 dcorr0[b,y,x1,x2] * fmap2[b,c,y,x2];   dfmap2[b,c,y,x2] = sum_x1 dcorr0[b,y,x1,x2] * fmap1[b,c,y,x1]
 * dfmap1 [B,C,H,W1] or dfmap2 [B,C,H,W2] may be NULL (not both): that gradient is not computed.  C <= 256.  The sums
 * over an image width run inside one wave in a fixed order -- no split-K, no atomics: the same bits on every launch. */
int dv_allpairs_corr_bwd_f32(const float* dcorr0, const float* fmap1, const float* fmap2, float* dfmap1, float* dfmap2,
                             int B, int C, int H, int W1, int W2, dv_stream_t stream);

/* ---- IGEV: geometry-encoding-volume lookup with the noise filter -----------------------
 * Combined_Geo_Encoding_Volume.__call__ (KITTI15/core/geometry_ddim.py:33-69), 2 pyramid levels,
 * radius 4: per pixel, (geo[c,:] * noise[:]) linearly sampled at disp/2^i + {-4..4} plus the all-pairs
 * correlation row sampled at coords/2^i - disp/2^i + {-4..4}.
 * geo [B,C,D,h,w]; corr0 [B,h,w,W2] (= corr() :72-80), corr1 [B,h,w,W2/2] (its avg_pool, :28-30);
 * disp, coords [B,h,w]; noisy: the [B,D,h,w] filter tensor, read as B*h*w rows of D floats (the
 * reference's raw reshape, :37); out [B, 2*(9C+9), h, w], channel order (geo0, corr0, geo1, corr1). */
int dv_geo_filter_lookup_f32(const float* geo, const float* corr0, const float* corr1,
                             const float* disp, const float* coords, const float* noisy, float* out,
                             int B, int C, int D, int h, int w, int W2, int radius, dv_stream_t stream);
/* Backward of the lookup for training (geometry_ddim.py:33-69 differentiated once per GRU iteration of the train loop,
 * igev_stereo_ddim.py:441-443).  The lookup is linear in the volume and in the correlation rows, so only grad_out
 * [B,2*(9C+9),h,w], disp, coords and noisy are read -- with the forward's sample positions, zero padding and raw-reshape
 * noise rows.  dgeo [B,C,D,h,w] and dcorr0 [B,h,w,W2] are caller-allocated; either may be NULL (not both) and is then
 * skipped.  dcorr0 includes the pooled level's share (corr1 = avg_pool of corr0, :28-30, factor 1/2): feed it to
 * dv_allpairs_corr_bwd_f32 (geometry_ddim.py:72-80).  Every output element has exactly one writer and is written exactly
 * once (zero outside the pixel's window): no atomics, no memset needed, the same bits on every launch.  radius 4 only. */
int dv_geo_filter_lookup_bwd_f32(const float* grad_out, const float* disp, const float* coords, const float* noisy,
                                 float* dgeo, float* dcorr0, int B, int C, int D, int h, int w, int W2, int radius,
                                 dv_stream_t stream);
/* The same lookup FUSED with the 1x1 convolution that consumes it in IGEV's update block (BasicMotionEncoder.convc1 +
 * bias + ReLU, KITTI15/core/update.py:79,:89): out[b, co, y, x] = act(bias[co] + sum_ch w[co, ch] * lookup[b, ch, y, x]),
 * out [B,64,h,w]; the [B,2*(C*9+9),h,w] lookup tensor is never written.  `wpacked` = dv_geo_lookup_conv1x1_pack_weights_f32 of
 * the nn.Conv2d weight [64, 2*(C*9+9)] (dv_geo_lookup_conv1x1_packed_floats(C) floats); Cout must be 64, radius 4. */
size_t dv_geo_lookup_conv1x1_packed_floats(int C);
int dv_geo_lookup_conv1x1_pack_weights_f32(const float* w, float* wpacked, int C, dv_stream_t stream);
int dv_geo_filter_lookup_conv1x1_f32(const float* geo, const float* corr0, const float* corr1, const float* disp,
                                     const float* coords, const float* noisy, const float* wpacked, const float* bias,
                                     float* out, int B, int C, int D, int h, int w, int W2, int radius, int Cout, int act,
                                     dv_stream_t stream);

/* ---- weight gradient of the 3-D convolutions (training) ---------------------
 * dW[co, ci, t] = sum_{b, o} g[b, co, o] * x[b, ci, stride*o + t - p] for the convolutions of dv_conv3d_f32
 * (cubic k in {1, 3}, p = (k-1)/2, stride in {1, 2}; k = 1 needs stride 1); x [B,Cin,D,H,W], g [B,Cout,Do,Ho,Wo],
 * dw [Cout,Cin,k,k,k], all fp32 and contiguous.  Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32) with the K
 * dimension (B*Do*Ho*Wo) split over blocks: every split writes its partial into `workspace`
 * (dv_conv3d_wgrad_workspace_floats floats, at most 48 MB; 0 = unsupported arguments) and a second kernel sums the
 * splits in a fixed order -- no atomics, the same bits on every launch.
 * The weight gradient of ConvTranspose3d(k3, s2, p1, op1) with weight [Cin_t,Cout_t,3,3,3] is this call with x and g
 * exchanged: x = the transposed convolution's output gradient (Cin = Cout_t, D = 2*D_t), g = its input (Cout = Cin_t). */
size_t dv_conv3d_wgrad_workspace_floats(int B, int Cin, int D, int H, int W, int Cout, int k, int stride);
int dv_conv3d_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int D, int H,
                        int W, int Cout, int k, int stride, dv_stream_t stream);

/* ---- training: backward of ConvTranspose3d(k4, s2, p1) (csrc/deconv3d_k4_bwd.hip) ---------------------
 * The hourglass's conv3_up / conv2_up / conv1_up (KITTI15/core/igev_stereo_ddim.py:44-51, BasicConv deconv
 * core/submodule.py:9-35; 48 -> 32, 32 -> 16, 16 -> 8).  w [Ci,Co,4,4,4], x [B,Ci,D,H,W], g = the output gradient
 * [B,Co,2D,2H,2W] (zero outside the volume), t in [0,4)^3, all fp32 and contiguous; any D, H, W >= 1 and any channel
 * counts (tiles are padded inside the kernels).  Exact fp32 on v_mfma_f32_16x16x4_f32, no atomics: the same bits on
 * every launch.
 *   input gradient   dx[b,ci,i]  = sum_{co,t} g[b,co,2i-1+t] * w[ci,co,t]   one fma chain of Co*64 products per element;
 *                    weights packed once per step by dv_deconv3d_k4s2_dgrad_pack_weights_f32
 *                    (dv_deconv3d_k4s2_dgrad_packed_floats floats).  W % 4 != 0 or pointers off 16 bytes: scalar path.
 *   weight gradient  dw[ci,co,t] = sum_{b,i} x[b,ci,i] * g[b,co,2i-1+t]     over bricks of 2 x 4 x 8 x positions, the
 *                    brick range split over blocks: every split writes its partial into `workspace`
 *                    (dv_deconv3d_k4s2_wgrad_workspace_floats floats = splits * Ci * Co * 64, at most 48 MB; 0 = invalid
 *                    shape) and a second kernel adds the splits in split order.  Inside a split, blocks of narrow
 *                    channel tiles deal the brick's rows to 2 or 4 waves whose chains are added in wave order. */
size_t dv_deconv3d_k4s2_dgrad_packed_floats(int Ci, int Co);
int dv_deconv3d_k4s2_dgrad_pack_weights_f32(const float* w /*[Ci,Co,4,4,4]*/, float* wpacked, int Ci, int Co,
                                            dv_stream_t stream);
int dv_deconv3d_k4s2_dgrad_f32(const float* g, const float* wpacked, float* dx, int B, int Ci, int D, int H, int W,
                               int Co, dv_stream_t stream);
size_t dv_deconv3d_k4s2_wgrad_workspace_floats(int B, int Ci, int D, int H, int W, int Co);
int dv_deconv3d_k4s2_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Ci, int D, int H,
                               int W, int Co, dv_stream_t stream);

/* ---- training: weight gradient of ConvTranspose2d(k4, s2, p1) (csrc/deconv2d_k4_bwd.hip) ---------------
 * IGEV's `spx_2_gru.conv1` (32 -> 32, BasicConv deconv core/submodule.py:9-35 inside Conv2x :36-76) and `spx_gru`
 * (64 -> 9 with bias, KITTI15/core/igev_stereo_ddim.py:110-112), differentiated by the reference at every GRU iteration
 * (`upsample_disp` :203-211 in the train loop :441-457).  w [Ci,Co,4,4], x [B,Ci,H,W], g = the output gradient
 * [B,Co,2H,2W] (zero outside the image), all fp32 and contiguous; any H, W >= 1 and any channel counts:
 *   dw[ci,co,ky,kx] = sum_{b,i,j} x[b,ci,i,j] * g[b,co,2i-1+ky,2j-1+kx]
 * Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), M = the 16 taps of one output channel, N = Ci, K = B*H*W, the
 * stride-2 taps of g gathered from an LDS halo; K (bricks of 4 x 16 input pixels of the whole batch) is split over
 * blocks, every split writes its partial into `workspace` (dv_deconv2d_k4s2_wgrad_workspace_floats floats =
 * splits * Ci * Co * 16, at most 48 MB, 16-byte aligned; 0 = invalid shape) and a second kernel adds the splits in split
 * order -- no atomics, the same bits on every launch of a shape.  (The input gradient runs on the forward kernels.) */
size_t dv_deconv2d_k4s2_wgrad_workspace_floats(int B, int Ci, int H, int W, int Co);
int dv_deconv2d_k4s2_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Ci, int H, int W,
                               int Co, dv_stream_t stream);

/* ---- training: 2-D convolution weight gradient (csrc/conv2d_wgrad.hip) -------------------------------
 * The backward of the dilated `convbn` / BasicBlock / conv8 layers of refinenet_version3 (KITTI12/models/
 * pwcnet_ddim.py:251-306, submodule.py:21-24, :192-215) with respect to the weights:
 *   dw[co, ci, ky, kx] = sum_{b, y, x} g[b, co, y, x] * x[b, ci, y + (ky-1)*d, x + (kx-1)*d]
 * (k in {1, 3}, stride 1, padding = dilation d in 1..16; x is zero outside the image); x [B,Cin,H,W], g [B,Cout,H,W],
 * dw [Cout,Cin,k,k], all fp32 and contiguous.  Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32) with the K dimension
 * (B*H*W) split over blocks: every split writes its partial into `workspace` (dv_conv2d_wgrad_workspace_floats floats,
 * at most 48 MB; 0 = unsupported arguments) and a second kernel sums the splits in a fixed order -- no atomics, the same
 * bits on every launch. */
size_t dv_conv2d_wgrad_workspace_floats(int B, int Cin, int H, int W, int Cout, int k, int dilation);
int dv_conv2d_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int H, int W,
                        int Cout, int k, int dilation, dv_stream_t stream);

/* ---- training: weight gradient of the update block's convolutions (csrc/conv2d_wgrad_cat.hip) ----------
 * The backward of ConvGRU's convz / convr / convq (KITTI15/core/update.py:26-40), of BasicMotionEncoder's convc1 /
 * convc2 / convd2 / conv (update.py:74-94), of DispHead.conv1 (update.py:15-24) and of mask_feat_4 (update.py:115-117)
 * with respect to the weights, over the VIRTUAL channel concatenation of dv_conv2d_cat_f32:
 *   dw[co, ci, ky, kx] = sum_{b, y, x} g[b, co, y, x] * X[b, ci, y + ky - p, x + kx - p],   X = cat(inputs, dim=1)
 * (k in {1, 3}, p = (k-1)/2, stride 1, dilation 1, X zero outside the image).  `inputs` / `channels` are HOST arrays of
 * n_inputs (1..4) device pointers [B,channels[i],H,W] and their channel counts (any positive counts); g [B,Cout,H,W];
 * dw [Cout, sum(channels), k, k]; all fp32 and contiguous.  Implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32),
 * 64 x 64 block tiles, staging double-buffered through registers; the K dimension (bricks of 2 x 32 output positions of
 * the whole batch) is split over blocks, every split writes its partial into `workspace`
 * (dv_conv2d_wgrad_cat_workspace_floats floats = splits * Cout * Cin * k * k, at most 48 MB; 0 = unsupported arguments)
 * and a second kernel sums the splits in split order -- no atomics, the same bits on every launch of a shape. */
size_t dv_conv2d_wgrad_cat_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout, int k);
int dv_conv2d_wgrad_cat_f32(const float* const* inputs, const int* channels, int n_inputs, const float* g, float* dw,
                            float* workspace, int B, int H, int W, int Cout, int k, dv_stream_t stream);

/* ConvGRU gate arithmetic of the training route (update.py:36-39; csrc/gru_gates.hip), elementwise over n floats (float4
 * bodies on 16-byte aligned pointers, scalar otherwise):
 *   dv_gru_reset_mul_f32        rh = r * h
 *   dv_gru_blend_f32            out = h + z * (q - h)   -- (1 - z) h + z q in the form, and with the rounding, of
 *                               dv_conv2d_gated_f32's blend epilogue: the training forward equals the eval forward's bits
 *   dv_gru_gates_bwd_blend_f32  dq_pre = dh' z (1 - q^2),  dz_pre = dh' (q - h) z (1 - z),  dh = dh' (1 - z)
 *   dv_gru_gates_bwd_reset_f32  dr_pre = d(rh) h r (1 - r),  dh += d(rh) r
 * z, r, q are the gates AFTER their non-linearity; *_pre are gradients of the convolutions' outputs. */
int dv_gru_reset_mul_f32(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream);
int dv_gru_blend_f32(const float* z, const float* q, const float* h, float* out, size_t n, dv_stream_t stream);
int dv_gru_gates_bwd_blend_f32(const float* dh_new, const float* z, const float* q, const float* h, float* dq_pre,
                               float* dz_pre, float* dh, size_t n, dv_stream_t stream);
int dv_gru_gates_bwd_reset_f32(const float* drh, const float* r, const float* h, float* dr_pre, float* dh, size_t n,
                               dv_stream_t stream);

/* Weight gradient of the single-input-channel convolution of dv_conv2d_1in_f32 (BasicMotionEncoder.convd1, 7x7,
 * KITTI15/core/update.py:78, :91): dw[co, 0, ky, kx] = sum_{b,y,x} g[b,co,y,x] * x[b,0,y+ky-p,x+kx-p], k = 7,
 * p = 3; x [B,1,H,W], g [B,Cout,H,W], dw [Cout,1,k,k].  Fixed summation order, no atomics. */
int dv_conv2d_1in_wgrad_f32(const float* x, const float* g, float* dw, int B, int H, int W, int Cout, int k,
                            dv_stream_t stream);

/* ---- mixed-precision training of the update block (csrc/conv2d_wgrad_cat_f16.hip, body in csrc/conv2d_wgrad_cat_mp.h) ----
 * dv_conv2d_wgrad_cat_f16: the weight gradient of dv_conv2d_wgrad_cat_f32 (same arguments, same virtual concatenation)
 * as KITTI15/core/update.py:26-142 computes it under `autocast(enabled=args.mixed_precision)` (train_stereo.py:146-173):
 *   dw[co, ci, ky, kx] = sum_{b, y, x} r16(g[b, co, y, x]) * r16(X[b, ci, y + ky - p, x + kx - p])
 * both float32 operands rounded to fp16 (nearest even) while they are staged, products accumulated in fp32 on
 * v_mfma_f32_16x16x32_f16, dw written as UNROUNDED float32 (the reference rounds it to fp16 before the cast back to the
 * float32 parameter: a deliberate difference).  A g or x beyond the fp16 range becomes Inf, and Inf / NaN appears in dw.
 * 64 x 64 block tiles, bricks of 4 x 32 output positions, K split over blocks into `workspace`
 * (dv_conv2d_wgrad_cat_f16_workspace_floats floats, at most 48 MB; 0 = unsupported arguments), summed in split order by a
 * second kernel: no atomics, the same bits on every launch of a shape. */
size_t dv_conv2d_wgrad_cat_f16_workspace_floats(const int* channels, int n_inputs, int B, int H, int W, int Cout, int k);
int dv_conv2d_wgrad_cat_f16(const float* const* inputs, const int* channels, int n_inputs, const float* g, float* dw,
                            float* workspace, int B, int H, int W, int Cout, int k, dv_stream_t stream);

/* ConvGRU gate arithmetic of the training forward (csrc/gru_gates.hip) with the rounding points of dv_conv2d_f16_cat's
 * epilogues (every result rounded to fp16, the operands taken as they are: fp16-exact on the route):
 *   dv_gru_reset_mul_f16   rh = r16(r * h)
 *   dv_gru_blend_f16       out = r16(r16(r16(1 - z) * h) + r16(z * q))
 * The backward of both stays on dv_gru_gates_bwd_*_f32. */
int dv_gru_reset_mul_f16(const float* r, const float* h, float* rh, size_t n, dv_stream_t stream);
int dv_gru_blend_f16(const float* z, const float* q, const float* h, float* out, size_t n, dv_stream_t stream);

/* ---- training: IGEV's once-per-pair 2-D front (csrc/igev_front_bwd.hip) -------------------------------
 * What `IGEVStereo_ddim.forward` computes before the cost volume (KITTI15/core/igev_stereo_ddim.py:364-377, :395-398)
 * needs two backward kernels beside the convolution ones above; both are fp32, contiguous, atomics-free (every output
 * element written once, the same bits on every launch of a shape).
 * dv_instance_norm_act_bwd_f32: backward of dv_instance_norm_act_f32 -- nn.InstanceNorm2d (affine=False) + activation of
 *   BasicConv_IN (core/submodule.py:79-107), the stems (igev_stereo_ddim.py:100-103) and `spx_4` (:104-108) -- over BC
 *   planes of HW floats.  x: the SAVED PRE-NORM tensor, g: the gradient of the activated output, act in {DV_ACT_NONE,
 *   DV_ACT_RELU, DV_ACT_LEAKY}.  Mean and rstd are recomputed with the forward's sums (its bits);
 *     x_hat = (x - mean) * rstd,  gh = g * act'(x_hat)   (act' = 0 / 0.01 where x_hat <= 0, like torch),
 *     dx = rstd * (gh - mean(gh) - x_hat * mean(gh * x_hat)).
 *   HW = 1 gives zeros.  dx must not alias x or g.
 * dv_conv2d_fewin_wgrad_f32: weight gradient of dv_conv2d_fewin_f32 (Cin <= 4, k in {3,5,7}, stride in {1,2}, padding
 *   k/2) -- `stem_2[0]` (3 -> 32, k3, s2, igev_stereo_ddim.py:100), `cnet.conv1` (3 -> 64, k7, s2, core/extractor.py:197)
 *   and a plain backbone's `conv_stem` (core/extractor.py:337):
 *     dw[co,ci,ky,kx] = sum_{b,y,x} g[b,co,y,x] * x[b,ci,y*stride-k/2+ky,x*stride-k/2+kx]   (x zero outside the image)
 *   x [B,Cin,H,W], g [B,Cout,Ho,Wo] with Ho = (H-1)/stride+1, dw [Cout,Cin,k,k].  The reduction over B*Ho*Wo (bricks of
 *   8 x 16 output pixels) is split over blocks, every split writes its partial into `workspace`
 *   (dv_conv2d_fewin_wgrad_workspace_floats floats = splits * Cout * Cin * k * k, at most 48 MB; 0 = unsupported
 *   arguments) and a second kernel adds the splits in split order.  The images are data: there is no input gradient. */
int dv_instance_norm_act_bwd_f32(const float* x, const float* g, float* dx, int BC, int HW, float eps, int act,
                                 dv_stream_t stream);
size_t dv_conv2d_fewin_wgrad_workspace_floats(int B, int Cin, int H, int W, int Cout, int k, int stride);
int dv_conv2d_fewin_wgrad_f32(const float* x, const float* g, float* dw, float* workspace, int B, int Cin, int H, int W,
                              int Cout, int k, int stride, dv_stream_t stream);

/* ---- metrics (SceneFlow/utils/metrics.py:22-65) -------------------------------
 * Per-image sums over pixels with mask!=0: sums[b] = { n_mask, n_gt_pos, sum|gt-est|,
 * n_D1 (err>3 & err/|gt|>0.05), n_err>1, n_err>2, n_err>3, 0 } as fp64 [B,8].
 * The <0.1 mask-ratio skip and the means are taken by the caller. */
int dv_masked_metrics_f32(const float* est, const float* gt, const uint8_t* mask, double* sums,
                          int B, int HW, dv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFUVOLUME_HIP_H */
