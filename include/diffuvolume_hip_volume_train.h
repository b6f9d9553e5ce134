/* diffuvolume_hip_volume_train.h -- C ABI of libdiffuvolume_hip.so, third table: the backward of the two cost-volume
 * builders (dv_gwc_volume_f32, dv_concat_volume_f32 / dv_concat_prob_volume_f32 of diffuvolume_hip.h), the warp +
 * correlation of PWCNet_ddim's refinement input in training, forward and backward, the BatchNorm3d (batch statistics)
 * + skip + activation of the ACV and PCW aggregation stacks in training, forward and backward, the backward of the
 * patch stencils of ACVNet_DDIM's attention branch (dv_patch_volume_runs_f32), the backward of the hourglass's
 * bottleneck window attention (dv_window_attn3d_f32), the backward of the align_corners=True bilinear resize
 * (dv_resize_bilinear_ac_f32), the depthwise 3x3 convolution of IGEV's MobileNetV2 backbone, forward and backward, and the
 * masked training losses of the three models, forward and backward.
 *
 * Bound by `_lib.VOLUME_TRAIN_SIGNATURES`, where every entry also carries the decision about its pointer and bounds
 * contract ("size only" or the GPU test that holds it); tests/test_volume_train_host.py reads that table.  A later
 * training entry is a row of that table and a declaration here.
 *
 * Conventions (those of diffuvolume_hip.h)
 *  - every pointer is a DEVICE pointer to a dense, contiguous row-major tensor in the reference's own layout
 *    (NCHW / NCDHW); outputs are caller-allocated;
 *  - nothing here allocates, frees, synchronises or keeps global mutable state; calls are re-entrant and are enqueued on
 *    `stream` of the current device;
 *  - alignment: a tensor operand needs only the alignment of its element type (4 bytes for float).  Like the forward
 *    builders, the entries take 16-byte accesses along W when W % 4 == 0 and every operand lies on a 16-byte line, and a
 *    one-thread-per-output kernel otherwise: the two agree within rounding (the sums over d run in the same order; the
 *    sum over c of `ds` is chunked on the fast path), not necessarily in bits;
 *  - every element of an output is written exactly once, in a fixed summation order, without atomics: the same call gives
 *    the same bits on every launch, and a batch gives the bits of its items run one by one;
 *  - a refused call launches nothing and writes nothing;
 *  - return value: 0 = ok, <0 = DV_ERR_* (bad argument), >0 = hipError_t.
 */
#ifndef DIFFUVOLUME_HIP_VOLUME_TRAIN_H
#define DIFFUVOLUME_HIP_VOLUME_TRAIN_H

#include "diffuvolume_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- group-wise correlation volume, backward -------------------------------------------------------------------------
 * What autograd computes for build_gwc_volume (SceneFlow/models/submodule.py:209-238) in training.
 *   ref, tgt [B,C,H,W], dvol [B,G,D,H,W] -> dref, dtgt [B,C,H,W];  cpg = C / G, g = c / cpg
 *   dref[b,c,y,x]  = (1/cpg) sum_{d<D, d<=x}   dvol[b,g,d,y,x]    tgt[b,c,y,x-d]
 *   dtgt[b,c,y,x'] = (1/cpg) sum_{d<D, x'+d<W} dvol[b,g,d,y,x'+d] ref[b,c,y,x'+d]
 * Either output may be NULL (a frozen side costs nothing); both NULL: DV_ERR_NULL.  C % G != 0: DV_ERR_SHAPE. */
int dv_gwc_volume_bwd_f32(const float* ref, const float* tgt, const float* dvol, float* dref, float* dtgt, int B, int C,
                          int H, int W, int D, int G, dv_stream_t stream);

/* ---- concatenation volume, backward ----------------------------------------------------------------------------------
 * What autograd computes for build_concat_volume (SceneFlow/models/submodule.py:180-191; KITTI12/models/submodule.py:86-97
 * with zero_left) and for a scale s[b,d,y,x] multiplied onto it (the softmax(att) * volume * noisy of
 * SceneFlow/models/acv_ddim.py:694-704), i.e. for the forward
 *   vol[b,c,d,y,x] = s ref[b,c,y,x]   (0 for x < d with zero_left),   vol[b,C+c,d,y,x] = s tgt[b,c,y,x-d]   (0 for x < d)
 *   ref, tgt [B,C,H,W], s [B,D,H,W] or NULL (= 1), dvol [B,2C,D,H,W] -> dref, dtgt [B,C,H,W], ds [B,D,H,W]
 *   dref[b,c,y,x]  = sum_d s dvol[b,c,d,y,x]                                       (d <= x only with zero_left)
 *   dtgt[b,c,y,x'] = sum_{d, x'+d<W} s[b,d,y,x'+d] dvol[b,C+c,d,y,x'+d]
 *   ds[b,d,y,x]    = sum_c dvol[b,c,d,y,x] ref[b,c,y,x] + [x>=d] sum_c dvol[b,C+c,d,y,x] tgt[b,c,y,x-d]
 * Each output may be NULL; all three NULL: DV_ERR_NULL.  ref / tgt are read only for ds and may be NULL without it.
 * ds without s: DV_ERR_NULL.  s together with zero_left: DV_ERR_UNSUPPORTED (dv_concat_prob_volume_f32 has no such
 * forward).  On the fast path ds is summed over chunks of 8 channels in `workspace`
 * (dv_concat_volume_bwd_workspace_floats floats, [chunks][B,D,H,W]) and then over the chunks in ascending order;
 * `workspace` is required (DV_ERR_NULL) when ds is wanted and that size is not 0, and may be NULL otherwise. */
size_t dv_concat_volume_bwd_workspace_floats(int B, int C, int H, int W, int D);
int dv_concat_volume_bwd_f32(const float* ref, const float* tgt, const float* s, const float* dvol, float* dref,
                             float* dtgt, float* ds, float* workspace, int B, int C, int H, int W, int D, int zero_left,
                             dv_stream_t stream);

/* ---- warp + correlation of the refinement input, forward and backward ------------------------------------------------
 * The part of PWCNet_ddim's refinement input that carries gradients (KITTI12/models/pwcnet_ddim.py:719-725):
 *   F = warp(right, disp) (KITTI12/models/submodule.py:137-176: bilinear taps of grid_sample with align_corners=False on a
 *   grid normalised by W-1 / H-1, times the validity m = [sampled ones >= 0.999]),
 *   diff[B,C,H,W] = left - F,   corr[B,49,H,W] = build_corrleation_volume(left, F, 24, 1):
 *   corr[i+24,x] = (1/C) sum_c left[c,x] F[c,x-i] for 0 <= i <= x;  corr[24-k,x] = (1/C) sum_c left[c,x] F[c,W-k+x] for
 *   x < k (the reference's slices pair the first k columns of left with the LAST k columns of F), 0 elsewhere.
 * diff and corr are channels [0,C) and [3C+1,3C+50) of dv_refine_inputs_f32 bit for bit.  disp is [B,H,W].
 * C > 32, maxshift != 24 and W < 24: DV_ERR_UNSUPPORTED;  B or H above 65535: DV_ERR_SHAPE  (as dv_refine_inputs_f32). */
int dv_warp_corr_f32(const float* left, const float* right, const float* disp, float* diff, float* corr, int B, int C,
                     int H, int W, int maxshift, dv_stream_t stream);

/* What autograd computes for those statements; F is recomputed, not saved.  With inv = 1/C and md = 24:
 *   dleft[c,x]  = g_diff[c,x] + inv (sum_{0<=i<=md, i<=x} g_corr[i+md,x] F[c,x-i] + sum_{1<=k<=md, x<k} g_corr[md-k,x] F[c,W-k+x])
 *   dF[c,x']    = -g_diff[c,x'] + inv (sum_{0<=i<=md, x'+i<W} g_corr[i+md,x'+i] left[c,x'+i]
 *                                      + sum_{1<=k<=md, x'>=W-k} g_corr[md-k,x'-(W-k)] left[c,x'-(W-k)])
 *   dright[c,ys,xs] = sum over the output pixels (y,x) and their in-range taps t on (ys,xs) of m(y,x) w_t(y,x) dF[c,y,x],
 *                     in the order y ascending, x ascending
 *   ddisp[y,x]  = -m W/max(W-1,1) sum_c dF[c,y,x] ((R[y0,x0+1] - R[y0,x0]) (fy+1-iy) + (R[y0+1,x0+1] - R[y0+1,x0]) (iy-fy)),
 *                 R = right, taps outside the image count as 0; the validity carries no gradient.
 * Each output may be NULL (not wanted); all three NULL: DV_ERR_NULL.  `workspace` holds m dF
 * (dv_warp_corr_bwd_workspace_floats = B C H W floats); it is required (DV_ERR_NULL) when dright is wanted and may be NULL
 * otherwise.  Refusals as dv_warp_corr_f32. */
size_t dv_warp_corr_bwd_workspace_floats(int B, int C, int H, int W);
int dv_warp_corr_bwd_f32(const float* left, const float* right, const float* disp, const float* g_diff, const float* g_corr,
                         float* dleft, float* dright, float* ddisp, float* workspace, int B, int C, int H, int W,
                         int maxshift, dv_stream_t stream);

/* ---- BatchNorm3d with batch statistics + skip + activation, forward and backward --------------------------------------
 * What nn.BatchNorm3d computes in training mode, the optional add of a second tensor and the activation behind it, as the
 * 3-D stacks of ACVNet_DDIM (ReLU) and PWCNet_ddim (Mish) apply them to a convolution's output:
 *   x, skip, y [B,C,S] with S = D*H*W;  mean, invstd, gamma, beta, running_mean, running_var [C];  n = B*S
 *   mean[c] = (1/n) sum_{b,s} x[b,c,s],  var[c] = (1/n) sum (x - mean)^2,  invstd = 1 / sqrt(var + eps)
 *   y = act((x - mean) * invstd * gamma + beta + skip),  act in {DV_ACT_NONE, DV_ACT_RELU, DV_ACT_MISH}
 * Every kernel gives one block one chunk of 8192 consecutive floats of one (b,c) slab.  Reductions are one partial per block
 * in `workspace`, then a combine launch of one wave per channel that merges a channel's partials in a fixed order in
 * double: no atomics, the same bits on every launch.  Here, unlike the builders above, the 16-byte path (S % 4 == 0 and
 * every tensor operand on a 16-byte line) and the scalar path assign the same elements to the same thread in the same
 * order, so they agree in bits.
 *
 * dv_bn3d_train_workspace_floats: floats of `workspace` for both launching entries below, C * (3 P + 2) with
 *   P = B * ceil(S / 8192) partials per channel; 0 for a non-positive size.
 *
 * dv_bn3d_stats_f32: partials (count, mean, M2) in the shifted form (sums of x - K and (x - K)^2 with K the chunk's first
 *   element, in fp32), merged with Chan's formula.  Writes mean and invstd.  running_mean / running_var: both or neither
 *   (DV_ERR_NULL otherwise); when given they are updated in place, r = (1 - momentum) r + momentum * (mean | var n/(n-1)).
 *   B*S == 1: DV_ERR_UNSUPPORTED (no variance; PyTorch raises there too).  eps < 0: DV_ERR_SHAPE.
 *
 * dv_bn3d_apply_act_f32: y from x, the statistics and the affine parameters; skip may be NULL.
 *   act outside the three above: DV_ERR_UNSUPPORTED.
 *
 * dv_bn3d_act_bwd_f32: with z recomputed by the forward's statement and xhat = (x - mean) invstd,
 *   dz = dy act'(z);  ReLU' = [z > 0];  Mish' = t + z (1 - t^2) e / (1 + e) with e = exp(z), n = e (e + 2), t = n / (n + 2)
 *   (dv_act's e and n), 1 for z > 20
 *   dskip = dz,  dbeta[c] = sum dz,  dgamma[c] = sum dz xhat,
 *   dx = gamma invstd (dz - dbeta / n - xhat dgamma / n)
 *   Pass 1 writes dz (into dskip when that is wanted, otherwise into dx as scratch; not at all when act is DV_ACT_NONE and
 *   skip is NULL, where dz is dy) and the per-block sums; the combine gives dbeta and dgamma; pass 2 forms dx in place.
 *   dx, dskip, dgamma, dbeta may each be NULL (not wanted: dx == NULL saves pass 2); all four NULL: DV_ERR_NULL.
 *   dskip without skip: DV_ERR_NULL.  dx must not overlap dy, x or skip.  Refusals as above. */
size_t dv_bn3d_train_workspace_floats(int B, int C, int S);
int dv_bn3d_stats_f32(const float* x, float* mean, float* invstd, float* running_mean, float* running_var,
                      float* workspace, int B, int C, int S, float momentum, float eps, dv_stream_t stream);
int dv_bn3d_apply_act_f32(const float* x, const float* skip, const float* mean, const float* invstd, const float* gamma,
                          const float* beta, float* y, int B, int C, int S, int act, dv_stream_t stream);
int dv_bn3d_act_bwd_f32(const float* dy, const float* x, const float* skip, const float* mean, const float* invstd,
                        const float* gamma, const float* beta, float* dx, float* dskip, float* dgamma, float* dbeta,
                        float* workspace, int B, int C, int S, int act, dv_stream_t stream);

/* ---- patch stencils of the attention branch, backward ------------------------------------------------------------------
 * What autograd computes for the four depth-wise Conv3d(.., (1,3,3), groups) the attention branch applies to the group-wise
 * correlation volume (SceneFlow/models/acv_ddim.py:181-188 define them, :377-381 apply them):
 *   gwc = patch(gwc);  out = cat(patch_l1(gwc[:, :8]), patch_l2(gwc[:, 8:24]), patch_l3(gwc[:, 24:40]))   dilation 1 / 2 / 3
 * i.e. for the forward dv_patch_volume_runs_f32 (diffuvolume_hip.h), which stays as it is.  Per plane (b, g, d) with dl the
 * dilation of group g, (k-1) the 2-D tap offset (ky-1, kx-1), x = gwc, go = dout:
 *   gwc, dout, dgwc [B,G,D,H,W];  w1, w2, dw1, dw2 [G,9]
 *   mid[p]  = sum_k w1[k] x[p + (k-1)]          for p in the image, 0 outside (recomputed on chip, never stored)
 *   dmid[p] = sum_k w2[k] go[p - (k-1) dl]      for p in the image, 0 outside;  go = 0 outside
 *   dgwc[p] = sum_k w1[k] dmid[p - (k-1)]
 *   dw2[g,k] = sum_{b,d,p} go[p] mid[p + (k-1) dl],   dw1[g,k] = sum_{b,d,p} dmid[p] x[p + (k-1)]
 * One pass over 16 x 128 tiles reads gwc and dout once and writes dgwc once.  Each block leaves its 18 partial sums in the
 * `workspace` slot of its block index; a second launch adds a group's slots in a fixed order in double.  The groups are
 * given as HOST-side runs of consecutive groups with one dilation (as to dv_patch_volume_runs_f32): one launch per run and
 * per 65535 planes.  16-byte accesses when W % 4 == 0 and gwc, dout and dgwc lie on 16-byte lines, element-wise accesses
 * otherwise; here the two paths do the same arithmetic in the same order and agree in bits.
 *
 * dgwc, dw1, dw2 may each be NULL (not wanted; that work is skipped: without dw1 and dw2 gwc is not read), and a result
 * has the same bits whichever of the others are wanted; all three NULL: DV_ERR_NULL.  `workspace`
 * (dv_patch_volume_bwd_workspace_floats = G * B*D*ceil(H/16)*ceil(W/128) * 18 floats; 0 for a non-positive size) is
 * required (DV_ERR_NULL) when dw1 or dw2 is wanted and may be NULL otherwise.  dgwc must not overlap gwc or dout.
 * Non-positive sizes, runs that do not tile 0..G in order, a dilation outside 1..3: DV_ERR_SHAPE. */
size_t dv_patch_volume_bwd_workspace_floats(int B, int G, int D, int H, int W);
int dv_patch_volume_bwd_f32(const float* gwc, const float* w1, const float* w2, const float* dout, float* dgwc, float* dw1,
                            float* dw2, float* workspace, int B, int G, int D, int H, int W, int nruns, const int* run_g0,
                            const int* run_ng, const int* run_dil, dv_stream_t stream);

/* ---- 4x4x4 window attention of the hourglass bottleneck, backward ---------------------------------------------------------
 * What autograd computes for attention_block.forward (SceneFlow/models/submodule.py:398-429), which the hourglass
 * (SceneFlow/models/acv_ddim.py:56-93) applies at its bottleneck, i.e. for the forward dv_window_attn3d_f32
 * (diffuvolume_hip.h), which stays as it is.  C = 128, heads = 16, head dim 8; D % 4 == 0; H and W are zero-padded up to
 * whole windows.  Per window, X [64,128] the tokens (0 at padded tokens), dY [64,128] the gradient of the output (0 at
 * padded tokens: the forward crops them), per head with its slices Q, K, V of QKV = X Wqkv^T + bqkv:
 *   S = 8^-0.5 Q K^T (-1000 between a padded and an unpadded token when H AND W are padded),  P = softmax(S),  O = P V,
 *   Y = Om Wp^T + bp with Om the heads of O side by side
 *   dOm = dY Wp,  Dq = rowsum(dO * O),  dV = P^T dO,  dP = dO V^T,  dS = P * (dP - Dq),  dQ = 8^-0.5 dS K,  dK = 8^-0.5 dS^T Q
 *   dx = dQKV Wqkv at unpadded tokens;  dqkv_w [384,128] = sum over tokens dQKV^T X;  dqkv_b [384] = sum over ALL tokens of
 *   dQKV (padded tokens are keys and values with qkv = bias, so their dK and dV rows count);  dproj_w [128,128] = sum dY^T Om;
 *   dproj_b [128] = sum dY.
 * x, dout, dx [B,128,D,H,W]; qkv_w [384,128], qkv_b [384], proj_w [128,128] and their gradients in the same shapes.
 * P is recomputed with the forward's arithmetic.  One block per window writes dx and, channel-major, Om and dQKV into
 * `workspace`; the two weight gradients are then split-K GEMMs over the tokens (partials summed in split order); dqkv_b adds
 * one partial per window and dproj_b the elements of dout in a fixed order in double.  No atomics: the same bits on every
 * launch, and dx of a batch has the bits of its items run one by one.  16-byte stores to dx (to the workspace) when
 * W % 4 == 0 and dx (the workspace) lies on a 16-byte line, element stores otherwise, with the same bits; x and dout need
 * 4-byte alignment only.
 *
 * dx, dqkv_w, dqkv_b, dproj_w, dproj_b may each be NULL (not wanted; that work is skipped), and a result has the same bits
 * whichever of the others are wanted; all five NULL: DV_ERR_NULL.  `workspace`
 * (dv_window_attn3d_bwd_workspace_floats = 512 B D H W + 384 windows + min(T, 64) 384*128 + min(T, 128) 128*128 with
 * T = B ceil(D H W / 32) chunks of tokens; 0 for invalid or unsupported arguments) is required (DV_ERR_NULL) when dqkv_w, dqkv_b or
 * dproj_w is wanted and may be NULL otherwise.  dx and the workspace must not overlap x or dout.
 * Refusals, before the device is touched, as dv_window_attn3d_f32: NULL inputs DV_ERR_NULL; non-positive sizes or
 * D % 4 != 0 DV_ERR_SHAPE; C != 128 or heads != 16 DV_ERR_UNSUPPORTED; qkv_w or proj_w off a 16-byte line DV_ERR_ALIGN. */
size_t dv_window_attn3d_bwd_workspace_floats(int B, int C, int D, int H, int W, int heads);
int dv_window_attn3d_bwd_f32(const float* x, const float* qkv_w, const float* qkv_b, const float* proj_w, const float* dout,
                             float* dx, float* dqkv_w, float* dqkv_b, float* dproj_w, float* dproj_b, float* workspace,
                             int B, int C, int D, int H, int W, int heads, dv_stream_t stream);

/* ---- bilinear resize with align_corners=True, backward -------------------------------------------------------------------
 * What autograd computes for F.interpolate(x, [H, W], mode="bilinear", align_corners=True), i.e. for the forward
 * dv_resize_bilinear_ac_f32 (diffuvolume_hip.h), which stays as it is: its exact adjoint in its own weights.
 *   dy [BC,H,W] -> dx [BC,h,w];  sy = (h-1)/(H-1) (0 for H == 1),  fy = sy Y,  y0 = (int)fy,  y1 = y0 + [y0 < h-1],
 *   ly = fy - y0,  hy = 1 - ly,  all in the forward's float expressions;  x likewise
 *   dx[bc,i,j] = sum_{Y,X} dy[bc,Y,X] (hy [y0 == i] + ly [y1 == i]) (hx [x0 == j] + lx [x1 == j])
 * A gather (ATen's backward scatters with atomics): y0 is monotone in Y, so the rows that touch source row i are one range,
 * found by bisection on the forward's expression.  One block per plane, band of 8 source rows and tile of 64 source
 * columns stages the dy rows it needs in LDS, sums along X (ascending), then along Y (ascending).  16-byte loads of dy when
 * W % 4 == 0 and dy lies on a 16-byte line, element loads otherwise, with the same bits; dx needs 4-byte alignment only.
 * Any sizes the forward takes: H == h, h == 1, downscaling, ratios that are no integers.
 * A NULL pointer or a non-positive size: DV_ERR_NULL (without a plane there is no element either pointer could name);
 * more than 2^31 - 1 blocks (BC ceil(h/8) ceil(w/64)): DV_ERR_SHAPE.  dx must not overlap dy. */
int dv_resize_bilinear_ac_bwd_f32(const float* dy, float* dx, int BC, int h, int w, int H, int W, dv_stream_t stream);

/* ---- depthwise 3x3 convolution of MobileNetV2's blocks, forward and backward ----------------------------------------------
 * nn.Conv2d(C, C, 3, stride, 1, groups=C, bias=False) as timm's mobilenetv2_100 (the backbone of KITTI15/core/extractor.py:
 * 327-361) uses it in its DepthwiseSeparableConv and InvertedResidual blocks, with the eval BatchNorm behind it folded into
 * scale / shift and its ReLU6 applied inside the launch:
 *   x [B,C,H,W], w [C,9] (tap = ky*3 + kx), scale, shift [C] -> out [B,C,Ho,Wo],  Ho = (H-1)/stride + 1,  Wo = (W-1)/stride + 1
 *   conv[b,c,oy,ox] = sum_{ky,kx} w[c,ky,kx] x[b,c, oy stride + ky - 1, ox stride + kx - 1]     (0 outside the image)
 *   out = act(conv * scale[c] + shift[c])
 * stride: 1 or 2 (anything else DV_ERR_UNSUPPORTED).  scale and shift: both or neither (one of them NULL: DV_ERR_NULL); NULL
 * is the identity and skips the multiply-add.  act: DV_ACT_NONE or DV_ACT_RELU; relu_max > 0 caps a ReLU from above
 * (min(max(v, 0), relu_max): 6 for ReLU6), 0 leaves it open.  Any other act, a negative or NaN relu_max, or a relu_max
 * without DV_ACT_RELU: DV_ERR_UNSUPPORTED.
 *
 * One wave works on one tile of one (b,c) plane: a lane owns four consecutive output columns and walks a band of output
 * rows, reading each input row once (one 16-byte quad, two at stride 2; the halo columns come from the neighbouring lanes)
 * and keeping the three rows an output needs in registers.  The tiles depend on H and W only and are handed to a capped
 * grid by a grid-stride loop; the nine taps are summed in the order ky, kx by one fmaf each.  So the same call gives the
 * same bits on every launch and an item of a batch has the bits of the item run alone.  16-byte loads when W % 4 == 0 and
 * x lies on a 16-byte line, 16-byte stores when Wo % 4 == 0 and out does, element accesses otherwise: the same arithmetic,
 * the same bits.
 *
 * Backward of the bare convolution (BatchNorm and the activation are autograd nodes of their own in training):
 *   dy [B,C,Ho,Wo] -> dx [B,C,H,W], dw [C,9]
 *   dx[b,c,iy,ix] = sum over the taps (ky,kx) with (iy + 1 - ky) and (ix + 1 - kx) multiples of stride and the quotients
 *                   (oy, ox) inside dy, of w[c,ky,kx] dy[b,c,oy,ox]: a gather, every element written once.  At stride 2
 *                   the parity of iy and ix picks 1, 2, 2 or 4 taps.
 *   dw[c,ky,kx]   = sum_{b,oy,ox} dy[b,c,oy,ox] x[b,c, oy stride + ky - 1, ox stride + kx - 1]: one partial of nine floats
 *                   per wave tile in `workspace`, then one wave per channel adds the channel's partials in a fixed order in
 *                   double.  No atomics.
 * dx or dw may be NULL (not wanted; that launch is skipped and the other has the same bits); both NULL: DV_ERR_NULL.
 * x is read only for dw and w only for dx; each is required (DV_ERR_NULL) with that output and may be NULL without it.
 * `workspace` (dv_dwconv3x3_bwd_workspace_floats = 9 B C tiles-per-plane floats; 0 for a non-positive size or another
 * stride) is required (DV_ERR_NULL) when dw is wanted.  dx must not overlap dy.  Gradients repeat bit for bit, and dx of
 * a batch has the bits of its items run one by one.
 * All three: a NULL tensor DV_ERR_NULL, a non-positive size or more than 0x7fff0000 tiles DV_ERR_SHAPE, before anything
 * touches the device. */
int dv_dwconv3x3_f32(const float* x, const float* w, const float* scale, const float* shift, float* out, int B, int C,
                     int H, int W, int stride, int act, float relu_max, dv_stream_t stream);
size_t dv_dwconv3x3_bwd_workspace_floats(int B, int C, int H, int W, int stride);
int dv_dwconv3x3_bwd_f32(const float* x, const float* w, const float* dy, float* dx, float* dw, float* workspace, int B,
                         int C, int H, int W, int stride, dv_stream_t stream);

/* ---- the masked training losses, forward and backward -------------------------------------------------------------------
 * The weighted sum of masked means every training script of the three models ends in (SceneFlow/models/loss.py,
 * KITTI12/models/loss.py: smooth-L1 / L1 over est[mask]; KITTI15/train_stereo.py:33-62: sequence_loss), for K predictions
 * in one pass instead of one boolean gather per prediction:
 *   pred_k, gt [n] float32;  d = pred_k[i] - gt[i];  g_k = |d| (DV_LOSS_L1) or, DV_LOSS_SMOOTH_L1 with beta 1,
 *   0.5 d^2 for |d| < 1 and |d| - 0.5 otherwise
 *   selected(i): DV_MASK_U8        mask is n bytes, non-zero selects (a bool tensor)
 *                DV_MASK_VALID_F32 mask is n floats `valid`: valid[i] >= 0.5f && sqrtf(gt[i] * gt[i]) < max_disp, in float32
 *   sum_k = sum_{selected} g_k,  count = #selected,   loss = sum_k w_k * sum_k / count
 * `preds`, `weights`, `kinds` (and `dpreds`) are HOST arrays of K entries; preds[k] / dpreds[k] are device pointers.  They are
 * read during the call only (they travel to the kernels by value).  1 <= K <= DV_MASKED_LOSS_MAX_K; more predictions are
 * several calls, whose sums do not depend on each other.
 *
 * Forward: one grid-stride launch of at most DV_MASKED_LOSS_MAX_BLOCKS blocks of 256 threads, a thread taking quads of four
 * consecutive elements, leaves one partial per block and figure, in double, in `workspace`
 * (dv_masked_loss_workspace_floats floats = 2 * blocks * (K + 6), on an 8-byte line; 0 for arguments the forward refuses);
 * a one-block launch adds the partials in a fixed order in double and writes
 *   stats [K + 6] double: sum_0 .. sum_{K-1}, count, and for prediction `metric_pred` (-1: none, the four are 0)
 *                         sum |d|, #(|d| < 1), #(|d| < 3), #(|d| < 5) over the selected pixels, then 1.0 if a selected gt is
 *                         infinite and 0.0 otherwise
 *   loss  [1] float32:    the expression above, combined in double and rounded once; NaN for count == 0 (the mean of an
 *                         empty selection) and when a selected d is NaN.
 * Backward: one launch writes every element of every dpreds[k] != NULL exactly once:
 *   dpred_k[i] = gout[0] * w_k / count * g_k'(d) at selected pixels, g' = sign(d) with sign(0) = 0 for L1, d for |d| < 1
 *   and sign(d) otherwise for smooth-L1, NaN for a NaN d;  0 at unselected pixels BY SELECTION, whatever pred and gt hold
 *   there (NaN, Inf);  all 0 for count == 0.  `gout` is a DEVICE float (the incoming gradient of the loss, e.g. a
 *   GradScaler's scale), `stats` the forward's.  dpreds[k] == NULL: that prediction needs no gradient and is skipped;
 *   all NULL: DV_ERR_NULL.  dpreds must not overlap an input.
 * No atomics in any launch: the same call gives the same bits.  16-byte loads and stores (the mask bytes four at a time) when
 * every tensor operand lies on a 16-byte line (a byte mask: a 4-byte line), element accesses otherwise and at the tail, with
 * the same assignment of elements to threads and the same order of additions: the same bits.
 * Refused before anything touches the device: a NULL pointer (an entry of preds included) DV_ERR_NULL; n <= 0, K outside
 * 1..DV_MASKED_LOSS_MAX_K or metric_pred outside -1..K-1 DV_ERR_SHAPE; an unknown kind or mask mode, a NaN max_disp with
 * DV_MASK_VALID_F32 DV_ERR_UNSUPPORTED; workspace or stats off an 8-byte line DV_ERR_ALIGN. */
#define DV_MASKED_LOSS_MAX_K 24
#define DV_MASKED_LOSS_MAX_BLOCKS 1024
#define DV_LOSS_L1 0
#define DV_LOSS_SMOOTH_L1 1
#define DV_MASK_U8 0
#define DV_MASK_VALID_F32 1
size_t dv_masked_loss_workspace_floats(int K, long long n);
int dv_masked_loss_fwd_f32(const float* const* preds, const double* weights, const int* kinds, const float* gt,
                           const void* mask, int mask_mode, float max_disp, int K, long long n, int metric_pred,
                           float* workspace, double* stats, float* loss, dv_stream_t stream);
int dv_masked_loss_bwd_f32(const float* const* preds, const double* weights, const int* kinds, const float* gt,
                           const void* mask, int mask_mode, float max_disp, const double* stats, const float* gout,
                           float* const* dpreds, int K, long long n, dv_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFUVOLUME_HIP_VOLUME_TRAIN_H */
