"""The ONE list of environment switches this package reads (INTEGRATION.md section 5 is generated from it).

Nothing here changes results silently on the default path: every switch is either an opt-in alternative that gives the same
bits (side stream, hipGraph replay), a documented numerics alternative (`DV_CONV_PRECISION`), or plumbing.  `overrides()`
returns the ones that are set; bench.py prints that dict in its JSON line as `env_overrides`, so a measured number carries
the switches it was measured under.  `route(knob)` is the one implementation of the ``DV_TRAIN_*`` route switches: no
other module of the package reads one of them from the environment.  The native library reads NO environment variable (tests pin kernel choices through
`dv_*_set_*` hooks of the C ABI)."""
from __future__ import annotations

import os

KNOBS = {
    # name: (default, where it is read, what it does)
    "DV_LIB_PATH": ("<package>/libdiffuvolume_hip.so", "_lib.py at import",
                    "load another build of the same C ABI (A/B of kernel variants, tools/build_variant.sh)"),
    "DV_CONV_PRECISION": ("f32", "submodule.default_conv_precision() when a plan is built",
                          "f32 = Winograd / polyphase fp32 MFMA kernels; f32_direct = direct implicit GEMM everywhere; "
                          "f16x3 = split-fp16 products (opt-in, not the contract's arithmetic)"),
    "DV_S2PP": ("1", "submodule.Conv3dPlan when a stride-2 plan is built",
                "0 = the stride-2 3-D layers on the direct kernel instead of the polyphase one (tests)"),
    "DV_TRAIN_CONV3D": ("hip", "train3d.route() on every training convolution",
                        "torch = the 3-D convolutions of ACVNet_DDIM training on F.conv3d / F.conv_transpose3d instead of "
                        "the HIP forward, input-gradient and weight-gradient kernels (A/B runs, tests)"),
    "DV_TRAIN_CONV2D": ("hip", "train2d.route() on every training convolution of refinenet3 and of IGEV's update block",
                        "torch = the 2-D convolutions of PWCNet_ddim's refinement network and the convolutions and ConvGRU gate "
                        "arithmetic of IGEV's update block in training on F.conv2d / torch expressions instead of "
                        "the HIP forward, input-gradient and weight-gradient kernels (A/B runs, tests)"),
    "DV_TRAIN_LOOKUP": ("hip", "geometry_ddim.route() when a training-route volume is built and on each of its lookups",
                        "torch = IGEV's geometry lookup and all-pairs correlation in training as torch expressions (einsum, "
                        "gather) instead of the HIP forward kernels and their HIP backward kernels (A/B runs, tests)"),
    "DV_TRAIN_TAIL": ("hip", "train_tail.route() on every regression head of ACVNet_DDIM / PWCNet_ddim training",
                      "torch = the x4 trilinear upsampling + softmax + disparity regression of the training heads as the "
                      "torch expression (F.interpolate, F.softmax, disparity_regression; atomics in its backward) instead "
                      "of the fused HIP forward and its atomics-free HIP backward (A/B runs, tests)"),
    "DV_TRAIN_VOLUME": ("hip", "train_volume.route() on every cost volume ACVNet_DDIM / PWCNet_ddim build while autograd records",
                        "torch = the group-wise-correlation and concatenation volumes in training as the PyTorch statements "
                        "of submodule.py (pad / unfold / flip, products, mean, cat) instead of the eval kernels with the "
                        "atomics-free HIP backward of csrc/volume_bwd.hip (A/B runs, tests)"),
    "DV_TRAIN_REFINE": ("hip", "train_refine.route() on the refinement input of PWCNet_ddim training",
                        "torch = left - warp(right, disp) and their +-24 correlation in training as the PyTorch statements "
                        "(two F.grid_sample, a loop over 49 shifts; atomics in grid_sample's backward) instead of the fused "
                        "HIP forward and the atomics-free HIP backward of csrc/warp_corr.hip (A/B runs, tests)"),
    "DV_TRAIN_NORM": ("hip", "train_norm.route() on every BatchNorm3d of the ACVNet_DDIM / PWCNet_ddim 3-D stacks in training",
                      "torch = BatchNorm3d with batch statistics, the hourglass skip add and the ReLU / Mish behind it in "
                      "training as the PyTorch statements (F.batch_norm, the add, F.relu / x * tanh(softplus(x))) instead of the "
                      "fused HIP forward and the atomics-free HIP backward of csrc/bn3d_act.hip (A/B runs, tests)"),
    "DV_TRAIN_PATCH": ("hip", "train_patch.route() on the patch stencils of ACVNet_DDIM's attention branch in training",
                       "torch = the four depth-wise (1,3,3) convolutions behind the group-wise correlation volume (patch, "
                       "patch_l1..3) in training as the nn.Conv3d calls, slices and torch.cat (MIOpen's grouped convolutions "
                       "forward and backward) instead of the fused HIP forward of csrc/patch_volume.hip and the atomics-free "
                       "HIP backward of csrc/patch_volume_bwd.hip (A/B runs, tests)"),
    "DV_TRAIN_ATTN": ("hip", "train_attn.route() on the bottleneck window attention of ACVNet_DDIM's hourglasses in training",
                      "torch = attention_block.forward in training as the PyTorch statements (pad, permute copies, F.linear, two "
                      "batched matmuls, a softmax over a materialised [B, windows, 16, 64, 64] tensor, the 1x1x1 convolution) "
                      "instead of the fused HIP forward of csrc/window_attn.hip and the atomics-free HIP backward of "
                      "csrc/window_attn_bwd.hip (A/B runs, tests)"),
    "DV_TRAIN_NET2D": ("torch", "train_net2d.route() on the 2-D networks of ACVNet_DDIM / PWCNet_ddim training: both feature "
                       "CNNs, ACV's concatconv, the BatchNorm2d layers of refinenet3 and the resize of PCW's refinement feature",
                       "hip = Conv2d + BatchNorm2d + ReLU / Mish (+ the BasicBlock's skip) on the HIP convolution routes of "
                       "train2d and the fused kernels of csrc/bn3d_act.hip, and F.interpolate(bilinear, align_corners=True) "
                       "on the inference kernel with the atomics-free backward of csrc/resize_bwd.hip, so that every "
                       "gradient repeats bit for bit; torch = the nn.Module calls (MIOpen, ATen's atomic resize backward)"),
    "DV_TRAIN_LOSS": ("hip", "train_loss.route() on every call of the model_loss_* functions and of sequence_loss",
                      "torch = the reference's expression for every argument (est[mask], gt[mask] and a mean per prediction: "
                      "a nonzero with a host synchronisation, index tensors and gathered copies kept for the backward) "
                      "instead of the fused forward and backward of csrc/masked_loss.hip for float32 GPU tensors in one "
                      "shape (gt and the mask read once for all predictions, loss and gradients repeat bit for bit, "
                      "sequence_loss reads its metrics in one copy).  Anything else (CPU, float64, broadcasting shapes, a gt "
                      "that requires a gradient) is the torch expression on either value (A/B runs, tests)"),
    "DV_IGEV_OVERLAP": ("1", "update.BasicMultiUpdateBlock.OVERLAP at import",
                        "0 = the motion encoder on the main stream instead of a side stream (same bits)"),
    "DV_IGEV_GRAPH": ("0", "igev_loop.IGEVDiffusionLoop.use_graph at import",
                      "1 = replay the GRU iterations of a DDIM step as a hipGraph (same bits, no gain measured)"),
    "DV_DIST_BACKEND": ("nccl on GPUs, gloo on CPUs", "distributed.init_from_env()", "torch.distributed backend of the metric reduce"),
    "DV_BENCH_OVERSUBSCRIBE": ("unset", "bench.py", "1 = let N ranks share fewer GPUs (plumbing test of the N-rank path only)"),
    "DV_BENCH_SELF_LAUNCHED": ("unset", "bench.py (set by bench.py for the ranks it starts itself)", "internal marker"),
    "DV_FULL_PARITY": ("unset", "tests/", "1 = the long parity runs (all steps against float64, second pair, diagnostic networks)"),
}


def route(knob: str) -> str:
    """'hip' or 'torch': what the training route switch ``knob`` (a ``DV_TRAIN_*`` row of `KNOBS`) says now.  Read from
    the environment on every call; unset or empty is the row's default.  Every ``train_*.route`` is this function bound
    to its knob."""
    default = KNOBS[knob][0]
    r = os.environ.get(knob, default) or default
    if r not in ("hip", "torch"):
        raise ValueError(f"{knob} must be 'hip' or 'torch', got {r!r}")
    return r


def overrides() -> dict:
    """The switches of `KNOBS` that are set in this process's environment, with their values."""
    return {k: os.environ[k] for k in KNOBS if os.environ.get(k) not in (None, "")}
