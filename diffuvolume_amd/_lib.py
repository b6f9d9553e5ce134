"""ctypes binding of libdiffuvolume_hip.so (the C ABI in include/diffuvolume_hip.h, include/diffuvolume_hip_train.h,
include/diffuvolume_hip_volume_train.h, include/diffuvolume_hip_amp3d.h, include/diffuvolume_hip_amp3d_bf16.h and
include/diffuvolume_hip_amp2d_bf16.h).

There is deliberately no CPU / eager fallback: if the library is missing or a
kernel reports an error the call raises.  ``import torch`` happens first so the
library resolves libamdhip64 against the HIP runtime PyTorch already loaded
(one runtime, one set of streams).

What every route needs around an entry is here once: ``check_f32`` (a float32 tensor on the GPU),
``launch(name, device, *args)`` (the call on PyTorch's current stream of that device, its code checked),
``timed_launch(tag, flops, nbytes, name, device, *args)`` (the same call under the kernel timer of profiling.py) and
``workspace(name, device, *dims)`` (the float32 scratch a ``*_workspace_floats`` entry sizes; None for 0).
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_longlong, c_size_t, c_void_p
from pathlib import Path

import torch  # noqa: F401  (must precede the dlopen below)

from .profiling import timed

# DV_LIB_PATH: load another build of the same ABI (A/B of compiler flags / kernel variants); default = the in-tree .so
_LIB_PATH = Path(os.environ.get("DV_LIB_PATH") or Path(__file__).resolve().parent / "libdiffuvolume_hip.so")
_lib = None


class DvDdimCoef(Structure):
    """struct dv_ddim_coef (include/diffuvolume_hip.h)."""
    _fields_ = [("sqrt_recip_alpha", c_double), ("sqrt_recipm1_alpha", c_double),
                ("sqrt_alpha_next", c_double), ("c", c_double), ("sigma", c_double),
                ("dif_thr", c_float), ("unc_thr", c_float), ("cof", c_float), ("last", c_int),
                ("clamp_max", c_float), ("ens_dif_thr", c_float)]


P = c_void_p
I = c_int
# name -> (restype, argtypes); mirrors include/diffuvolume_hip.h one to one
SIGNATURES = {
    "dv_version": (c_int, []),
    "dv_error_string": (c_char_p, [I]),
    "dv_gwc_volume_f32": (c_int, [P, P, P, I, I, I, I, I, I, P]),
    "dv_concat_volume_f32": (c_int, [P, P, P, I, I, I, I, I, I, P]),
    "dv_concat_attn_volume_f32": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "dv_concat_prob_volume_f32": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "dv_pointwise_expand_packed_floats": (c_size_t, [I, I]),
    "dv_pointwise_expand_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_pointwise_expand_f32": (c_int, [P, P, P, I, I, I, I, P]),
    "dv_softmax_d_f32": (c_int, [P, P, I, I, I, P]),
    "dv_mul_f32": (c_int, [P, P, P, c_size_t, P]),
    "dv_conv3d_rank1_filter_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_noise_prepare_f32": (c_int, [P, P, P, I, I, I, P]),
    "dv_noise_prepare_f64": (c_int, [P, P, P, P, I, I, I, P]),
    "dv_conv3d_packed_floats": (c_size_t, [I, I, I]),
    "dv_conv3d_pack_weights_f32": (c_int, [P, P, I, I, I, P]),
    "dv_conv3d_f32": (c_int, [P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dv_conv3d_set_s2_tile": (c_int, [I]),
    "dv_conv3d_set_c1z": (c_int, [I, I]),
    "dv_conv3d_f16x3_packed_bytes": (c_size_t, [I, I]),
    "dv_conv3d_f16x3_pack_weights": (c_int, [P, P, I, I, P]),
    "dv_conv3d_f16x3_f32": (c_int, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv3d_wino_packed_floats": (c_size_t, [I, I]),
    "dv_conv3d_wino_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_conv3d_wino_f32": (c_int, [P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv3d_wino3_packed_floats": (c_size_t, [I, I]),
    "dv_conv3d_wino3_supported": (c_int, [I, I, I, I, I]),
    "dv_conv3d_wino3_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_conv3d_wino3_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv3d_s2pp_supported": (c_int, [I, I, I, I, I]),
    "dv_conv3d_s2pp_packed_floats": (c_size_t, [I, I]),
    "dv_conv3d_s2pp_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_conv3d_s2pp_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_deconv3d_packed_floats": (c_size_t, [I, I]),
    "dv_deconv3d_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_deconv3d_k3s2_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_deconv3d_pl_supported": (c_int, [I, I, I, I, I, I]),
    "dv_deconv3d_set_impl": (c_int, [I]),
    "dv_deconv3d_pl_set_max_blocks": (c_int, [I]),
    "dv_deconv3d_k4_packed_floats": (c_size_t, [I, I]),
    "dv_deconv3d_k4_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_deconv3d_k4s2_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_packed_floats": (c_size_t, [I, I, I, I]),
    "dv_conv2d_pack_weights_f32": (c_int, [P, P, I, I, I, I, P]),
    "dv_conv2d_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_conv2d_gated_f32": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_conv2d_cat_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_auto_kslices": (c_int, [I, I, I, I, I, I, I]),
    "dv_conv2d_cat_ksplit_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_conv2d_s2_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_wino_packed_floats": (c_size_t, [I, I]),
    "dv_conv2d_wino_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_conv2d_wino_cat_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, P]),
    "dv_conv2d_wino_cat_pair_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_conv2d_wino_dil_cat_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_refine_inputs_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, P]),
    "dv_space_to_batch2_f32": (c_int, [P, P, I, I, I, I, P]),
    "dv_conv2d_wino_auto_kslices": (c_int, [I, I, I, I, I]),
    "dv_conv2d_wino_cat_ksplit_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_wino_cat_pair_ksplit_f32": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_wino_s2b_f32": (c_int, [P, P, I, P, P, P, P, I, I, I, I, I, P]),
    "dv_batch_to_space_f32": (c_int, [P, P, I, I, I, I, I, P]),
    "dv_softmax_regress_f32": (c_int, [P, P, I, I, I, I, P]),
    "dv_feature_gate_f32": (c_int, [P, P, P, I, I, I, I, I, P]),
    "dv_deconv3d_k3s2_redir_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_patch_volume_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, P]),
    "dv_patch_volume_runs_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, I, P, P, P, P]),
    "dv_window_attn3d_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_upsample_softmax_regress_f32": (c_int, [P, P, P, I, I, I, I, I, P]),
    "dv_upsample_softmax_uncertainty_f32": (c_int, [P, P, P, I, I, I, I, I, P]),
    "dv_disparity_regression_f32": (c_int, [P, P, I, I, I, I, P]),
    "dv_encode_two_hot_f32": (c_int, [P, P, I, I, I, P]),
    "dv_ddim_step": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, POINTER(DvDdimCoef), P]),
    "dv_context_upsample_f32": (c_int, [P, P, P, I, I, I, c_float, I, P]),
    "dv_allpairs_corr_f32": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "dv_allpairs_corr_bwd_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, P]),
    "dv_conv2d_1in_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, P]),
    "dv_conv2d_1in_f16": (c_int, [P, P, P, P, I, I, I, I, I, I, P]),
    "dv_conv2d_f16_packed_bytes": (c_size_t, [I, I, I]),
    "dv_conv2d_f16_pack_weights": (c_int, [P, P, I, I, I, P]),
    "dv_conv2d_f16_auto_kslices": (c_int, [I, I, I, I, I]),
    "dv_conv2d_f16_cat": (c_int, [P, P, I, P, P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_conv2d_f16_cat_ksplit": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_f16_cat_pair": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P]),
    "dv_conv2d_f16_cat_pair_ksplit": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_resize_bilinear_ac_f32": (c_int, [P, P, I, I, I, I, I, P]),
    "dv_avg_pool3s2_f32": (c_int, [P, P, I, I, I, P]),
    "dv_conv2d_fewin_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_instance_norm_act_f32": (c_int, [P, P, I, I, ctypes.c_float, I, P]),
    "dv_geo_filter_lookup_f32": (c_int, [P, P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_geo_filter_lookup_bwd_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_geo_lookup_conv1x1_packed_floats": (c_size_t, [I]),
    "dv_geo_lookup_conv1x1_pack_weights_f32": (c_int, [P, P, I, P]),
    "dv_geo_filter_lookup_conv1x1_f32": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, P]),
    "dv_masked_metrics_f32": (c_int, [P, P, P, P, I, I, P]),
    "dv_conv3d_wgrad_workspace_floats": (c_size_t, [I, I, I, I, I, I, I, I]),
    "dv_conv3d_wgrad_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, I, I, P]),
    "dv_deconv3d_k4s2_dgrad_packed_floats": (c_size_t, [I, I]),
    "dv_deconv3d_k4s2_dgrad_pack_weights_f32": (c_int, [P, P, I, I, P]),
    "dv_deconv3d_k4s2_dgrad_f32": (c_int, [P, P, P, I, I, I, I, I, I, P]),
    "dv_deconv3d_k4s2_wgrad_workspace_floats": (c_size_t, [I, I, I, I, I, I]),
    "dv_deconv3d_k4s2_wgrad_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, P]),
    "dv_feature_gate_bwd_workspace_floats": (c_size_t, [I, I, I, I, I]),
    "dv_feature_gate_bwd_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, P]),
    "dv_conv2d_wgrad_workspace_floats": (c_size_t, [I, I, I, I, I, I, I]),
    "dv_conv2d_wgrad_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, I, P]),
    "dv_conv2d_wgrad_cat_workspace_floats": (c_size_t, [P, I, I, I, I, I, I]),
    "dv_conv2d_wgrad_cat_f32": (c_int, [P, P, I, P, P, P, I, I, I, I, I, P]),
    "dv_conv2d_1in_wgrad_f32": (c_int, [P, P, P, I, I, I, I, I, P]),
    "dv_conv2d_wgrad_cat_f16_workspace_floats": (c_size_t, [P, I, I, I, I, I, I]),
    "dv_conv2d_wgrad_cat_f16": (c_int, [P, P, I, P, P, P, I, I, I, I, I, P]),
    "dv_context_upsample_bwd_f32": (c_int, [P, P, P, P, P, P, I, I, I, c_float, I, P]),
    "dv_deconv2d_k4s2_wgrad_workspace_floats": (c_size_t, [I, I, I, I, I]),
    "dv_deconv2d_k4s2_wgrad_f32": (c_int, [P, P, P, P, I, I, I, I, I, P]),
    "dv_gru_reset_mul_f32": (c_int, [P, P, P, c_size_t, P]),
    "dv_gru_blend_f32": (c_int, [P, P, P, P, c_size_t, P]),
    "dv_gru_reset_mul_f16": (c_int, [P, P, P, c_size_t, P]),
    "dv_gru_blend_f16": (c_int, [P, P, P, P, c_size_t, P]),
    "dv_gru_gates_bwd_blend_f32": (c_int, [P, P, P, P, P, P, P, c_size_t, P]),
    "dv_gru_gates_bwd_reset_f32": (c_int, [P, P, P, P, P, c_size_t, P]),
    "dv_instance_norm_act_bwd_f32": (c_int, [P, P, P, I, I, ctypes.c_float, I, P]),
    "dv_conv2d_fewin_wgrad_workspace_floats": (c_size_t, [I, I, I, I, I, I, I]),
    "dv_conv2d_fewin_wgrad_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, I, P]),
}


# Second table: training entries declared in include/diffuvolume_hip_train.h (same library, same conventions).  They are
# kept out of SIGNATURES because every name there must be a row of the inference arena table or an exclusion next to it
# (tests/test_abi_arena_complete.py); the same decision for these is recorded in tests/test_regress_train_host.py.
TRAIN_SIGNATURES = {
    "dv_upsample_softmax_regress_bwd_workspace_floats": (c_size_t, [I, I, I, I]),
    "dv_upsample_softmax_regress_bwd_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, P]),
}


# Third table: include/diffuvolume_hip_volume_train.h.  name -> (restype, argtypes, decision): the decision about the
# entry's pointer and bounds contract sits beside its signature -- SIZE_ONLY, or held_by(<GPU test>) naming the test that
# calls the entry through offset views, between sentinels and with the arguments it refuses.
# tests/test_volume_train_host.py reads this table; a later training entry is a row here and a declaration in that header.
SIZE_ONLY = "only returns a size: launches nothing"


def held_by(test: str) -> str:
    return f"offset views, sentinel-guarded outputs and refusals are held by: {test}"


VOLUME_TRAIN_SIGNATURES = {
    "dv_gwc_volume_bwd_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, I, P],
                              held_by("test_gpu_volume_train.py::test_gwc_abi_offset_views_bounds_and_refusals")),
    "dv_concat_volume_bwd_workspace_floats": (c_size_t, [I, I, I, I, I], SIZE_ONLY),
    "dv_concat_volume_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, P],
                                 held_by("test_gpu_volume_train.py::test_concat_abi_offset_views_bounds_and_refusals")),
    "dv_warp_corr_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, P],
                         held_by("test_gpu_refine_train.py::test_warp_corr_abi_offset_views_bounds_and_refusals")),
    "dv_warp_corr_bwd_workspace_floats": (c_size_t, [I, I, I, I], SIZE_ONLY),
    "dv_warp_corr_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, P, I, I, I, I, I, P],
                             held_by("test_gpu_refine_train.py::test_warp_corr_abi_offset_views_bounds_and_refusals")),
    "dv_bn3d_train_workspace_floats": (c_size_t, [I, I, I], SIZE_ONLY),
    "dv_bn3d_stats_f32": (c_int, [P, P, P, P, P, P, I, I, I, c_float, c_float, P],
                          held_by("test_gpu_norm_train.py::test_bn3d_abi_offset_views_bounds_and_refusals")),
    "dv_bn3d_apply_act_f32": (c_int, [P, P, P, P, P, P, P, I, I, I, I, P],
                              held_by("test_gpu_norm_train.py::test_bn3d_abi_offset_views_bounds_and_refusals")),
    "dv_bn3d_act_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, P],
                            held_by("test_gpu_norm_train.py::test_bn3d_abi_offset_views_bounds_and_refusals")),
    "dv_patch_volume_bwd_workspace_floats": (c_size_t, [I, I, I, I, I], SIZE_ONLY),
    "dv_patch_volume_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, I, I, I, I, I, I, P, P, P, P],
                                held_by("test_gpu_patch_train.py::test_patch_bwd_abi_offset_views_bounds_and_refusals")),
    "dv_window_attn3d_bwd_workspace_floats": (c_size_t, [I, I, I, I, I, I], SIZE_ONLY),
    "dv_window_attn3d_bwd_f32": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P],
                                 held_by("test_gpu_attn_train.py::test_attn_bwd_abi_offset_views_bounds_and_refusals")),
    "dv_resize_bilinear_ac_bwd_f32": (c_int, [P, P, I, I, I, I, I, P],
                                      held_by("test_gpu_resize_bwd.py::test_resize_bwd_abi_offset_views_bounds_and_refusals")),
    "dv_dwconv3x3_f32": (c_int, [P, P, P, P, P, I, I, I, I, I, I, c_float, P],
                         held_by("test_gpu_dwconv.py::test_dwconv_abi_offset_views_bounds_and_refusals")),
    "dv_dwconv3x3_bwd_workspace_floats": (c_size_t, [I, I, I, I, I], SIZE_ONLY),
    "dv_dwconv3x3_bwd_f32": (c_int, [P, P, P, P, P, P, I, I, I, I, I, P],
                             held_by("test_gpu_dwconv.py::test_dwconv_abi_offset_views_bounds_and_refusals")),
    "dv_masked_loss_workspace_floats": (c_size_t, [I, c_longlong], SIZE_ONLY),
    "dv_masked_loss_fwd_f32": (c_int, [P, P, P, P, P, I, c_float, I, c_longlong, I, P, P, P, P],
                               held_by("test_gpu_loss_train.py::test_masked_loss_abi_offset_views_bounds_and_refusals")),
    "dv_masked_loss_bwd_f32": (c_int, [P, P, P, P, P, I, c_float, P, P, P, I, c_longlong, P],
                               held_by("test_gpu_loss_train.py::test_masked_loss_abi_offset_views_bounds_and_refusals")),
}


# Fourth table: include/diffuvolume_hip_amp3d.h, the fp16-MFMA products of the 3x3x3 stride-1 convolutions at train
# precision "f16" (train3d.py).  Same shape as the third table; tests/test_amp3d_host.py reads it.  There is no pack entry
# and no tuning hook here: the kernels read the module's raw float32 weight.
AMP3D_SIGNATURES = {
    "dv_conv3d_k3s1_f16_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, I, I, P],
                               held_by("test_gpu_amp3d_abi.py::test_conv3d_f16_abi_offset_views_bounds_and_refusals")),
    "dv_conv3d_wgrad_f16_workspace_floats": (c_size_t, [I, I, I, I, I, I], SIZE_ONLY),
    "dv_conv3d_wgrad_f16_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, P],
                                held_by("test_gpu_amp3d_abi.py::test_conv3d_wgrad_f16_abi_offset_views_bounds_and_refusals")),
}


# Fifth table: include/diffuvolume_hip_amp3d_bf16.h, the bf16-MFMA twins of the fourth table (train precision "bf16"):
# the same signatures, the same kernels instantiated for the other element type.  tests/test_amp3d_bf16_host.py reads it.
AMP3D_BF16_SIGNATURES = {
    "dv_conv3d_k3s1_bf16_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, I, I, P],
                                held_by("test_gpu_amp3d_bf16_abi.py::test_conv3d_bf16_abi_offset_views_bounds_and_refusals")),
    "dv_conv3d_wgrad_bf16_workspace_floats": (c_size_t, [I, I, I, I, I, I], SIZE_ONLY),
    "dv_conv3d_wgrad_bf16_f32": (c_int, [P, P, P, P, I, I, I, I, I, I, P],
                                 held_by("test_gpu_amp3d_bf16_abi.py::test_conv3d_wgrad_bf16_abi_offset_views_bounds_and_refusals")),
}


# Sixth table: include/diffuvolume_hip_amp2d_bf16.h, IGEV's update block at train precision "bf16": the bf16 twins of the
# fp16 entries of SIGNATURES (dv_conv2d_f16_*, dv_conv2d_1in_f16, dv_gru_*_f16, dv_conv2d_wgrad_cat_f16*), each with its
# twin's signature.  The sizes and the K-split choice are the fp16 entries' (dv_conv2d_f16_packed_bytes,
# dv_conv2d_f16_auto_kslices): they do not depend on the element type.  tests/test_update_bf16_host.py reads this table.
PACKS_WEIGHTS = "packs weights: writes the packed image only, held with the plan by the forward tests"
_HELD2D = "test_gpu_update_bf16_abi.py::"
AMP2D_BF16_SIGNATURES = {
    "dv_conv2d_bf16_pack_weights": (c_int, [P, P, I, I, I, P], PACKS_WEIGHTS),
    "dv_conv2d_bf16_cat": (c_int, [P, P, I, P, P, P, P, P, P, P, I, I, I, I, I, I, P],
                           held_by(_HELD2D + "test_conv2d_bf16_cat_abi_offset_views_bounds_and_refusals")),
    "dv_conv2d_bf16_cat_ksplit": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P],
                                  held_by(_HELD2D + "test_conv2d_bf16_cat_abi_offset_views_bounds_and_refusals")),
    "dv_conv2d_bf16_cat_pair": (c_int, [P, P, I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, P],
                                held_by(_HELD2D + "test_conv2d_bf16_pair_abi_offset_views_bounds_and_refusals")),
    "dv_conv2d_bf16_cat_pair_ksplit": (c_int, [P, P, I, P, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, P],
                                       held_by(_HELD2D + "test_conv2d_bf16_pair_abi_offset_views_bounds_and_refusals")),
    "dv_conv2d_1in_bf16": (c_int, [P, P, P, P, I, I, I, I, I, I, P],
                           held_by(_HELD2D + "test_conv2d_1in_bf16_abi_offset_views_bounds_and_refusals")),
    "dv_gru_reset_mul_bf16": (c_int, [P, P, P, c_size_t, P],
                              held_by(_HELD2D + "test_gru_gates_bf16_abi_offset_views_bounds_and_refusals")),
    "dv_gru_blend_bf16": (c_int, [P, P, P, P, c_size_t, P],
                          held_by(_HELD2D + "test_gru_gates_bf16_abi_offset_views_bounds_and_refusals")),
    "dv_conv2d_wgrad_cat_bf16_workspace_floats": (c_size_t, [P, I, I, I, I, I, I], SIZE_ONLY),
    "dv_conv2d_wgrad_cat_bf16": (c_int, [P, P, I, P, P, P, I, I, I, I, I, P],
                                 held_by(_HELD2D + "test_conv2d_wgrad_cat_bf16_abi_offset_views_bounds_and_refusals")),
}


class DiffuVolumeError(RuntimeError):
    pass


def lib_path() -> Path:
    return _LIB_PATH


def load() -> ctypes.CDLL:
    """Load (once) and type the shared library; raise loudly when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise DiffuVolumeError(
            f"{_LIB_PATH} is missing: build it with `python -m diffuvolume_amd._build` "
            "(there is no CPU fallback for the DiffuVolume hot path)")
    lib = ctypes.CDLL(os.fspath(_LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    tables = {**SIGNATURES, **TRAIN_SIGNATURES, **{k: v[:2] for k, v in VOLUME_TRAIN_SIGNATURES.items()},
              **{k: v[:2] for k, v in AMP3D_SIGNATURES.items()}, **{k: v[:2] for k, v in AMP3D_BF16_SIGNATURES.items()},
              **{k: v[:2] for k, v in AMP2D_BF16_SIGNATURES.items()}}
    for name, (res, args) in tables.items():
        fn = getattr(lib, name)          # AttributeError => ABI mismatch, also loud
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().dv_error_string(code).decode()
        raise DiffuVolumeError(f"{what} failed with code {code}: {msg}")


def stream_ptr() -> int:
    """Raw hipStream_t of PyTorch's current stream on the current device."""
    return torch.cuda.current_stream().cuda_stream


def ptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def check_f32(t, name: str) -> None:
    """Every route's tensor check: a float32 tensor on the GPU, or an error that names it."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise DiffuVolumeError(f"{name} is on {t.device}: this path only runs on the MI355X (HIP kernels, no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32, got {t.dtype}")


def launch(name: str, device, *args) -> None:
    """Call the entry ``name`` with ``args`` and PyTorch's current stream of ``device``; raise on its error code."""
    with torch.cuda.device(device):
        check(getattr(load(), name)(*args, stream_ptr()), name)


def timed_launch(tag: str, flops: float, nbytes: float, name: str, device, *args, issued: float = 0.0, valu: float = 0.0) -> None:
    """``launch`` as one record of the kernel timer (``profiling.timed``: what ``tag``, ``flops``, ``nbytes``, ``issued`` and
    ``valu`` mean).  The device is entered around the timer, whose events go to the current device's stream."""
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        timed(tag, flops, nbytes, lambda: check(fn(*args, stream_ptr()), name), issued, valu)


def workspace(name: str, device, *dims):
    """A float32 tensor on ``device`` of as many elements as the size entry ``name`` returns for ``dims``; None for 0."""
    n = getattr(load(), name)(*dims)
    return torch.empty(n, dtype=torch.float32, device=device) if n else None
