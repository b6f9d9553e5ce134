"""diffuvolume_amd -- MI355X-native DiffuVolume hot path (cost volumes, DDIM volume filter,
3-D hourglass aggregation, regression) behind the reference's Python API.  The arithmetic
lives in hand-written gfx950 HIP kernels (csrc/, C ABI in include/diffuvolume_hip.h)."""
from ._lib import DiffuVolumeError, lib_path, load
from .submodule import (AttentionConcatVolume, build_concat_attention_volume, build_concat_volume, build_gwc_volume,
                        disparity_regression, upsample_softmax_regress)
from .acv_ddim import ACVNet, ACVNet_DDIM, __models__
from .loss import (model_loss_kitti12, model_loss_test, model_loss_train, model_loss_train_attn_only,
                   model_loss_train_freeze_attn)
from .pwcnet_ddim import PWCNet, PWCNet_G, PWCNet_GC, PWCNet_ddim
from .train_tail import upsample_softmax_regress_train
from .train_volume import build_concat_volume_train, build_gwc_volume_train
from .train_refine import warp_corr_train
from .train_norm import batch_norm_act_train
from .train_patch import patch_volume_train
from .train_attn import window_attention_train
from .train_net2d import resize_bilinear_train
from .train_loss import masked_loss_train, sequence_loss_train
from .train3d import (conv3d as conv3d_train, conv3d_k3s1_bf16, conv3d_k3s1_f16, conv3d_weight_grad_bf16,
                      conv3d_weight_grad_f16, precision_scope as train_precision_scope)

__all__ = ["ACVNet", "ACVNet_DDIM", "PWCNet", "PWCNet_ddim", "__models__", "build_gwc_volume", "build_concat_volume",
           "build_concat_attention_volume", "AttentionConcatVolume", "disparity_regression", "upsample_softmax_regress",
           "upsample_softmax_regress_train", "build_gwc_volume_train", "build_concat_volume_train",
           "warp_corr_train", "batch_norm_act_train", "patch_volume_train", "window_attention_train",
           "resize_bilinear_train", "masked_loss_train", "sequence_loss_train",
           "conv3d_train", "conv3d_k3s1_f16", "conv3d_weight_grad_f16", "conv3d_k3s1_bf16", "conv3d_weight_grad_bf16",
           "train_precision_scope",
           "DiffuVolumeError", "lib_path", "load", "model_loss_train", "model_loss_train_freeze_attn",
           "model_loss_train_attn_only", "model_loss_test", "model_loss_kitti12"]
# KITTI12/models/__init__.py:5-9: the origin network under both registry names and the DiffuVolume flavour
__models__ = dict(__models__, **{"gwcnet-g": PWCNet_G, "gwcnet-gc": PWCNet_GC,
                                 "pwc_ddimgc": lambda d: PWCNet_ddim(d, use_concat_volume=True)})
__version__ = "0.1.0"
