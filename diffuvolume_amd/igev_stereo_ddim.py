"""IGEV-Stereo + DiffuVolume: ``IGEVStereo_ddim``, the drop-in module (KITTI15/core/igev_stereo_ddim.py:118-224
constructor, :361-427 eval forward, :364-463 train branch as ``forward_train``).  Module / buffer names are the
reference's, so its checkpoints load with strict=True.  It is assembled from pieces that also stand alone:
  igev_layers    BasicConv, BasicConv_IN, Conv2x, ResidualBlock and the HIP / TORCH / TRAIN routes they run on
  igev_front2d   Feature, MultiBasicEncoder, IGEVFront2d: feature pyramid, stems, context encoder
  igev_volume    FeatureAtt, hourglass, IGEVCostVolume: gwc volume -> hourglass(8) -> initial disparity
  igev_upsample  context_upsample, IGEVUpsampler: the spx heads and the convex upsampling
  igev_loop      DynamicHead180, IGEVDiffusionLoop: the DDIM volume-filter loop around the GRU iterations
All of it runs on HIP kernels.  The MobileNetV2 backbone is injected (``Feature(backbone)``):
``mobilenetv2.MobileNetV2Features()`` is the real network under timm's parameter names and runs on the HIP kernels too
(depthwise 3x3 on csrc/dwconv2d.hip); a timm object runs as it is, and the pretrained weights are the caller's either
way.  Every name of the five modules is importable from here too."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from . import _lib, ddim
from .igev_front2d import Feature, MultiBasicEncoder, _front2d
from .igev_layers import (HIP, TRAIN, BasicConv, BasicConv_IN, Conv2x, Conv2x_IN, _Conv2xBase, _FewInPlan,  # noqa: F401
                          _PLAN_CACHE, _bn_tuple, _require_cuda, _stem, _train_mode, _wants_autograd, freeze_bn)
from .igev_loop import DynamicHead180, IGEVDiffusionLoop, round_gru_inputs_bf16, round_gru_inputs_f16
from .igev_upsample import (_context_upsample_launch, _context_upsample_shapes, _spx_init_train, _spx_plans,  # noqa: F401
                            _spx_train_key, _spx_train_plans, _upsample_disp, _upsample_disp_train, context_upsample)
from .igev_volume import (FeatureAtt, _cost_volume, _cost_volume_plans, _cost_volume_train, _run, _run_train,  # noqa: F401
                          _seq_plans, hourglass)
# every other name this module held before it was split: the same objects, importable from here as before
from .igev_front2d import *            # noqa: F401,F403
from .igev_layers import *             # noqa: F401,F403
from .igev_loop import *               # noqa: F401,F403
from .igev_upsample import *           # noqa: F401,F403
from .igev_volume import *             # noqa: F401,F403
from .submodule import PlanCache, _dev_f32, _gwc_volume_autograd  # noqa: F401


class IGEVStereo_ddim(PlanCache, nn.Module):
    """``IGEVStereo_ddim(args).forward(image1, image2, flow_full, flow_gt, iters=12, flow_init=None, test_mode=False)
    -> (pred, pred)`` (eval path, igev_stereo_ddim.py:361-427).  ``args``: hidden_dims, n_gru_layers, n_downsample,
    corr_levels, corr_radius, slow_fast_gru, max_disp, mixed_precision.  ``mixed_precision=True`` runs the update block
    of every GRU iteration under fp16 autocast like the reference (:242-246): its convolutions on fp16 MFMA with the
    reference's fp16 rounding points (csrc/conv2d_f16.hip); the front, hourglass(8), the geometry lookup,
    ``upsample_disp`` and the DDIM state stay float32.  The flag is read at every forward.
    ``feature``: the MobileNetV2 feature pyramid (``Feature(backbone)``); None = the reference's own construction from
    timm's pretrained ``mobilenetv2_100`` (core/extractor.py:327-335), which needs ``timm`` to be importable;
    ``cnet``: optional replacement for the context encoder.  ``sampling_timesteps`` / ``ensemble_cof`` are
    hard-coded to 2 / [0.6, 0.1, 0.3] in the reference (:124, :353); BASELINE config 5 asks for 20 steps.
    Training: ``forward`` refuses train mode; ``forward_train`` is the reference's train branch (:364-463) on the
    differentiable HIP routes and returns ``(init_disp, disp_preds)`` for ``loss.sequence_loss``."""

    def __init__(self, args, feature: Optional[nn.Module] = None, cnet: Optional[nn.Module] = None,
                 sampling_timesteps: int = 2, ensemble_cof: Optional[Sequence[float]] = None):
        super().__init__()
        if feature is None:
            # the reference's own construction (core/extractor.py:327-335): timm's pretrained MobileNetV2, when timm exists
            try:
                import timm
            except ImportError:
                timm = None
            if timm is None or not hasattr(timm, "create_model"):
                raise _lib.DiffuVolumeError(
                    "IGEVStereo_ddim(args) builds its feature pyramid from timm.create_model('mobilenetv2_100', "
                    "pretrained=True, features_only=True) like the reference (core/extractor.py:331); timm is not "
                    "importable here -- pass feature=Feature(backbone) (mobilenetv2.MobileNetV2Features(), the same "
                    "network under timm's parameter names, a timm model or synth.StubMobileNetV2())")
            feature = Feature(timm.create_model("mobilenetv2_100", pretrained=True, features_only=True))
        self.args = args
        self.scale = 1.0
        self.num_timesteps = 1000
        self.sampling_timesteps = sampling_timesteps
        self.is_ddim_sampling = sampling_timesteps < self.num_timesteps
        self.ddim_sampling_eta = 1
        self.renewal = self.use_ensemble = True
        if ensemble_cof is None:
            if sampling_timesteps != 2:
                raise ValueError("give ensemble_cof (S+1 weights) when sampling_timesteps != 2")
            ensemble_cof = (0.6, 0.1, 0.3)
        self.ensemble_cof = tuple(float(c) for c in ensemble_cof)
        ddim.register_schedule(self, self.num_timesteps)

        from .update import BasicMultiUpdateBlock
        hidden = list(args.hidden_dims)
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hidden, hidden], norm_fn="batch",
                                                                    downsample=args.n_downsample)
        self.update_block = BasicMultiUpdateBlock(args, hidden_dims=hidden)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hidden[i], hidden[i] * 3, 3, padding=1)
                                                for i in range(args.n_gru_layers)])
        self.time_embedding = DynamicHead180(180)
        self.feature = feature
        self.stem_2, self.stem_4 = _stem(3, 32), _stem(32, 48)
        self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.spx_2 = Conv2x_IN(24, 32, True)
        self.spx_4 = nn.Sequential(BasicConv_IN(96, 24, kernel_size=3, stride=1, padding=1),
                                   nn.Conv2d(24, 24, 3, 1, 1, bias=False), nn.InstanceNorm2d(24), nn.ReLU())
        self.spx_2_gru = Conv2x(32, 32, True)
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.conv = BasicConv_IN(96, 96, kernel_size=3, padding=1, stride=1)
        self.desc = nn.Conv2d(96, 96, kernel_size=1, padding=0, stride=1)
        self.corr_stem = BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1)
        self.corr_feature_att = FeatureAtt(8, 96)
        self.cost_agg = hourglass(8)
        self.classifier = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

    def _build_plans(self, slot):
        """The default slot: corr_stem and classifier of the cost volume.  Slot "spx": `spx_2_gru` (transposed conv + BN +
        LeakyReLU, concat with the 1/2-resolution stem, 3x3 conv + BN + LeakyReLU) and `spx_gru` (biased transposed conv
        to the 9 convex-upsampling logits).  Slot "spx_train": the same three layers for the training route."""
        if slot == "spx":
            return _spx_plans(self)
        if slot == "spx_train":
            return _spx_train_plans(self)
        return _cost_volume_plans(self)

    freeze_bn = freeze_bn

    # ---- pieces -----------------------------------------------------------------------------------------
    def upsample_disp(self, disp, mask_feat_4, stem_2x):
        """:209-217: spx_2_gru / spx_gru (3x3 HIP kernels; the transposed convolutions as four parity convolutions + pixel
        shuffle), then softmax over the 9 taps + context_upsample(disp*4) in one HIP pass.  Returns [B,1,4h,4w].  In train
        mode with autograd recording: the differentiable route of IGEVUpsampler."""
        return _upsample_disp(self, disp, mask_feat_4, stem_2x, "spx", "spx_train")

    def cost_volume(self, match_left, match_right, features_left):
        """:378-386: gwc (8 groups) -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier -> softmax + regression."""
        return _cost_volume(self, match_left, match_right, features_left, self.args.max_disp)

    def _loop(self):
        return IGEVDiffusionLoop(self.time_embedding, self.update_block, self.upsample_disp,
                                 n_gru_layers=self.args.n_gru_layers, slow_fast_gru=self.args.slow_fast_gru,
                                 sampling_timesteps=self.sampling_timesteps, ensemble_cof=self.ensemble_cof,
                                 mixed_precision=bool(getattr(self.args, "mixed_precision", False)))

    @torch.no_grad()
    def model_predictions(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, noise, t, stem_2x):
        self.refresh_plans()
        return self._loop().model_predictions(coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, noise,
                                              t, stem_2x)

    @torch.no_grad()
    def ddim_sample(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, used, asd, stem_2x,
                    noise=None, generator=None):
        self.refresh_plans()
        return self._loop().ddim_sample(coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, used, asd,
                                        stem_2x, noise=noise, generator=generator)

    @torch.no_grad()
    def encode_disparity(self, flow_gt):
        """:405-419: two-hot x_0 of the quarter-resolution origin disparity, clamped to [0, 47]."""
        dq = torch.clamp(_dev_f32(flow_gt, "flow_gt"), 0, 47).contiguous()
        return ddim.encode_two_hot(dq, 48)

    def _front(self, image1, image2):
        """:364-400 up to the GRU inputs: feature pyramid + stems, matching features, cost volume + initial disparity,
        context encoder, geometry lookup object.  Shared with the origin network (igev_stereo.py:151-194)."""
        features_left, stem_2x, match_left, match_right, net_list, inp_list = _front2d(HIP, self, image1, image2,
                                                                                        self.args.n_gru_layers)
        geo, init_disp = self.cost_volume(match_left, match_right, features_left)
        from .geometry_ddim import Combined_Geo_Encoding_Volume
        geo_fn = Combined_Geo_Encoding_Volume(match_left, match_right, geo, radius=self.args.corr_radius,
                                              num_levels=self.args.corr_levels)
        return features_left, stem_2x, init_disp, net_list, inp_list, geo_fn

    def q_sample(self, x_start, t, noise=None):
        """:213-218 with ``t`` of shape [1] (one draw for the batch, :430)."""
        if noise is None:
            noise = torch.randn_like(x_start)
        return self.sqrt_alphas_cumprod[t].reshape(-1, 1, 1, 1) * x_start + \
            self.sqrt_one_minus_alphas_cumprod[t].reshape(-1, 1, 1, 1) * noise

    def forward_train(self, image1, image2, flow_full, flow_gt, iters=12, flow_init=None, test_mode=False, *, t=None,
                      noise=None, amp=False):
        """The reference's train branch (:364-463) -> ``(init_disp [B,1,H,W], disp_preds: iters x [B,1,H,W])``, what
        train_stereo.py:160-163 feeds to ``sequence_loss``; ``disp_up`` of the last iteration under ``test_mode``.  Every
        stage runs on its differentiable HIP route: the 2-D front (``_front2d`` on TRAIN), the cost volume, the spx heads, the
        geometry lookup, the update block and the convex upsampling.  ``flow_gt``: the quarter-resolution origin disparity
        [B,1,h,w] that is two-hot encoded and diffused (:405-432); ``flow_full`` is unused, as in the reference's train
        branch.  ``t`` ([1], long) / ``noise`` ([B,48,h,w]): the diffusion step and the q_sample noise, by default the
        reference's draws ``torch.randint(0, 1000, (1,))`` and ``randn_like``.  The noisy volume is detached like :436, so
        `time_embedding` gets no gradient, as in the reference.

        ``amp=True`` is the reference's ``--mixed_precision`` training (train_stereo.py:146-173 with
        ``autocast(enabled=args.mixed_precision)`` around every update-block call, :444-449): the update block runs at
        train precision "f16" for this call (``BasicMultiUpdateBlock.set_train_precision``; restored afterwards, also when
        the call raises) -- the boundary ``mixed_precision=True`` has in inference.  The front, the cost volume, the
        lookup and the upsampling head stay float32 (a deliberate difference: the reference autocasts them too), and all
        outputs are float32.  Step through ``torch.amp.GradScaler``: a scaled loss that overflows fp16 inside the block
        gives Inf / NaN gradients and the scaler skips the step.  The call takes no ``torch.autocast`` of the caller's
        and ``args.mixed_precision=True`` alone does not select it: both raise and point here.

        ``amp`` takes ``False``, ``True``, ``torch.float16`` (the same as ``True``) and ``torch.bfloat16``; anything else
        raises ValueError.  ``amp=torch.bfloat16``: the update block runs at train precision "bf16" for the call (restored
        afterwards, also when the call raises) on the bf16 kernels; the hidden states and context terms the front hands it
        are rounded to bfloat16, values and gradients (``round_gru_inputs_bf16``).  Everything else stays float32.  The range
        is float32's: step with the plain optimizer, no ``GradScaler``."""
        if not (amp is False or amp is True or amp is torch.float16 or amp is torch.bfloat16):
            raise ValueError(f"forward_train: amp must be False, True, torch.float16 or torch.bfloat16, got {amp!r}")
        if not self.training:
            raise _lib.DiffuVolumeError("forward_train is the training entry (model.train()); forward is the eval one")
        if not torch.is_grad_enabled():
            raise _lib.DiffuVolumeError("forward_train under no_grad: validation runs model.eval() and forward")
        if torch.is_autocast_enabled("cuda") or (getattr(self.args, "mixed_precision", False) and not amp):
            raise _lib.DiffuVolumeError("IGEVStereo_ddim.forward_train takes no args.mixed_precision / torch.autocast of "
                                        "the caller's: mixed-precision training is forward_train(..., amp=True) (the "
                                        "update block on the fp16 kernels, everything else float32) with "
                                        "torch.amp.GradScaler")
        if amp:
            before = self.update_block.train_precision
            self.update_block.set_train_precision(torch.bfloat16 if amp is torch.bfloat16 else "f16")
            try:
                return self._forward_train(image1, image2, flow_gt, iters, flow_init, test_mode, t, noise)
            finally:
                self.update_block.set_train_precision({"bf16": torch.bfloat16}.get(before, before))
        return self._forward_train(image1, image2, flow_gt, iters, flow_init, test_mode, t, noise)

    def _forward_train(self, image1, image2, flow_gt, iters, flow_init, test_mode, t, noise):
        if flow_init is not None:
            raise _lib.DiffuVolumeError("flow_init: the reference's train branch does not read it (:441-457)")
        _require_cuda(("image1", image1), ("image2", image2), ("flow_gt", flow_gt))
        n_layers = self.args.n_gru_layers
        features_left, stem_2x, match_left, match_right, net_list, inp_list = _front2d(TRAIN, self, image1, image2, n_layers)
        if self.update_block.train_precision == "f16":
            # as the inference loop under mixed_precision: the reference's front hands the block fp16 tensors (their
            # gradients pass through the same cast: rounded to fp16, Inf beyond its range -- what GradScaler watches)
            net_list, inp_list = round_gru_inputs_f16(net_list, inp_list)
        elif self.update_block.train_precision == "bf16":
            net_list, inp_list = round_gru_inputs_bf16(net_list, inp_list)      # (the same boundary at bf16; no scaler)
        geo, init_disp = self.cost_volume(match_left, match_right, features_left)
        spx_pred = None if test_mode else _spx_init_train(self, features_left[0], stem_2x)
        from .geometry_ddim import Combined_Geo_Encoding_Volume
        geo_fn = Combined_Geo_Encoding_Volume(match_left, match_right, geo, radius=self.args.corr_radius,
                                              num_levels=self.args.corr_levels)
        b, _, h, w = match_left.shape
        dev = match_left.device
        with torch.no_grad():                                                           # :402-436
            coords = torch.arange(w, dtype=torch.float32, device=dev).reshape(1, 1, 1, w).repeat(b, 1, h, 1)
            x0 = self.encode_disparity(flow_gt)
            if tuple(x0.shape) != (b, 48, h, w):
                raise RuntimeError(f"flow_gt must be the quarter-resolution disparity [B,1,{h},{w}], got {tuple(flow_gt.shape)}")
            t = torch.randint(0, self.num_timesteps, (1,), device=dev).long() if t is None else t.to(dev).long().reshape(1)
            noisy = self.q_sample(x0, t, None if noise is None else noise.to(device=dev, dtype=torch.float32))
            noisy = self.time_embedding(noisy, t)
            noisy = noisy + t.reshape(1, 1, 1, 1) / self.num_timesteps
            noisy = torch.clamp(noisy, min=-1 * self.scale, max=self.scale)
            noisy = (((noisy / self.scale) + 1) / 2.).float().contiguous()
        disp, disp_preds, disp_up = init_disp, [], None
        for itr in range(iters):                                                        # :441-457
            disp = disp.detach()
            geo_feat = geo_fn(disp, coords, noisy)
            if n_layers == 3 and self.args.slow_fast_gru:
                net_list = self.update_block(net_list, inp_list, iter16=True, iter08=False, iter04=False, update=False)
            if n_layers >= 2 and self.args.slow_fast_gru:
                net_list = self.update_block(net_list, inp_list, iter16=n_layers == 3, iter08=True, iter04=False, update=False)
            net_list, mask_feat_4, delta_disp = self.update_block(net_list, inp_list, geo_feat, disp, iter16=n_layers == 3,
                                                                  iter08=n_layers >= 2)
            disp = disp + delta_disp
            if test_mode and itr < iters - 1:
                continue
            disp_up = self.upsample_disp(disp, mask_feat_4, stem_2x)
            disp_preds.append(disp_up)
        if test_mode:
            return disp_up
        return context_upsample(init_disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1), disp_preds       # :462

    def forward(self, image1, image2, flow_full, flow_gt, iters=12, flow_init=None, test_mode=False, noise=None):
        if self.training:
            raise NotImplementedError("the MI355X DiffuVolume path is inference-only (model.eval())")
        self.refresh_plans()
        with torch.no_grad():
            _, stem_2x, init_disp, net_list, inp_list, geo_fn = self._front(image1, image2)
            x0 = self.encode_disparity(flow_gt)
            pred = self.ddim_sample(init_disp, init_disp, flow_init, iters, net_list, inp_list, geo_fn, flow_full, x0,
                                    stem_2x, noise=noise)
        return pred, pred
