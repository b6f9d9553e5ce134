"""ACVNet + DiffuVolume (SceneFlow flavour) behind the reference's module API.

Drop-in for ``ACVNet_DDIM`` of SceneFlow/models/acv_ddim.py:122-482 (eval path):
same constructor, same ``forward(left, right, used, disp, mask_gt=None) -> [pred]``,
``model_predictions`` and ``ddim_sample``; same submodule / parameter / buffer names, so a
reference ``state_dict`` (579 keys, float64 schedule buffers) loads with ``strict=True``.

What runs where
  * cost volumes, the per-step volume filter, both 3-D hourglasses, the regression tail
    and the DDIM state update: HIP kernels of libdiffuvolume_hip.so (``submodule.py``);
  * the 2-D feature CNN, ``concatconv`` and the depthwise ``patch`` convolutions: plain
    PyTorch (MIOpen) -- outside the hot path named by the north star;
  * the 56 k-parameter time MLP: PyTorch, once per step.
The dead pre-DDIM aggregation pass of the reference's eval branch (acv_ddim.py:392-401,
its result ``pred2`` is never returned) is skipped; outputs are unchanged.
Training (``model.train()``, the reference's :424-482 branch): ``forward`` returns
``[pred_attention, pred0, pred1, pred2]`` with the 3-D convolutions on the differentiable HIP route of
``train3d.py``, the patch stencils on ``train_patch.py``, the hourglasses' window attention on ``train_attn.py``, the
feature CNN and ``concatconv`` on the nn.Modules or -- with ``DV_TRAIN_NET2D=hip`` -- on ``train_net2d.py``, and
everything else on PyTorch autograd; on CPU tensors it raises.
The containers (convbn, BasicBlock, the hourglass), their prepared plans and the walk that runs a Sequential in training
are ``net_blocks.py``'s, shared with the PCW flavour; the training filter is ``ddim.train_filter``.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from . import ddim
from . import net_blocks
from . import train3d
from .train_tail import regress_head
from . import train_volume
from .train_volume import build_concat_volume_train
from .train_patch import patch_volume_train
from .train_attn import window_attention_train
from . import train_net2d
from .head import DynamicHead
from .net_blocks import (BasicBlockPlan, HourglassPlan, PairPlan, WindowAttention, cb2, cb3, plan_cb2, plan_seq2d,
                         init_weights, run_plans, stack, walk)
from .submodule import (ACT_NONE, ACT_RELU, Conv2dPlan, PlanCache, Rank1FilterPlan,
                        _dev_f32,
                        AttentionConcatVolume, build_concat_attention_volume, build_concat_volume, build_gwc_volume,
                        check_split_overflow, default_conv_precision, patch_volume, upsample_softmax_regress)


PATCH_DILATION = (1,) * 8 + (2,) * 16 + (3,) * 16      # patch_l1 / patch_l2 / patch_l3 on groups 0-7 / 8-23 / 24-39


def any_split_plan(plans) -> bool:
    """True if the prepared layers include a split-fp16 convolution (its range guard must be read)."""
    return plans is not None and getattr(plans.dres0.b, "split", False)


# the ReLU flavour of net_blocks' containers and plans, under the names tests, tools and oracle/ import
_cb3 = cb3
_WindowAttention = WindowAttention


def _train_window_attention(ab: WindowAttention, x: torch.Tensor) -> torch.Tensor:
    """attention_block.forward (SceneFlow/models/submodule.py:398-429) in training on the route of `train_attn`
    (DV_TRAIN_ATTN: the fused HIP forward and backward, or the PyTorch statement)."""
    return window_attention_train(x, ab.qkv_3d.weight, ab.qkv_3d.bias, ab.final1x1.weight, ab.final1x1.bias, ab.num_heads)


class Hourglass(net_blocks.Hourglass):
    """3-D encoder/decoder with skip convs and bottleneck window attention (acv_ddim.py:56-93)."""

    def __init__(self, c: int):
        super().__init__(c, "relu", heads=16, attention=_train_window_attention)


_HourglassPlan = HourglassPlan


class FeatureExtraction(PlanCache, nn.Module):
    """2-D feature CNN (acv_ddim.py:14-53): 320-channel 1/4-resolution ``gwc_feature``.  On the GPU (eval) all 55
    convolutions run on the 2-D implicit-GEMM kernel with BN / ReLU / the residual add fused (csrc/conv2d.hip)."""

    def __init__(self):
        super().__init__()
        self.firstconv = nn.Sequential(cb2(3, 32, 3, 2, 1, 1), nn.ReLU(inplace=True),
                                       cb2(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                       cb2(32, 32, 3, 1, 1, 1), nn.ReLU(inplace=True))
        self.layer1 = stack(32, 32, 3, 1, 1, 1, "relu")
        self.layer2 = stack(32, 64, 16, 2, 1, 1, "relu")
        self.layer3 = stack(64, 128, 3, 1, 1, 1, "relu")
        self.layer4 = stack(128, 128, 3, 1, 1, 2, "relu")

    def _build_plans(self, slot):
        if slot == train_net2d.SLOT:
            return train_net2d.build_plans(self)
        with torch.no_grad():
            p = {"firstconv": plan_seq2d(self.firstconv)}
            for n in ("layer1", "layer2", "layer3", "layer4"):
                p[n] = [BasicBlockPlan(b, down_first=False) for b in getattr(self, n)]
        return p

    def _graph(self, x, stack, head):
        """The network, once for its three routes: ``stack(name, x)`` runs a layer of BasicBlocks, ``head(name, x)`` a
        plain Sequential."""
        x = stack("layer1", head("firstconv", x))
        l2 = stack("layer2", x)
        l3 = stack("layer3", l2)
        l4 = stack("layer4", l3)
        return {"gwc_feature": torch.cat((l2, l3, l4), dim=1)}

    def forward(self, x):
        if not x.is_cuda:
            raise _lib.DiffuVolumeError(f"input is on {x.device}: the feature CNN runs on the MI355X (no CPU fallback)")
        if self.training and train_net2d.route() == "hip":
            # training on the HIP route: convolutions on train2d's kernels, BatchNorm2d + ReLU + skip on train_norm's
            n = train_net2d.Net2d(self)
            return self._graph(x, lambda k, t: n.stack(getattr(self, k), t), lambda k, t: n.seq(getattr(self, k), t))
        if self.training or (torch.is_grad_enabled() and x.requires_grad):
            module = lambda k, t: getattr(self, k)(t)       # training / autograd: the plain PyTorch modules, on the GPU
            return self._graph(x, module, module)
        p = self.prepare(check_weights=True)
        plan = lambda k, t: run_plans(p[k], t)
        with torch.no_grad():
            return self._graph(x, plan, plan)


# A/B switch for tools/ and tests: False keeps the first layer of a DDIM step on the generic filtered convolution
RANK1_FILTER = True


class _Plans:
    def __init__(self, m: "ACVNet_DDIM"):
        self.dres0 = PairPlan(m.dres0)
        # dres0[0] on the factors of a filtered attention-concat volume (acv_ddim.py:260, :388-390); exact-fp32 paths only
        conv0, bn0 = m.dres0[0][0], m.dres0[0][1]
        self.dres0_rank1 = None
        if default_conv_precision() in ("f32", "f32_direct") and RANK1_FILTER:
            self.dres0_rank1 = Rank1FilterPlan(conv0.weight, (bn0.weight, bn0.bias, bn0.running_mean, bn0.running_var),
                                               act=ACT_RELU, eps=bn0.eps)
        self.dres1 = PairPlan(m.dres1)
        self.dres2 = _HourglassPlan(m.dres2)
        self.dres3 = _HourglassPlan(m.dres3)
        self.classif2 = PairPlan(m.classif2)
        self.dres1_att = PairPlan(m.dres1_att_)
        self.dres2_att = _HourglassPlan(m.dres2_att_)
        self.classif_att = PairPlan(m.classif_att_)
        # attention branch front: the two depth-wise (1,3,3) stencils fuse into one pass; concatconv on the 2-D kernel
        self.patch_w1 = m.patch.weight.detach().float().reshape(40, 9).contiguous()
        self.patch_w2 = torch.cat([p.weight.detach().float().reshape(-1, 9) for p in (m.patch_l1, m.patch_l2, m.patch_l3)]).contiguous()
        self.patch_dil = torch.tensor([1] * 8 + [2] * 16 + [3] * 16, dtype=torch.int32, device=self.patch_w1.device)
        self.concat_a = plan_cb2(m.concatconv[0], ACT_RELU)
        self.concat_b = Conv2dPlan(m.concatconv[2].weight, None, act=ACT_NONE)
        # the origin ACVNet has no diffusion schedule
        self.ddim = ddim.Tables(m.alphas_cumprod) if hasattr(m, "alphas_cumprod") else None


def _volume_arg(volume):
    """The `volume` argument of the reference API: a float32 device tensor, or the factor handle standing in for it."""
    return volume if isinstance(volume, AttentionConcatVolume) else _dev_f32(volume, "volume")


def _volume_tensor(volume) -> torch.Tensor:
    return volume.tensor() if isinstance(volume, AttentionConcatVolume) else volume


class ProbVolumeHandle:
    """Stand-in for ``pred_volume2`` ([B,192,H,W], 377 MB per pair in the reference): keeps the
    quarter-resolution cost and the fused uncertainty; ``dense()`` materialises the softmax
    volume with PyTorch ops for callers that really want it."""

    def __init__(self, cost: torch.Tensor, uncertainty: torch.Tensor, maxdisp: int, align_corners: bool = False):
        self.cost, self.uncertainty, self.maxdisp, self.align_corners = cost, uncertainty, maxdisp, align_corners

    def dense(self) -> torch.Tensor:
        b, _, d, h, w = self.cost.shape
        up = F.interpolate(self.cost, [self.maxdisp, h * 4, w * 4], mode="trilinear",
                           align_corners=True if self.align_corners else None)
        return F.softmax(up.squeeze(1), dim=1)


class _HipPlanMixin(PlanCache, nn.Module):
    """The plans of the ACV wrappers (submodule.PlanCache: rebuilt when the weights change)."""

    def _build_plans(self, slot) -> _Plans:
        if slot == train_net2d.SLOT:
            return train_net2d.build_plans(self, ("concatconv.",))
        dev = self.dres0[0][0].weight.device
        if dev.type != "cuda":
            raise _lib.DiffuVolumeError("the ACVNet hot path needs the model on the MI355X (model.cuda()); no CPU fallback")
        with torch.no_grad(), torch.cuda.device(dev):
            return _Plans(self)

    def _init_backbone(self, time_embedding: bool):
        """Sub-modules under the reference's attribute names, in its construction order (acv_ddim.py:174-222,
        acv.py:103-150), and its weight initialisation (:224-238)."""
        def pair(cin):
            return nn.Sequential(cb3(cin, 32, 3, 1, 1), nn.ReLU(inplace=True), cb3(32, 32, 3, 1, 1))

        def classifier():
            return nn.Sequential(cb3(32, 32, 3, 1, 1), nn.ReLU(inplace=True), nn.Conv3d(32, 1, 3, 1, 1, bias=False))
        self.feature_extraction = FeatureExtraction()
        self.concatconv = nn.Sequential(cb2(320, 128, 3, 1, 1, 1), nn.ReLU(inplace=True),
                                        nn.Conv2d(128, self.concat_channels, 1, bias=False))
        self.patch = nn.Conv3d(40, 40, (1, 3, 3), 1, (0, 1, 1), 1, groups=40, bias=False)
        self.patch_l1 = nn.Conv3d(8, 8, (1, 3, 3), 1, (0, 1, 1), 1, groups=8, bias=False)
        self.patch_l2 = nn.Conv3d(16, 16, (1, 3, 3), 1, (0, 2, 2), 2, groups=16, bias=False)
        self.patch_l3 = nn.Conv3d(16, 16, (1, 3, 3), 1, (0, 3, 3), 3, groups=16, bias=False)
        self.dres1_att_ = pair(40)
        self.dres2_att_ = Hourglass(32)
        self.classif_att_ = classifier()
        if time_embedding:
            self.time_embedding = DynamicHead(d_model=48)
        self.dres0 = nn.Sequential(cb3(64, 32, 3, 1, 1), nn.ReLU(inplace=True),
                                   cb3(32, 32, 3, 1, 1), nn.ReLU(inplace=True))
        self.dres1 = pair(32)
        self.dres2 = Hourglass(32)
        self.dres3 = Hourglass(32)
        self.classif0, self.classif1, self.classif2 = classifier(), classifier(), classifier()
        init_weights(self)


class ACVNet_DDIM(train3d.TrainPrecision, _HipPlanMixin):
    def __init__(self, maxdisp: int, attn_weights_only: bool = False, freeze_attn_weights: bool = False,
                 sampling_timesteps: int = 5, ensemble_cof: Optional[Sequence[float]] = None):
        super().__init__()
        if maxdisp != 192:
            # the reference hard-codes 48 / 192 (acv_ddim.py:278,:302,:325)
            raise ValueError("ACVNet_DDIM is defined for maxdisp == 192")
        self.maxdisp = maxdisp
        self.attn_weights_only = attn_weights_only
        self.freeze_attn_weights = freeze_attn_weights
        self.num_groups = 40
        self.concat_channels = 32
        self.scale = 1.0
        self.num_timesteps = 1000
        self.sampling_timesteps = sampling_timesteps
        self.ddim_sampling_eta = 1.0
        self.renewal = True
        self.use_ensemble = True
        # ensemble over [used, disp_1 .. disp_S] (acv_ddim.py:367)
        if ensemble_cof is None:
            if sampling_timesteps != 5:
                raise ValueError("give ensemble_cof (S+1 weights) when sampling_timesteps != 5")
            ensemble_cof = (0.5, 0.0, 0.0, 0.0, 0.2, 0.3)
        if len(ensemble_cof) != sampling_timesteps + 1:
            raise ValueError("ensemble_cof needs sampling_timesteps + 1 entries")
        self.ensemble_cof = tuple(float(c) for c in ensemble_cof)
        self.dif_threshold, self.unc_threshold = 1.0, 3.0

        ddim.register_schedule(self, self.num_timesteps)

        self._init_backbone(time_embedding=True)

    # ---- pieces of the hot path ----------------------------------------------------------
    def _time_pairs(self):
        return ddim.time_pairs(self.num_timesteps, self.sampling_timesteps)

    def _filter(self, x_t: torch.Tensor, t: Optional[torch.Tensor], shift: Optional[torch.Tensor] = None):
        return ddim.noise_prepare(self.time_embedding, x_t, t, shift)

    def _aggregate(self, volume: torch.Tensor, n01f: Optional[torch.Tensor]) -> torch.Tensor:
        """acv_ddim.py:260-266: (volume * filter) -> dres0 -> dres1(+res) -> dres2 -> dres3 -> classif2."""
        p = self.prepare()
        r1 = getattr(p, "dres0_rank1", None)
        if r1 is not None and r1.applies(volume):
            cost0 = p.dres0.second(r1(volume, n01f))            # first layer on the volume's factors (Rank1FilterPlan)
        else:                                                   # any other tensor; a factor handle is materialised once
            cost0 = p.dres0(_volume_tensor(volume), in_scale=n01f)
        cost0 = p.dres1(cost0, residual_self=True)
        out2 = p.dres3(p.dres2(cost0))
        return p.classif2(out2)

    def _step_coef(self, time: int, time_next: int, cof: float) -> _lib.DvDdimCoef:
        return ddim.step_coef(self.prepare().ddim, time, time_next, cof, eta=self.ddim_sampling_eta,
                              dif_thr=self.dif_threshold, unc_thr=self.unc_threshold,
                              clamp_max=float(self.maxdisp - 1), ens_dif_thr=0.0)

    def _loop_plan(self):
        return ddim.loop_plan(self, self.prepare().ddim, self.dres0[0][0].weight.device)

    # ---- reference API ---------------------------------------------------------------------
    @torch.no_grad()
    def model_predictions(self, volume: torch.Tensor, noise: torch.Tensor, t: torch.Tensor):
        """acv_ddim.py:254-296 -> (pred_noise fp64, x_start fp32, pred [B,H,W], ProbVolumeHandle)."""
        volume = _volume_arg(volume)
        b, _, d, h, w = volume.shape
        self.prepare(check_weights=True)
        with torch.cuda.device(volume.device):
            n01, n01f = self._filter(noise, t)
            cost = self._aggregate(volume, n01f)
            pred, unc = upsample_softmax_regress(cost, want_uncertainty=True)
            time = int(t.reshape(-1)[0])
            coef = self._step_coef(time, -1, 0.0)
            mask = torch.zeros((b, h, w), dtype=torch.float32, device=volume.device)
            x_start, _, pred_noise = ddim.ddim_update(pred, pred, n01, None, None, mask, None, coef, unc=unc,
                                                      want_pred_noise=True)
        return pred_noise, x_start, pred, ProbVolumeHandle(cost, unc, self.maxdisp)

    @torch.no_grad()
    def ddim_step(self, i: int, volume: torch.Tensor, used: torch.Tensor, img: torch.Tensor, mask: torch.Tensor,
                  ens: Optional[torch.Tensor] = None, eps: Optional[torch.Tensor] = None,
                  fill: Optional[torch.Tensor] = None, out_disp: Optional[torch.Tensor] = None):
        """Iteration ``i`` of the loop of acv_ddim.py:313-362 from explicit state: ``img`` is the DDIM state entering
        the step (fp32 for i == 0, fp64 later), ``mask`` [B,h,w] the accumulated renewal mask (updated in place),
        ``ens`` the ensemble accumulator (updated in place when given), ``eps`` / ``fill`` this step's
        ``randn_like(img)`` / ``rand_like`` draws (not needed on the last step).
        Returns (disp [B,4h,4w], uncertainty, x_start fp32, x_next fp64 | None)."""
        st = self._loop_plan()[i]
        b = volume.shape[0]
        n01, n01f = self._filter(img, None, st.shift_rows(b))
        cost = self._aggregate(volume, n01f)
        disp, unc = upsample_softmax_regress(cost, want_uncertainty=True, out_disp=out_disp)
        x_start, x_next, _ = ddim.ddim_update(disp, used, n01, eps, fill, mask, ens, st.coef, unc=unc)
        return disp, unc, x_start, x_next

    @torch.no_grad()
    def ddim_sample(self, volume: torch.Tensor, used: torch.Tensor, asd: torch.Tensor,
                    noise: Optional[ddim.NoiseFn] = None, generator: Optional[torch.Generator] = None,
                    trace: Optional[Callable[[int, dict], None]] = None):
        """acv_ddim.py:298-370.  ``noise(kind, shape, dtype)`` (kind 'eps' = randn_like(img) :354,
        'fill' = rand_like :360) injects the random draws for parity tests; by default they come
        from the device generator.  ``trace(i, state)`` (tests) receives every step's tensors.
        Returns (final_prediction [B,H,W], stack [S+1,B,H,W])."""
        volume = _volume_arg(volume)
        used = ddim.check_loop_args(volume, _dev_f32(used, "used"), asd, self.maxdisp)
        b, _, d, h, w = volume.shape
        dev = volume.device
        self.prepare(check_weights=True)
        draw = ddim.make_draw(noise, generator, dev)

        with torch.cuda.device(dev):
            steps = self._loop_plan()
            img = asd.to(dev).contiguous()
            stack = torch.empty((len(steps) + 1, b, 4 * h, 4 * w), dtype=torch.float32, device=dev)
            stack[0].copy_(used)
            mask = torch.zeros((b, h, w), dtype=torch.float32, device=dev)
            ens = used * self.ensemble_cof[0]
            for i, st in enumerate(steps):
                eps = fill = None
                if st.time_next >= 0:
                    eps = draw("eps", tuple(img.shape), img.dtype)
                    fill = draw("fill", tuple(img.shape), torch.float64)
                if trace is not None:
                    trace(i, {"when": "in", "img": img, "mask": mask.clone(), "eps": eps, "fill": fill})
                disp, unc, x_start, x_next = self.ddim_step(i, volume, used, img, mask, ens, eps, fill,
                                                            out_disp=stack[i + 1])
                if trace is not None:
                    trace(i, {"when": "out", "disp": disp, "unc": unc, "x_start": x_start, "x_next": x_next,
                              "mask": mask.clone()})
                img = x_start if st.time_next < 0 else x_next
        if any_split_plan(self._plans):
            check_split_overflow(dev)
        if self.use_ensemble:
            return ens, stack
        return stack[-1]

    @torch.no_grad()
    def encode_disparity(self, disp: torch.Tensor, mask_gt: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x_T of acv_ddim.py:403-419: quarter-resolution disparity [B,1,h,w] -> [B,48,h,w] in [-1,1].  `mask_gt` (None
        at every call site of the reference; anything that broadcasts against [B,48,h,w]) puts the uniform distribution
        1/48 where it is 0 (:415-417)."""
        disp = _dev_f32(disp, "disp")
        nb = self.maxdisp // 4
        x = ddim.encode_two_hot(disp, nb)
        if mask_gt is not None:
            # the reference selects before the *2-1 rescale; the same fp32 operations on the one constant it selects
            uniform = ((torch.ones((), dtype=torch.float32, device=x.device) / nb) * 2 - 1) * self.scale
            x = torch.where(mask_gt.to(x.device) == 0, uniform, x)
        return x

    @torch.no_grad()
    def attention_logits(self, feat_left: torch.Tensor, feat_right: torch.Tensor) -> torch.Tensor:
        """acv_ddim.py:375-384 (= acv.py:171-197): gwc volume -> patch convs -> attention aggregation -> `att_weights`
        [B,1,D/4,H/4,W/4]."""
        p = self.prepare()
        gwc = build_gwc_volume(feat_left, feat_right, self.maxdisp // 4, self.num_groups)
        att = p.dres1_att(patch_volume(gwc, p.patch_w1, p.patch_w2, p.patch_dil))     # patch, patch_l1..3 (:377-381)
        return p.classif_att(p.dres2_att(att))

    @torch.no_grad()
    def attention_concat_volume(self, feat_left: torch.Tensor, feat_right: torch.Tensor, lazy: bool = False):
        """acv_ddim.py:375-390: gwc volume -> patch convs -> attention aggregation -> logits, then the
        softmax-weighted concat volume (the tensor the DDIM loop filters), [B,64,D/4,H/4,W/4] like the reference's :390.
        ``lazy=True`` (what ``forward`` passes) returns its factors instead (``AttentionConcatVolume``: the first
        aggregation layer reads nothing else, so the 3 GB tensor is not written) -- same default as
        ``build_concat_attention_volume``, so a caller who indexes / clones the result gets a tensor."""
        p = self.prepare()
        att = self.attention_logits(feat_left, feat_right)
        cl = p.concat_b(p.concat_a(feat_left))
        cr = p.concat_b(p.concat_a(feat_right))
        return build_concat_attention_volume(cl, cr, att, self.maxdisp // 4, lazy=lazy)

    def train_forward(self, left, right, disp, mask_gt=None):
        """The reference's training branch (acv_ddim.py:372-399, :424-482) -> [pred_attention, pred0, pred1, pred2].
        Draws ``t = torch.randint(0, T, (1,))`` and then q_sample's ``torch.randn_like`` (in that order).
        Runs at ``self.train_precision`` ("f32", "f16" or "bf16"; ``set_train_precision``, which takes ``torch.bfloat16``
        for the last): every ``train3d`` call below, the no-grad statistics
        pass and the hourglasses' helpers included, sees it for the length of this call, on this thread only."""
        with self._train_scope():
            return self._train_forward(left, right, disp, mask_gt)

    def _train_forward(self, left, right, disp, mask_gt=None):
        if not left.is_cuda:
            raise NotImplementedError("training runs on the MI355X only (model.cuda()); no CPU path")
        fl = self.feature_extraction(left)["gwc_feature"]
        fr = self.feature_extraction(right)["gwc_feature"]
        gwc = build_gwc_volume(fl, fr, self.maxdisp // 4, self.num_groups)
        # :377-381 on the route of train_patch (DV_TRAIN_PATCH: one fused pass forward and one backward, or the nn.Conv3d
        # statement); autograd splits the gradient onto the four weights
        patch = patch_volume_train(gwc, self.patch.weight.reshape(40, 9),
                                   torch.cat([m.weight.reshape(-1, 9) for m in (self.patch_l1, self.patch_l2, self.patch_l3)]),
                                   PATCH_DILATION)
        cost_attention = walk(self.dres1_att_, patch)
        cost_attention = self.dres2_att_(cost_attention)
        att_weights = walk(self.classif_att_, cost_attention)

        if train_net2d.route() == "hip":
            n2d = train_net2d.Net2d(self, ("concatconv.",))
            cl, cr = n2d.seq(self.concatconv, fl), n2d.seq(self.concatconv, fr)
        else:
            cl = self.concatconv(fl)
            cr = self.concatconv(fr)
        # :388-390 `F.softmax(att_weights, dim=2) * concat_volume`, and :451 `* noisy` below, as factors: the softmax on
        # the [B,1,D,h,w] logits, both products on the [B,D,h,w] scale of build_concat_volume_train.  (p * n) * v instead
        # of the reference's (p * v) * n: at most one rounding per element, the order of the eval path
        # DV_TRAIN_VOLUME=torch: the statements as the reference orders them, on the [B,64,D,h,w] tensors
        factored = train_volume.route() == "hip"
        p_att = F.softmax(att_weights, dim=2)
        if not factored:
            ac_volume = p_att * build_concat_volume(cl, cr, self.maxdisp // 4)

        # :384-398 run the aggregation stack once on the un-filtered volume in training mode too; its prediction is
        # overwritten, but the BatchNorm layers of dres0..dres3 / classif2 update their running statistics on it
        with torch.no_grad():
            if factored:
                ac_volume = build_concat_volume_train(cl.detach(), cr.detach(), self.maxdisp // 4,
                                                      scale=p_att.detach()[:, 0])
            cost0 = walk(self.dres0, ac_volume)
            cost0 = walk(self.dres1, cost0) + cost0
            walk(self.classif2, self.dres3(self.dres2(cost0)))
            del cost0
            if factored:
                del ac_volume

        # two-hot x_start (:426-439), the mask_gt form of the training branch
        x_start = self.encode_disparity(disp.detach().float())
        if mask_gt is not None:
            uniform = ((torch.ones((), dtype=torch.float32, device=x_start.device) / (self.maxdisp // 4)) * 2 - 1) * self.scale
            x_start = torch.where(mask_gt.to(x_start.device).unsqueeze(1) == 0, uniform, x_start.unsqueeze(1)).squeeze(1)
        noisy = ddim.train_filter(self.sqrt_alphas_cumprod, self.sqrt_one_minus_alphas_cumprod, self.time_embedding,
                                  self.scale, self.num_timesteps, x_start)

        if factored:
            ac_volume = build_concat_volume_train(cl, cr, self.maxdisp // 4, scale=(p_att * noisy)[:, 0])
        else:
            ac_volume = ac_volume * noisy
        cost0 = walk(self.dres0, ac_volume)
        cost0 = walk(self.dres1, cost0) + cost0
        out1 = self.dres2(cost0)
        out2 = self.dres3(out1)

        size = [self.maxdisp, left.size()[2], left.size()[3]]

        # the fused tail with its HIP backward (train_tail.py; DV_TRAIN_TAIL)
        pred_attention = regress_head(att_weights, size)
        pred0 = regress_head(walk(self.classif0, cost0), size)
        pred1 = regress_head(walk(self.classif1, out1), size)
        pred2 = regress_head(walk(self.classif2, out2), size)
        return [pred_attention, pred0, pred1, pred2]

    def forward(self, left, right, used, disp, mask_gt=None):
        if self.training:
            return self.train_forward(left, right, disp, mask_gt)
        with torch.no_grad():
            self.prepare(check_weights=True)
            fl = self.feature_extraction(left)["gwc_feature"]
            fr = self.feature_extraction(right)["gwc_feature"]
            ac_volume = self.attention_concat_volume(fl, fr, lazy=True)
            x_T = self.encode_disparity(disp, mask_gt)
            pred, _ = self.ddim_sample(ac_volume, used, x_T)
        return [pred]


class ACVNet(_HipPlanMixin):
    """The origin network that supplies ``used`` (SceneFlow/models/acv.py:94-260, eval path): same feature CNN, attention
    branch, concat volume and aggregation stack as ACVNet_DDIM, run on the same HIP kernels, without the diffusion loop.
    ``forward(left, right) -> [pred2]``, or ``[pred_attention]`` (the regression of the attention logits, acv.py:246-252)
    when built with ``attn_weights_only=True`` -- the reference builds every module either way, so the ``state_dict``
    (561 keys) is the same and loads with strict=True."""

    def __init__(self, maxdisp: int, attn_weights_only: bool = False, freeze_attn_weights: bool = False):
        super().__init__()
        if maxdisp != 192:
            raise ValueError("ACVNet on the HIP path: maxdisp == 192")
        self.maxdisp, self.attn_weights_only, self.freeze_attn_weights = maxdisp, attn_weights_only, freeze_attn_weights
        self.num_groups, self.concat_channels = 40, 32
        self._init_backbone(time_embedding=False)

    attention_logits = ACVNet_DDIM.attention_logits
    attention_concat_volume = ACVNet_DDIM.attention_concat_volume
    _aggregate = ACVNet_DDIM._aggregate

    def forward(self, left, right):
        if self.training:
            raise NotImplementedError("the MI355X path is inference-only (model.eval())")
        with torch.no_grad():
            self.prepare(check_weights=True)
            fl = self.feature_extraction(left)["gwc_feature"]
            fr = self.feature_extraction(right)["gwc_feature"]
            if self.attn_weights_only:                                           # acv.py:246-252
                cost = self.attention_logits(fl, fr)
            else:
                cost = self._aggregate(self.attention_concat_volume(fl, fr, lazy=True), None)
            pred2, _ = upsample_softmax_regress(cost, want_uncertainty=False)
            if any_split_plan(self._plans):
                check_split_overflow(pred2.device)
        return [pred2]


__models__ = {"acvnet": ACVNet, "acvnet_ddim": ACVNet_DDIM}
