"""IGEV-Stereo + DiffuVolume: the DDIM volume-filter loop (KITTI15/core/igev_stereo_ddim.py:226-359).

What is here: the pieces of ``IGEVStereo_ddim`` that are on the hot path -- the time embedding with its
180 -> 48 channel interpolation (core/head.py:74-83), ``model_predictions`` (noise filter -> `iters` GRU
iterations each looking the filtered geometry volume up -> two-hot re-encoding -> noise prediction) and
``ddim_sample`` (renewal mask dif<5, output rule dif<3, fresh q_sample fill, ensemble [0.6,0.1,0.3]).
The geometry lookup, the filter and the DDIM state update are HIP kernels; the ConvGRU update block and the
convex upsampling are 2-D PyTorch modules supplied by the caller (``update_block`` / ``upsample_disp``), exactly
as the reference method calls them.  The MobileNetV2 backbone (timm, pretrained) and the rest of the
``IGEVStereo_ddim`` constructor are out of scope, so this is a loop object rather than
the full nn.Module.  Batch handling: the reference head is batch-1 only; here the shift is
taken per sample.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, train2d, train3d
from .acv_ddim import cosine_beta_schedule
from .head import SinusoidalPositionEmbeddings
from .submodule import (ACT_LEAKY, ACT_NONE, ACT_RELU, Conv2dPlan, Conv3dPlan, Deconv2dK4S2Plan, Deconv3dPlan, PlanCache, _dev_f32, build_gwc_volume,
                        _gwc_volume_autograd, feature_gate, softmax_regress, weight_key)


class DynamicHead180(nn.Module):
    """KITTI15/core/head.py:51-83: DynamicHead(d_model=180) whose 180-channel shift is linearly
    interpolated to the 48 disparity bins before it is added."""

    def __init__(self, d_model: int = 180, bins: int = 48):
        super().__init__()
        self.d_model, self.bins = d_model, bins
        width = d_model * 4
        self.time_mlp = nn.Sequential(SinusoidalPositionEmbeddings(d_model), nn.Linear(d_model, width), nn.GELU(),
                                      nn.Linear(width, width))
        self.block_time_mlp = nn.Sequential(nn.SiLU(), nn.Linear(width, d_model))
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def shift(self, t: torch.Tensor) -> torch.Tensor:
        s = self.block_time_mlp(self.time_mlp(t))                                   # [B,180]
        return F.interpolate(s.unsqueeze(1), self.bins, mode="linear").squeeze(1)    # [B,48]

    def forward(self, noisy, t):
        return noisy + self.shift(t).unsqueeze(-1).unsqueeze(-1)


def round_gru_inputs_f16(net_list, inp_list):
    """The hidden states and the context terms cz / cr / cq rounded to fp16 values (kept as float32) when the GRU loop
    starts under `mixed_precision`: the reference's front produces them under autocast as fp16 tensors (`torch.tanh`,
    `torch.relu` and `context_zqr_convs`, igev_stereo_ddim.py:366-400) while this build's front stays float32 (it runs
    once per forward, and float32 is closer to the exact result).  Idempotent on fp16-exact values."""
    r = lambda t: t.half().float() if isinstance(t, torch.Tensor) else t
    return [r(t) for t in net_list], [[r(t) for t in trio] for trio in inp_list]


class IGEVDiffusionLoop:
    def __init__(self, time_embedding: DynamicHead180, update_block: Callable, upsample_disp: Callable,
                 n_gru_layers: int = 3, slow_fast_gru: bool = False, sampling_timesteps: int = 2,
                 ensemble_cof: Sequence[float] = (0.6, 0.1, 0.3), mixed_precision: bool = False):
        if len(ensemble_cof) != sampling_timesteps + 1:
            raise ValueError("ensemble_cof needs sampling_timesteps + 1 entries")
        self.time_embedding, self.update_block, self.upsample_disp = time_embedding, update_block, upsample_disp
        self.n_gru_layers, self.slow_fast_gru = n_gru_layers, slow_fast_gru
        self.mixed_precision = bool(mixed_precision)     # the update block under fp16 autocast (igev_stereo_ddim.py:242)
        self.num_timesteps, self.sampling_timesteps, self.eta = 1000, sampling_timesteps, 1.0
        self.ensemble_cof = tuple(float(c) for c in ensemble_cof)
        ac = torch.cumprod(1.0 - cosine_beta_schedule(1000), dim=0)
        self.alphas_cumprod = ac
        self.sqrt_ac, self.sqrt_1mac = torch.sqrt(ac), torch.sqrt(1.0 - ac)
        self.sqrt_recip, self.sqrt_recipm1 = torch.sqrt(1.0 / ac), torch.sqrt(1.0 / ac - 1)

    def _time_pairs(self):
        times = torch.linspace(-1, self.num_timesteps - 1, steps=self.sampling_timesteps + 1)
        times = list(reversed(times.int().tolist()))
        return list(zip(times[:-1], times[1:]))

    def _filter(self, x_t, t):
        b, c, h, w = x_t.shape
        shift = self.time_embedding.shift(t).float().contiguous()
        lib = _lib.load()
        x_t = x_t.contiguous()
        n01 = torch.empty_like(x_t)
        if x_t.dtype == torch.float32:
            _lib.check(lib.dv_noise_prepare_f32(x_t.data_ptr(), shift.data_ptr(), n01.data_ptr(), b, c, h * w,
                                                _lib.stream_ptr()), "dv_noise_prepare_f32")
            return n01, n01
        n01f = torch.empty(x_t.shape, dtype=torch.float32, device=x_t.device)
        _lib.check(lib.dv_noise_prepare_f64(x_t.data_ptr(), shift.data_ptr(), n01.data_ptr(), n01f.data_ptr(), b, c,
                                            h * w, _lib.stream_ptr()), "dv_noise_prepare_f64")
        return n01, n01f

    # ---- the GRU iterations of one DDIM step as a hipGraph -------------------------------------------------------
    # One step launches `iters` x ~30 small kernels (1/8- and 1/16-scale convolutions of 0.06-0.1 ms) from Python through
    # ctypes: the launch gaps are a measurable part of config 5 (20 steps x 32 iterations per pair).  Within ONE forward
    # everything a step reads besides its carried state is constant (features, context, geometry volume, stem), so the
    # first step of a forward is captured and the other steps replay it with (coords1, hidden states, filtered noise)
    # copied into the graph's static inputs.  The eager loop below is the same code the capture records; a new forward
    # (new corr_fn object) re-captures; one graph is kept.  MEASURED (round 5, 1248x384, batch 4, 20 x 32 iterations, same
    # box): eager 2 059.9 ms per forward, graph 2 082.0 ms -- the eager loop is already GPU-bound (the host runs ahead of
    # 0.06-0.1 ms kernels), a replay only adds the state copies and the capture.  OPT-IN: `use_graph` / DV_IGEV_GRAPH=1.
    use_graph = os.environ.get("DV_IGEV_GRAPH", "0") == "1"
    _graph = None
    _graph_warm = frozenset()           # the precision modes whose eager warm-up pass has run

    def _gru_iterations(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, n01f, stem_2x):
        ok = (self.use_graph and flow_init is None and coords1.is_cuda and not torch.cuda.is_current_stream_capturing()
              and all(isinstance(t, torch.Tensor) for t in net_list))
        if not ok:
            return self._gru_iterations_eager(coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, n01f, stem_2x)
        if self.mixed_precision not in self._graph_warm:   # plans / packed weights (fp32 and fp16 ones apart) are built
            self._graph_warm = self._graph_warm | {self.mixed_precision}     # lazily on a mode's first pass: never in a capture
            return self._gru_iterations_eager(coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, n01f, stem_2x)
        key = (id(corr_fn), id(inp_list), iters, tuple(coords1.shape), coords0.data_ptr(), id(stem_2x), self.mixed_precision)
        g = self._graph
        if g is None or g["key"] != key:
            self._graph = g = None                                   # drop the previous graph (and its memory pool) first
            st = {"key": key, "coords1": coords1.clone(), "net": [t.clone() for t in net_list], "n01f": n01f.clone()}
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                st["out"] = self._gru_iterations_eager(coords0, st["coords1"], None, iters, list(st["net"]), inp_list,
                                                       corr_fn, st["n01f"], stem_2x)
            st["graph"] = graph
            st["keep"] = (corr_fn, inp_list, stem_2x, coords0)       # what the recorded launches point at stays alive
            self._graph = g = st
        else:
            g["coords1"].copy_(coords1)
            for dst, src in zip(g["net"], net_list):
                dst.copy_(src)
            g["n01f"].copy_(n01f)
        g["graph"].replay()
        flow_up, c1, nl = g["out"]
        # the graph's outputs live in its pool and are overwritten by the next replay: hand out copies.  (The key's objects
        # are kept alive by the cached graph, so neither their ids nor their device addresses can be reused by a later forward.)
        return flow_up.clone(), c1.clone(), [t.clone() for t in nl]

    def _gru_iterations_eager(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, n01f, stem_2x):
        """igev_stereo_ddim.py:233-261 -- the 2-D update block is the caller's; the lookup is HIP."""
        if flow_init is not None:
            coords1 = coords1 + flow_init
        flow_up = None
        # mask_feat_4 is read only after the last iteration (:255-259): this build's update block can skip it elsewhere.
        # (The update block runs lookup + motion encoder on a side stream beside gru16 / gru08: update.py, OVERLAP.)
        from .update import BasicMultiUpdateBlock
        skip_mask = isinstance(self.update_block, BasicMultiUpdateBlock)
        amp = self.mixed_precision
        if amp:
            net_list, inp_list = round_gru_inputs_f16(net_list, inp_list)
        for itr in range(iters):
            flow = coords1 - coords0
            # this build's update block takes the lookup as a request and runs it fused with its first convolution
            corr = corr_fn.request(flow, coords1, n01f) if (skip_mask and hasattr(corr_fn, "request")) else corr_fn(flow, coords1, n01f)
            with torch.autocast("cuda", dtype=torch.float16, enabled=amp):      # :242-246
                if self.n_gru_layers == 3 and self.slow_fast_gru:
                    net_list = self.update_block(net_list, inp_list, iter32=True, iter16=False, iter08=False, update=False)
                if self.n_gru_layers >= 2 and self.slow_fast_gru:
                    net_list = self.update_block(net_list, inp_list, iter32=self.n_gru_layers == 3, iter16=True,
                                                 iter08=False, update=False)
                net_list, up_mask, delta_flow = self.update_block(net_list, inp_list, corr, flow,
                                                                  iter16=self.n_gru_layers == 3,
                                                                  iter08=self.n_gru_layers >= 2,
                                                                  **({"mask": itr == iters - 1} if skip_mask else {}))
            if amp:                # an update block that returns fp16 tensors (the reference's own): float32 from here on
                up_mask, delta_flow = (None if up_mask is None else up_mask.float()), delta_flow.float()
            coords1 = coords1 + delta_flow
            if itr == iters - 1:
                flow_up = self.upsample_disp(coords1 - coords0, up_mask, stem_2x)[:, :1]
        return flow_up, coords1, net_list

    def _coef(self, time, time_next, cof):
        k = _lib.DvDdimCoef()
        k.sqrt_recip_alpha, k.sqrt_recipm1_alpha = float(self.sqrt_recip[time]), float(self.sqrt_recipm1[time])
        k.dif_thr, k.unc_thr, k.cof, k.last = 5.0, float("inf"), cof, int(time_next < 0)
        k.clamp_max, k.ens_dif_thr = 47.0, 3.0        # clamp(pred, 0, 48-1) :265; output rule dif<3 :323-327
        if time_next >= 0:
            alpha, alpha_next = self.alphas_cumprod[time], self.alphas_cumprod[time_next]
            sigma = self.eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            k.sigma, k.c, k.sqrt_alpha_next = float(sigma), float((1 - alpha_next - sigma ** 2).sqrt()), float(alpha_next.sqrt())
        return k

    def _update(self, pred, used, coords0, n01, eps, fill, mask, ens, coef, want_pred_noise=False):
        b, c, h, w = n01.shape
        dev = pred.device
        x_start = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
        x_next = None if coef.last else torch.empty((b, c, h, w), dtype=torch.float64, device=dev)
        pn = torch.empty((b, c, h, w), dtype=torch.float64, device=dev) if want_pred_noise else None
        f32 = n01.dtype == torch.float32
        e32 = eps if (eps is not None and eps.dtype == torch.float32) else None
        e64 = eps if (eps is not None and eps.dtype == torch.float64) else None
        _lib.check(_lib.load().dv_ddim_step(pred.data_ptr(), 0, used.data_ptr(), coords0.data_ptr(),
                                            n01.data_ptr() if f32 else 0, 0 if f32 else n01.data_ptr(),
                                            _lib.ptr(e32), _lib.ptr(e64), _lib.ptr(fill), mask.data_ptr(),
                                            x_start.data_ptr(), _lib.ptr(pn), _lib.ptr(x_next), _lib.ptr(ens),
                                            b, c, h, w, ctypes.byref(coef), _lib.stream_ptr()), "dv_ddim_step")
        return x_start, x_next, pn

    @torch.no_grad()
    def model_predictions(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, noise, t, stem_2x):
        """igev_stereo_ddim.py:226-292 -> (pred_noise fp64, x_start fp32, pred [B,1,H,W], coords1)."""
        n01, n01f = self._filter(noise, t)
        pred, coords1, _ = self._gru_iterations(coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, n01f, stem_2x)
        pred = _dev_f32(pred, "pred")
        b, _, hh, ww = pred.shape
        c0 = _dev_f32(coords0, "coords0").reshape(b, hh // 4, ww // 4)
        mask = torch.zeros((b, hh // 4, ww // 4), dtype=torch.float32, device=pred.device)
        coef = self._coef(int(t.reshape(-1)[0]), -1, 0.0)
        p2 = pred.reshape(b, hh, ww)
        x_start, _, pn = self._update(p2, p2, c0, n01, None, None, mask, None, coef, want_pred_noise=True)
        return pn, x_start, pred, coords1

    @torch.no_grad()
    def ddim_sample(self, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, used, asd, stem_2x,
                    noise: Optional[Callable] = None, generator: Optional[torch.Generator] = None):
        """igev_stereo_ddim.py:294-359.  Draws in reference order: 'x_T' (randn_like(asd) :303), then per
        non-final step 'eps' (:338) and 'q' (randn_like inside q_sample :343)."""
        asd = _dev_f32(asd, "asd")
        b, d, h, w = asd.shape
        dev = asd.device
        used2 = _dev_f32(used, "used").reshape(b, 4 * h, 4 * w)

        def draw(kind, shape, dtype):
            if noise is not None:
                return noise(kind, shape, dtype).to(device=dev, dtype=dtype).contiguous()
            return torch.randn(shape, device=dev, dtype=dtype, generator=generator)

        img = draw("x_T", tuple(asd.shape), torch.float32)
        mask = torch.zeros((b, h, w), dtype=torch.float32, device=dev)
        ens = used2 * self.ensemble_cof[0]
        for i, (time, time_next) in enumerate(self._time_pairs()):
            eps = fill = None
            if time_next >= 0:
                eps = draw("eps", tuple(img.shape), img.dtype)
                fill = (self.sqrt_ac[time].item() * asd.double()
                        + self.sqrt_1mac[time].item() * draw("q", tuple(asd.shape), asd.dtype).double()).contiguous()
            _, x_start, x_next, coords1, net_list = self.ddim_step(i, coords0, coords1, flow_init, iters, net_list, inp_list,
                                                                   corr_fn, used2, img, mask, ens, eps, fill, stem_2x)
            img = x_start if time_next < 0 else x_next
        return ens

    @torch.no_grad()
    def ddim_step(self, i, coords0, coords1, flow_init, iters, net_list, inp_list, corr_fn, used, img, mask, ens=None,
                  eps=None, fill=None, stem_2x=None):
        """Iteration ``i`` of the loop of igev_stereo_ddim.py:306-351 from explicit state: ``img`` entering the step,
        ``mask`` (updated in place), ``coords1`` and the hidden states ``net_list`` as the previous step left them,
        ``eps`` = randn_like(img), ``fill`` = q_sample(asd, t).  Returns (pred [B,4h,4w], x_start fp32,
        x_next fp64 | None, coords1, net_list)."""
        time, time_next = self._time_pairs()[i]
        b, _, h, w = img.shape
        dev = img.device
        t = torch.full((b,), time, device=dev, dtype=torch.long)
        n01, n01f = self._filter(img, t)
        pred, coords1, net_list = self._gru_iterations(coords0, coords1, flow_init, iters, net_list, inp_list,
                                                       corr_fn, n01f, stem_2x)
        pred2 = _dev_f32(pred, "pred").reshape(b, 4 * h, 4 * w)
        used2 = _dev_f32(used, "used").reshape(b, 4 * h, 4 * w)
        c0 = _dev_f32(coords0, "coords0").reshape(b, h, w)
        coef = self._coef(time, time_next, self.ensemble_cof[i + 1])
        x_start, x_next, _ = self._update(pred2, used2, c0, n01, eps, fill, mask, ens, coef)
        return pred2, x_start, x_next, coords1, net_list


# ---------------------------------------------------------------------------------------------------
# The once-per-pair cost-volume front of IGEVStereo_ddim.forward (igev_stereo_ddim.py:377-386):
# gwc volume (8 groups) -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier -> softmax -> regression.
# Module and parameter names are the reference's, so its checkpoints load unchanged
# (`corr_stem.conv.weight`, `cost_agg.feature_att_16.feat_att.1.bias`, ...).
# ---------------------------------------------------------------------------------------------------
# ---------------------------------------------------------------------------------------------------
# The once-per-pair 2-D front on the in-tree kernels (round 5): every nn.Conv2d / nn.ConvTranspose2d / BatchNorm2d (eval) /
# InstanceNorm2d / activation of the feature pyramid, the stems, the context encoder and the spx heads runs through
# `hip_conv2d` / `instance_norm_act` -- no MIOpen, so a rerun and a shard of a batch give the same bits as the batch
# (MIOpen may pick another solver on a later call or for another batch size).  Plans are cached per module and rebuilt when
# a weight is loaded, moved or overwritten in place (key = data pointers + versions).  A tensor that asks for gradients
# takes the module's own torch expression (explicit autograd dispatch, like submodule.py's builders).
# ---------------------------------------------------------------------------------------------------
import weakref

_PLAN_CACHE = weakref.WeakKeyDictionary()


def _wants_autograd(x) -> bool:
    return torch.is_grad_enabled() and x.requires_grad


def _train_mode(m: nn.Module) -> bool:
    """The training route of a volume-side module, decided per module like the update block's (update.py): the module is
    in train mode and autograd records.  Not ``x.requires_grad``: a frozen backbone still trains the volume weights."""
    return m.training and torch.is_grad_enabled()


def _bn_tuple(bn):
    return None if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)


def hip_conv2d(conv: nn.Module, x: torch.Tensor, bn: Optional[nn.BatchNorm2d] = None, act: int = ACT_NONE,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``act(bn(conv(x)) [+ residual])`` for nn.Conv2d (k 1 / 3 with stride 1 / 2, k 3 / 5 / 7 with <= 4 input channels) and
    nn.ConvTranspose2d (k 4, stride 2, padding 1) with eval-mode BatchNorm folded, on the HIP kernels."""
    x = _dev_f32(x, "x")
    if bn is not None and bn.training:
        raise _lib.DiffuVolumeError("BatchNorm2d in training mode: the HIP front folds running statistics (model.eval())")
    tensors = [conv.weight, conv.bias] + (list(_bn_tuple(bn)) if bn is not None else [])
    key = (act, weight_key(t for t in tensors if t is not None))
    hit = _PLAN_CACHE.get(conv)
    if hit is None or hit[0] != key:
        w = conv.weight
        if isinstance(conv, nn.ConvTranspose2d):
            if conv.kernel_size != (4, 4) or conv.stride != (2, 2) or conv.padding != (1, 1):
                raise _lib.DiffuVolumeError("ConvTranspose2d on the HIP front: kernel 4, stride 2, padding 1")
            plan = Deconv2dK4S2Plan(w, _bn_tuple(bn), bias=conv.bias, act=act, eps=bn.eps if bn is not None else 1e-5)
        else:
            k, st = conv.kernel_size[0], conv.stride[0]
            if (conv.kernel_size != (k, k) or conv.stride != (st, st) or conv.padding != (k // 2, k // 2)
                    or conv.dilation != (1, 1) or conv.groups != 1 or st not in (1, 2)):
                raise _lib.DiffuVolumeError(f"Conv2d on the HIP front: square kernel, padding k/2, stride 1 or 2, got {conv}")
            if w.shape[1] <= 4 and k in (3, 5, 7):
                plan = _FewInPlan(w, conv.bias, bn, st, act)
            elif k in (1, 3):
                plan = Conv2dPlan(w, _bn_tuple(bn), act=act, bias=conv.bias, stride=st, eps=bn.eps if bn is not None else 1e-5)
            else:
                raise _lib.DiffuVolumeError(f"Conv2d on the HIP front: unsupported layer {conv}")
        _PLAN_CACHE[conv] = hit = (key, plan)
    plan = hit[1]
    if residual is not None:
        if isinstance(plan, Conv2dPlan):
            return plan(x, residual=residual)
        raise _lib.DiffuVolumeError("residual: 3x3 / 1x1 Conv2d layers only")
    return plan(x)


class _FewInPlan:
    """nn.Conv2d with <= 4 input channels (the RGB stems, the 7x7 stride-2 stem of the context encoder) [+ eval BatchNorm]
    [+ activation] on `dv_conv2d_fewin_f32`."""

    def __init__(self, w, bias, bn, stride, act):
        self.w = w.detach().float().contiguous()
        self.bias = None if bias is None else bias.detach().float().contiguous()
        self.cout, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        self.stride, self.act = stride, act
        self.scale = self.shift = None
        if bn is not None:
            sc = (bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps))
            self.scale = sc.float().contiguous()
            self.shift = (bn.bias.detach().double() - bn.running_mean.detach().double() * sc).float().contiguous()

    def __call__(self, x):
        b, c, h, w = x.shape
        if c != self.cin:
            raise RuntimeError(f"expected {self.cin} input channels, got {c}")
        out = torch.empty((b, self.cout, (h - 1) // self.stride + 1, (w - 1) // self.stride + 1), dtype=torch.float32,
                          device=x.device)
        with torch.cuda.device(x.device):
            _lib.check(_lib.load().dv_conv2d_fewin_f32(x.data_ptr(), self.w.data_ptr(), _lib.ptr(self.bias),
                                                       _lib.ptr(self.scale), _lib.ptr(self.shift), out.data_ptr(), b, c, h, w,
                                                       self.cout, self.k, self.stride, self.act, _lib.stream_ptr()),
                       "dv_conv2d_fewin_f32")
        return out


def instance_norm_act(x: torch.Tensor, act: int = ACT_NONE, eps: float = 1e-5, inplace: bool = True) -> torch.Tensor:
    """nn.InstanceNorm2d (affine=False) + activation: `dv_instance_norm_act_f32`, one block per (b, c) plane."""
    x = _dev_f32(x, "x")
    b, c, h, w = x.shape
    out = x if inplace else torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().dv_instance_norm_act_f32(x.data_ptr(), out.data_ptr(), b * c, h * w, float(eps), act,
                                                        _lib.stream_ptr()), "dv_instance_norm_act_f32")
    return out




def hip_sequential(seq, x: torch.Tensor) -> torch.Tensor:
    """An nn.Sequential of the front (stems, spx heads, stub backbone stages, FeatureAtt's gate) with every
    [conv][BatchNorm2d | InstanceNorm2d][ReLU | ReLU6 | LeakyReLU(0.01)] run fused on the HIP kernels; members that have
    a HIP forward of their own (BasicConv, BasicConv_IN, ResidualBlock, Conv2x...) are called."""
    mods = list(seq) if isinstance(seq, (nn.Sequential, list, tuple)) else [seq]
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            j, bn, inorm, act, clamp6 = i + 1, None, None, ACT_NONE, False
            if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
                bn, j = mods[j], j + 1
            elif j < len(mods) and isinstance(mods[j], nn.InstanceNorm2d):
                inorm, j = mods[j], j + 1
                if inorm.affine or inorm.track_running_stats:
                    raise _lib.DiffuVolumeError("InstanceNorm2d on the HIP front: affine=False, no running statistics")
            if j < len(mods) and isinstance(mods[j], (nn.ReLU, nn.ReLU6, nn.LeakyReLU)):
                a = mods[j]
                if isinstance(a, nn.LeakyReLU) and abs(a.negative_slope - 0.01) > 1e-12:
                    raise _lib.DiffuVolumeError("LeakyReLU on the HIP front: negative_slope 0.01")
                act = ACT_LEAKY if isinstance(a, nn.LeakyReLU) else ACT_RELU            # (isinstance: subclasses of the three too)
                clamp6, j = isinstance(a, nn.ReLU6), j + 1
            if inorm is not None:
                x = instance_norm_act(hip_conv2d(m, x), act, inorm.eps)
            else:
                x = hip_conv2d(m, x, bn, act)
            if clamp6:
                x = x.clamp_(max=6.0)
            i = j
        elif isinstance(m, nn.Sequential):
            x = hip_sequential(m, x)
            i += 1
        elif isinstance(m, (nn.Identity, nn.Dropout, nn.Dropout2d)):
            i += 1
        else:
            x = m(x)
            i += 1
    return x


class BasicConv(nn.Module):
    """core/submodule.py:9-35: conv (bias=False) [+ BatchNorm] [+ LeakyReLU(0.01)].  The 3-D flavours run as
    fused HIP plans (``plan()``); ``forward`` is the 2-D flavour used inside FeatureAtt."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, bn=True, relu=True, **kwargs):
        super().__init__()
        self.relu, self.use_bn, self.is_3d, self.deconv = relu, bn, is_3d, deconv
        if is_3d:
            self.conv = (nn.ConvTranspose3d if deconv else nn.Conv3d)(in_channels, out_channels, bias=False, **kwargs)
            self.bn = nn.BatchNorm3d(out_channels)
        else:
            self.conv = (nn.ConvTranspose2d if deconv else nn.Conv2d)(in_channels, out_channels, bias=False, **kwargs)
            self.bn = nn.BatchNorm2d(out_channels)

    def plan(self):
        if not self.is_3d:
            raise _lib.DiffuVolumeError("only the 3-D BasicConv flavours have HIP plans")
        bn = (self.bn.weight, self.bn.bias, self.bn.running_mean, self.bn.running_var) if self.use_bn else None
        act = ACT_LEAKY if self.relu else ACT_NONE
        if self.deconv:
            return Deconv3dPlan(self.conv.weight, bn, act=act, eps=self.bn.eps)
        return Conv3dPlan(self.conv.weight, bn, stride=self.conv.stride[0], act=act, eps=self.bn.eps)

    def train_forward(self, x, plan=None):
        """The training route: the convolution as an autograd function on the HIP kernels (train3d / train2d), BatchNorm
        on batch statistics (running buffers updated) and LeakyReLU in PyTorch.  No plan is built or refreshed here;
        ``plan`` (2-D transposed flavour only): a callable that returns the layer's cached train2d.TrainDeconvPlan."""
        if self.is_3d:
            x = (train3d.conv_transpose3d_module if self.deconv else train3d.conv3d_module)(self.conv, x)
        elif self.deconv:
            x = train2d.conv_transpose2d_module(self.conv, x, plan)
        else:
            x = train2d.conv2d_module(self.conv, x)
        if self.use_bn:
            x = self.bn(x)
        return F.leaky_relu(x, 0.01) if self.relu else x

    def forward(self, x):
        if self.is_3d:
            raise _lib.DiffuVolumeError("3-D BasicConv runs through its HIP plan, not nn.Module.forward")
        if _wants_autograd(x):
            x = self.conv(x)
            if self.use_bn:
                x = self.bn(x)
            return F.leaky_relu(x, 0.01) if self.relu else x
        return hip_conv2d(self.conv, x, self.bn if self.use_bn else None, ACT_LEAKY if self.relu else ACT_NONE)


class FeatureAtt(nn.Module):
    """core/submodule.py:226-239: image-feature guided channel gate of a cost volume."""

    def __init__(self, cv_chan, feat_chan):
        super().__init__()
        self.feat_att = nn.Sequential(BasicConv(feat_chan, feat_chan // 2, kernel_size=1, stride=1, padding=0),
                                      nn.Conv2d(feat_chan // 2, cv_chan, 1))

    def forward(self, cv, feat, inplace=False):
        if _train_mode(self):                   # out of place: the gate's backward reads the ungated volume
            logit = train2d.conv2d_module(self.feat_att[1], self.feat_att[0].train_forward(feat))
            return train3d.feature_gate_train(cv, logit)
        return feature_gate(cv, hip_sequential(self.feat_att, feat), inplace=inplace)


def _seq_plans(seq):
    return [m.plan() for m in seq]


def _run(plans, x):
    for p in plans:
        x = p(x)
    return x


def _run_train(seq, x):
    for m in seq:
        x = m.train_forward(x)
    return x


class hourglass(PlanCache, nn.Module):
    """igev_stereo_ddim.py:24-91 (`hourglass(8)`, runs once per pair on the gated gwc volume)."""

    def __init__(self, in_channels):
        super().__init__()
        c = in_channels
        k3 = dict(is_3d=True, bn=True, relu=True, kernel_size=3, padding=1, dilation=1)
        self.conv1 = nn.Sequential(BasicConv(c, c * 2, stride=2, **k3), BasicConv(c * 2, c * 2, stride=1, **k3))
        self.conv2 = nn.Sequential(BasicConv(c * 2, c * 4, stride=2, **k3), BasicConv(c * 4, c * 4, stride=1, **k3))
        self.conv3 = nn.Sequential(BasicConv(c * 4, c * 6, stride=2, **k3), BasicConv(c * 6, c * 6, stride=1, **k3))
        up = dict(deconv=True, is_3d=True, kernel_size=(4, 4, 4), padding=(1, 1, 1), stride=(2, 2, 2))
        self.conv3_up = BasicConv(c * 6, c * 4, bn=True, relu=True, **up)
        self.conv2_up = BasicConv(c * 4, c * 2, bn=True, relu=True, **up)
        self.conv1_up = BasicConv(c * 2, 8, bn=False, relu=False, **up)

        def agg(cin, cout):
            return nn.Sequential(BasicConv(cin, cout, is_3d=True, kernel_size=1, padding=0, stride=1),
                                 BasicConv(cout, cout, is_3d=True, kernel_size=3, padding=1, stride=1),
                                 BasicConv(cout, cout, is_3d=True, kernel_size=3, padding=1, stride=1))

        self.agg_0 = agg(c * 8, c * 4)
        self.agg_1 = agg(c * 4, c * 2)
        self.feature_att_8 = FeatureAtt(c * 2, 64)
        self.feature_att_16 = FeatureAtt(c * 4, 192)
        self.feature_att_32 = FeatureAtt(c * 6, 160)
        self.feature_att_up_16 = FeatureAtt(c * 4, 192)
        self.feature_att_up_8 = FeatureAtt(c * 2, 64)

    def _build_plans(self, slot):
        p = {n: _seq_plans(getattr(self, n)) for n in ("conv1", "conv2", "conv3", "agg_0", "agg_1")}
        for n in ("conv3_up", "conv2_up", "conv1_up"):
            p[n] = getattr(self, n).plan()
        return p

    def _train_forward(self, x, features):
        conv1 = self.feature_att_8(_run_train(self.conv1, x), features[1])
        conv2 = self.feature_att_16(_run_train(self.conv2, conv1), features[2])
        conv3 = self.feature_att_32(_run_train(self.conv3, conv2), features[3])
        conv2 = _run_train(self.agg_0, torch.cat((self.conv3_up.train_forward(conv3), conv2), dim=1))
        conv2 = self.feature_att_up_16(conv2, features[2])
        conv1 = _run_train(self.agg_1, torch.cat((self.conv2_up.train_forward(conv2), conv1), dim=1))
        conv1 = self.feature_att_up_8(conv1, features[1])
        return self.conv1_up.train_forward(conv1)

    def forward(self, x, features):
        if _train_mode(self):
            return self._train_forward(x, features)
        p = self.plans()
        conv1 = self.feature_att_8(_run(p["conv1"], x), features[1], inplace=True)
        conv2 = self.feature_att_16(_run(p["conv2"], conv1), features[2], inplace=True)
        conv3 = self.feature_att_32(_run(p["conv3"], conv2), features[3], inplace=True)
        conv2 = _run(p["agg_0"], torch.cat((p["conv3_up"](conv3), conv2), dim=1))
        conv2 = self.feature_att_up_16(conv2, features[2], inplace=True)
        conv1 = _run(p["agg_1"], torch.cat((p["conv2_up"](conv2), conv1), dim=1))
        conv1 = self.feature_att_up_8(conv1, features[1], inplace=True)
        return p["conv1_up"](conv1)


def _cost_volume_plans(m):
    return m.corr_stem.plan(), Conv3dPlan(m.classifier.weight, None, stride=1, act=ACT_NONE)


def _cost_volume(m, match_left, match_right, features_left, max_disp):
    """IGEVStereo_ddim :378-386 on the modules of ``m`` (an IGEVCostVolume or the IGEVStereo_ddim itself): gwc (8 groups)
    -> corr_stem -> FeatureAtt -> hourglass(8) -> classifier -> softmax + regression."""
    if _train_mode(m):
        return _cost_volume_train(m, match_left, match_right, features_left, max_disp)
    m.refresh_plans()
    stem, classifier = m.plans()
    gwc = stem(build_gwc_volume(match_left, match_right, max_disp // 4, 8))
    gwc = m.corr_feature_att(gwc, features_left[0], inplace=True)
    geo = m.cost_agg(gwc, features_left)
    return geo, softmax_regress(classifier(geo)).unsqueeze(1)          # F.softmax + disparity_regression :382-383


def _cost_volume_train(m, match_left, match_right, features_left, max_disp):
    """The same front for training (train mode with autograd recording): every convolution and gate an autograd function
    on the HIP kernels, BatchNorm / LeakyReLU / softmax / regression PyTorch, the gwc volume its differentiable expression
    (whether or not the features ask for gradients, so that a frozen backbone gives the same bits)."""
    for name, t in (("match_left", match_left), ("match_right", match_right),
                    *((f"features_left[{i}]", f) for i, f in enumerate(features_left))):
        if not t.is_cuda:
            raise _lib.DiffuVolumeError(f"{name} is on {t.device}: training runs on the MI355X (no CPU fallback)")
    if match_left.dim() != 4 or match_left.shape != match_right.shape:
        raise RuntimeError(f"feature shapes differ or are not 4-D: {tuple(match_left.shape)} vs {tuple(match_right.shape)}")
    d, (h, w) = max_disp // 4, match_left.shape[2:]
    if d % 8 or h % 8 or w % 8:
        raise _lib.DiffuVolumeError(f"training the cost-volume front needs d, h, w of the 1/4-resolution volume to be "
                                    f"multiples of 8 (three stride-2 levels whose skips are concatenated), got {d} x {h} x {w}")
    gwc = _gwc_volume_autograd(match_left, match_right, d, 8)
    gwc = m.corr_feature_att(m.corr_stem.train_forward(gwc), features_left[0])
    geo = m.cost_agg(gwc, features_left)
    prob = F.softmax(train3d.conv3d_module(m.classifier, geo).squeeze(1), dim=1)            # :382
    disp_values = torch.arange(0, d, dtype=prob.dtype, device=prob.device).view(1, d, 1, 1)
    return geo, torch.sum(prob * disp_values, 1, keepdim=True)                               # disparity_regression :383


class IGEVCostVolume(PlanCache, nn.Module):
    """The volume-side modules of IGEVStereo_ddim (:196-199) and the part of its forward that uses them
    (:377-386).  ``forward(match_left, match_right, features_left)`` returns the geometry encoding volume
    [B,8,D/4,h,w] (what Combined_Geo_Encoding_Volume filters at every GRU iteration) and `init_disp`
    [B,1,h,w]."""

    def __init__(self, max_disp: int = 192):
        super().__init__()
        self.max_disp = max_disp
        self.corr_stem = BasicConv(8, 8, is_3d=True, kernel_size=3, stride=1, padding=1)
        self.corr_feature_att = FeatureAtt(8, 96)
        self.cost_agg = hourglass(8)
        self.classifier = nn.Conv3d(8, 1, 3, 1, 1, bias=False)

    def _build_plans(self, slot):
        return _cost_volume_plans(self)

    def forward(self, match_left, match_right, features_left):
        return _cost_volume(self, match_left, match_right, features_left, self.max_disp)


# ---------------------------------------------------------------------------------------------------
# IGEVStereo_ddim: the drop-in module (KITTI15/core/igev_stereo_ddim.py:118-224 constructor, :361-427 eval forward).
# Module / buffer names are the reference's, so its checkpoints load with strict=True.  On HIP: gwc volume, corr_stem,
# FeatureAtt gates, hourglass(8), classifier + softmax + regression, the filtered geometry lookup, the whole update
# block, the convex upsampling (softmax + 9-tap gather) and the DDIM state update.  PyTorch (2-D, once per pair or
# once per DDIM step): the MobileNetV2 feature pyramid, the context encoder, the stems and the spx heads' convolutions.
# ---------------------------------------------------------------------------------------------------
def _context_upsample_shapes(disp_low, up_weights):
    b, c, h, w = disp_low.shape
    if c != 1 or tuple(up_weights.shape) != (b, 9, 4 * h, 4 * w):
        raise RuntimeError(f"context_upsample: disp_low [B,1,h,w] and up_weights [B,9,4h,4w], got "
                           f"{tuple(disp_low.shape)} and {tuple(up_weights.shape)}")
    return b, h, w


def _context_upsample_launch(disp_low, up_weights, scale, apply_softmax):
    b, h, w = _context_upsample_shapes(disp_low, up_weights)
    out = torch.empty((b, 4 * h, 4 * w), dtype=torch.float32, device=disp_low.device)
    with torch.cuda.device(disp_low.device):
        _lib.check(_lib.load().dv_context_upsample_f32(disp_low.data_ptr(), up_weights.data_ptr(), out.data_ptr(), b, h,
                                                       w, float(scale), int(bool(apply_softmax)), _lib.stream_ptr()),
                   "dv_context_upsample_f32")
    return out


class ContextUpsampleFn(torch.autograd.Function):
    """context_upsample with both gradients on ``dv_context_upsample_bwd_f32``: the forward is the inference launch (its
    bits); the backward recomputes the softmax from the saved logits -- no probabilities, no unfolded or x4-repeated
    disparity are kept -- and gathers, so two runs give the same bits."""

    @staticmethod
    def forward(ctx, disp_low, up_weights, scale, apply_softmax):
        disp_low, up_weights = disp_low.contiguous(), up_weights.contiguous()
        ctx.save_for_backward(disp_low, up_weights)
        ctx.scale, ctx.apply_softmax = scale, apply_softmax
        return _context_upsample_launch(disp_low, up_weights, scale, apply_softmax)

    @staticmethod
    def backward(ctx, g):
        disp_low, up_weights = ctx.saved_tensors
        b, _, h, w = disp_low.shape
        g = g.contiguous()
        need_d, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_d or need_w):
            return None, None, None, None
        d_w = torch.empty_like(up_weights) if need_w else None
        d_d = torch.empty_like(disp_low) if need_d else None
        sums = torch.empty((b, 9, h, w), dtype=torch.float32, device=g.device) if need_d else None
        with torch.cuda.device(g.device):
            _lib.check(_lib.load().dv_context_upsample_bwd_f32(disp_low.data_ptr(), up_weights.data_ptr(), g.data_ptr(),
                                                               _lib.ptr(d_w), _lib.ptr(d_d), _lib.ptr(sums), b, h, w,
                                                               float(ctx.scale), int(ctx.apply_softmax), _lib.stream_ptr()),
                       "dv_context_upsample_bwd_f32")
        return d_d, d_w, None, None


def context_upsample(disp_low: torch.Tensor, up_weights: torch.Tensor, scale: float = 1.0,
                     apply_softmax: bool = False) -> torch.Tensor:
    """core/submodule.py:241-253: disp_low [B,1,h,w], up_weights [B,9,4h,4w] -> [B,4h,4w].  ``apply_softmax`` /
    ``scale`` fold the ``F.softmax(spx_pred, 1)`` and ``disp*4.`` of the call site into the same pass.  Differentiable
    when autograd records and an input asks for gradients (``ContextUpsampleFn``; the reference's torch expression under
    DV_TRAIN_CONV2D=torch); otherwise the inference launch."""
    if torch.is_grad_enabled() and (disp_low.requires_grad or up_weights.requires_grad):
        train2d._check(disp_low, "disp_low")
        train2d._check(up_weights, "up_weights")
        b, h, w = _context_upsample_shapes(disp_low, up_weights)
        if train2d.route() == "torch":
            weights = F.softmax(up_weights, 1) if apply_softmax else up_weights
            unfold = F.unfold(disp_low * scale, 3, 1, 1).reshape(b, -1, h, w)
            unfold = F.interpolate(unfold, (h * 4, w * 4), mode="nearest").reshape(b, 9, h * 4, w * 4)
            return (unfold * weights).sum(1)
        return ContextUpsampleFn.apply(disp_low, up_weights, float(scale), bool(apply_softmax))
    disp_low, up_weights = _dev_f32(disp_low, "disp_low"), _dev_f32(up_weights, "up_weights")
    return _context_upsample_launch(disp_low, up_weights, scale, apply_softmax)


class BasicConv_IN(nn.Module):
    """core/submodule.py:79-107 (2-D flavours only): conv (bias=False) [+ InstanceNorm2d] [+ LeakyReLU(0.01)]."""

    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, IN=True, relu=True, **kwargs):
        super().__init__()
        if is_3d:
            raise _lib.DiffuVolumeError("IGEV uses BasicConv_IN in 2-D only")
        self.relu, self.use_in = relu, IN
        self.conv = (nn.ConvTranspose2d if deconv else nn.Conv2d)(in_channels, out_channels, bias=False, **kwargs)
        self.IN = nn.InstanceNorm2d(out_channels)

    def forward(self, x):
        if _wants_autograd(x):
            x = self.conv(x)
            if self.use_in:
                x = self.IN(x)
            return F.leaky_relu(x, 0.01) if self.relu else x
        act = ACT_LEAKY if self.relu else ACT_NONE
        if self.use_in:
            return instance_norm_act(hip_conv2d(self.conv, x), act, self.IN.eps)
        return hip_conv2d(self.conv, x, None, act)


class _Conv2xBase(nn.Module):
    """core/submodule.py:36-76 / :110-150: stride-2 (de)convolution, resize to the skip tensor, concat (or add), 3x3."""

    def _finish(self, x, rem):
        x = self.conv1(x)
        if x.shape != rem.shape:
            x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="nearest")
        x = torch.cat((x, rem), 1) if self.concat else x + rem
        return self.conv2(x)

    def forward(self, x, rem):
        return self._finish(x, rem)


class Conv2x(_Conv2xBase):
    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, concat=True, keep_concat=True, bn=True,
                 relu=True, keep_dispc=False):
        super().__init__()
        if is_3d or keep_dispc:
            raise _lib.DiffuVolumeError("IGEV uses Conv2x in 2-D only")
        self.concat = concat
        self.conv1 = BasicConv(in_channels, out_channels, deconv, False, bn=True, relu=True,
                               kernel_size=4 if deconv else 3, stride=2, padding=1)
        cin, cout = (out_channels * 2, out_channels * (2 if keep_concat else 1)) if concat else (out_channels, out_channels)
        self.conv2 = BasicConv(cin, cout, False, False, bn, relu, kernel_size=3, stride=1, padding=1)


class Conv2x_IN(_Conv2xBase):
    def __init__(self, in_channels, out_channels, deconv=False, is_3d=False, concat=True, keep_concat=True, IN=True,
                 relu=True, keep_dispc=False):
        super().__init__()
        if is_3d or keep_dispc:
            raise _lib.DiffuVolumeError("IGEV uses Conv2x_IN in 2-D only")
        self.concat = concat
        self.conv1 = BasicConv_IN(in_channels, out_channels, deconv, False, IN=True, relu=True,
                                  kernel_size=4 if deconv else 3, stride=2, padding=1)
        cin, cout = (out_channels * 2, out_channels * (2 if keep_concat else 1)) if concat else (out_channels, out_channels)
        self.conv2 = BasicConv_IN(cin, cout, False, False, IN, relu, kernel_size=3, stride=1, padding=1)


# ---------------------------------------------------------------------------------------------------
# The convex-upsampling head (igev_stereo_ddim.py:203-211 `upsample_disp`, once per GRU iteration in the train loop
# :441-457; :390-393 + :462 for `init_disp`), shared by IGEVStereo_ddim and IGEVUpsampler.
# ---------------------------------------------------------------------------------------------------
def _spx_plans(m):
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    bn = lambda c: (c.bn.weight, c.bn.bias, c.bn.running_mean, c.bn.running_var) if c.use_bn else ()
    act = lambda c: ACT_LEAKY if c.relu else ACT_NONE
    return (Deconv2dK4S2Plan(c1.conv.weight, bn(c1) or None, act=act(c1), eps=c1.bn.eps),
            Conv2dPlan(c2.conv.weight, bn(c2) or None, act=act(c2), eps=c2.bn.eps),
            Deconv2dK4S2Plan(head.weight, None, bias=head.bias))


def _spx_train_key(m):
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    return weight_key((c1.conv.weight, c2.conv.weight, head.weight, head.bias))


def _spx_train_plans(m):
    """(key, plans) of the three layers for the training route: forward plans without BatchNorm / activation and the
    packed weights of the input gradients.  The key covers the three layers' weights only: in train mode BatchNorm
    rewrites its running statistics on every call, which the module-wide key of ``refresh_plans`` would take for a change."""
    c1, c2, head = m.spx_2_gru.conv1, m.spx_2_gru.conv2, m.spx_gru[0]
    return _spx_train_key(m), (train2d.TrainDeconvPlan(c1.conv.weight), train2d.TrainConvPlan(c2.conv, ACT_NONE),
                               train2d.TrainDeconvPlan(head.weight, head.bias))


def _upsample_train_entry(*named):
    for name, t in named:
        if not t.is_cuda:
            raise _lib.DiffuVolumeError(f"{name} is on {t.device}: training runs on the MI355X (no CPU fallback)")
    if torch.is_autocast_enabled("cuda"):
        raise _lib.DiffuVolumeError("the convex-upsampling head trains in float32: fp16 / bf16 autocast is not supported "
                                    "in train mode (mixed-precision training is not implemented)")


def _upsample_disp(m, disp, mask_feat_4, stem_2x, slot, train_slot):
    if _train_mode(m):
        return _upsample_disp_train(m, disp, mask_feat_4, stem_2x, train_slot)
    if mask_feat_4.is_cuda and m.spx_2_gru.concat:
        up, mix, head = m.plans(slot)
        x = up(mask_feat_4)
        if x.shape != stem_2x.shape:
            x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
        spx_pred = head(mix([x, stem_2x]))              # torch.cat((x, rem), 1) is never materialised
    else:
        spx_pred = m.spx_gru(m.spx_2_gru(mask_feat_4, stem_2x))
    return context_upsample(disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


def _upsample_disp_train(m, disp, mask_feat_4, stem_2x, train_slot):
    """`upsample_disp` for training (train mode with autograd recording): both transposed convolutions and the 3x3 over
    the un-materialised [x | stem_2x] concatenation autograd functions on the HIP kernels (train2d), BatchNorm on batch
    statistics and LeakyReLU in PyTorch, softmax + convex upsampling one differentiable HIP pass."""
    _upsample_train_entry(("disp", disp), ("mask_feat_4", mask_feat_4), ("stem_2x", stem_2x))
    c = m.spx_2_gru
    if not c.concat:
        raise _lib.DiffuVolumeError("the training route of upsample_disp needs spx_2_gru built with concat=True")

    def plan(i):
        def get():                                   # only called on the HIP route; rebuilt when a weight was written
            if m.plans(train_slot)[0] != _spx_train_key(m):
                m.drop_slot(train_slot)
            return m.plans(train_slot)[1][i]
        return get
    x = c.conv1.train_forward(mask_feat_4, plan(0))
    if x.shape != stem_2x.shape:
        x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
    x = train2d.conv_cat(plan(1), c.conv2.conv, ACT_NONE, [x, stem_2x])
    if c.conv2.use_bn:
        x = c.conv2.bn(x)
    if c.conv2.relu:
        x = F.leaky_relu(x, 0.01)
    spx_pred = train2d.conv_transpose2d_module(m.spx_gru[0], x, plan(2))
    return context_upsample(disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


def _basic_in_train(m, x):
    """A 2-D BasicConv_IN on the training route: the convolution an autograd function on the HIP kernels (train2d; plans
    built per call: these layers run once per pair), InstanceNorm and LeakyReLU in PyTorch."""
    conv = train2d.conv_transpose2d_module if isinstance(m.conv, nn.ConvTranspose2d) else train2d.conv2d_module
    x = conv(m.conv, x)
    if m.use_in:
        x = m.IN(x)
    return F.leaky_relu(x, 0.01) if m.relu else x


def _spx_init_train(m, features_left0, stem_2x):
    """The spx_4 / spx_2 / spx logits (:390-392) on the training route, on the modules of ``m`` (an IGEVUpsampler or the
    IGEVStereo_ddim itself)."""
    s4, c = m.spx_4, m.spx_2
    x = s4[3](s4[2](train2d.conv2d_module(s4[1], _basic_in_train(s4[0], features_left0))))
    x = _basic_in_train(c.conv1, x)
    if x.shape != stem_2x.shape:
        x = F.interpolate(x, size=(stem_2x.shape[-2], stem_2x.shape[-1]), mode="nearest")
    return train2d.conv_transpose2d_module(m.spx[0], _basic_in_train(c.conv2, torch.cat((x, stem_2x), 1)))


class IGEVUpsampler(PlanCache, nn.Module):
    """The upsampling-side modules of IGEVStereo_ddim (:110-112 `spx_2_gru` / `spx_gru`, :104-108 `spx_4` / `spx_2` /
    `spx`) under the reference's attribute names, and the parts of its forward that use them.
    ``forward(disp, mask_feat_4, stem_2x)`` is `upsample_disp` (:203-211) -> [B,1,4h,4w]; ``init_forward(features_left0,
    stem_2x, init_disp)`` is :390-393 + :462 -> [B,1,4h,4w].  In eval mode (or under no_grad) ``forward`` runs the fused
    inference plans; in train mode with autograd recording it is differentiable on the HIP kernels (see
    ``_upsample_disp_train``).  `spx_4` / `spx_2` / `spx` run once per pair: the modules' own forwards in eval mode, in train
    mode their convolutions as the same autograd functions (plans built per call, InstanceNorm / activations PyTorch)
    and their softmax + convex upsampling of `init_disp` the same differentiable HIP pass."""

    def __init__(self):
        super().__init__()
        self.spx = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))
        self.spx_2 = Conv2x_IN(24, 32, True)
        self.spx_4 = nn.Sequential(BasicConv_IN(96, 24, kernel_size=3, stride=1, padding=1),
                                   nn.Conv2d(24, 24, 3, 1, 1, bias=False), nn.InstanceNorm2d(24), nn.ReLU())
        self.spx_2_gru = Conv2x(32, 32, True)
        self.spx_gru = nn.Sequential(nn.ConvTranspose2d(2 * 32, 9, kernel_size=4, stride=2, padding=1))

    def _build_plans(self, slot):
        return _spx_train_plans(self) if slot == "train" else _spx_plans(self)

    def forward(self, disp, mask_feat_4, stem_2x):
        if not _train_mode(self):
            for c in (self.spx_2_gru.conv1, self.spx_2_gru.conv2):
                if c.use_bn and c.bn.training:
                    raise _lib.DiffuVolumeError("BatchNorm2d in training mode under no_grad: the inference plans fold "
                                                "running statistics (model.eval())")
            _dev_f32(mask_feat_4, "mask_feat_4")
            self.refresh_plans()
        return _upsample_disp(self, disp, mask_feat_4, stem_2x, None, "train")

    def init_forward(self, features_left0, stem_2x, init_disp):
        if _train_mode(self):
            _upsample_train_entry(("features_left[0]", features_left0), ("stem_2x", stem_2x), ("init_disp", init_disp))
            # (the modules' own forwards take the inference kernels for inputs that ask for no gradient, which would leave
            # these weights without one under a frozen backbone; and MIOpen's backward-weights of these layers does not
            # return the same bits twice, so the convolutions go through train2d like the per-iteration ones)
            spx_pred = _spx_init_train(self, features_left0, stem_2x)
        else:
            spx_pred = self.spx(self.spx_2(self.spx_4(features_left0), stem_2x))
        return context_upsample(init_disp, spx_pred, scale=4.0, apply_softmax=True).unsqueeze(1)


class ResidualBlock(nn.Module):
    """core/extractor.py:10-74 with norm_fn='batch' (what MultiBasicEncoder is built with, :143).  `downsample`
    holds `norm3` a second time, so both key sets exist in the state_dict, as in the reference."""

    def __init__(self, in_planes, planes, norm_fn="batch", stride=1):
        super().__init__()
        if norm_fn != "batch":
            raise _lib.DiffuVolumeError("the context encoder is built with norm_fn='batch'")
        self.conv1 = nn.Conv2d(in_planes, planes, kernel_size=3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        self.norm1, self.norm2 = nn.BatchNorm2d(planes), nn.BatchNorm2d(planes)
        self.downsample = None
        if not (stride == 1 and in_planes == planes):
            self.norm3 = nn.BatchNorm2d(planes)
            self.downsample = nn.Sequential(nn.Conv2d(in_planes, planes, kernel_size=1, stride=stride), self.norm3)

    def forward(self, x):
        if _wants_autograd(x):
            y = self.relu(self.norm1(self.conv1(x)))
            y = self.relu(self.norm2(self.conv2(y)))
            if self.downsample is not None:
                x = self.downsample(x)
            return self.relu(x + y)
        y = hip_conv2d(self.conv1, x, self.norm1, ACT_RELU)
        y = hip_conv2d(self.conv2, y, self.norm2, ACT_RELU)
        if self.downsample is not None:
            x = hip_conv2d(self.downsample[0], x, self.downsample[1], ACT_NONE)
        return torch.relu_(y.add_(x))


class MultiBasicEncoder(nn.Module):
    """core/extractor.py:190-295: the context encoder (`cnet`).  2-D, once per pair: PyTorch."""

    def __init__(self, output_dim=((128, 128, 128),), norm_fn="batch", dropout=0.0, downsample=3):
        super().__init__()
        self.norm_fn, self.downsample = norm_fn, downsample
        self.norm1 = nn.BatchNorm2d(64)
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=1 + (downsample > 2), padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        self.in_planes = 64
        self.layer1 = self._make_layer(64, stride=1)
        self.layer2 = self._make_layer(96, stride=1 + (downsample > 1))
        self.layer3 = self._make_layer(128, stride=1 + (downsample > 0))
        self.layer4 = self._make_layer(128, stride=2)
        self.layer5 = self._make_layer(128, stride=2)
        self.outputs04 = nn.ModuleList([nn.Sequential(ResidualBlock(128, 128, norm_fn, 1), nn.Conv2d(128, d[2], 3, padding=1))
                                        for d in output_dim])
        self.outputs08 = nn.ModuleList([nn.Sequential(ResidualBlock(128, 128, norm_fn, 1), nn.Conv2d(128, d[1], 3, padding=1))
                                        for d in output_dim])
        self.outputs16 = nn.ModuleList([nn.Conv2d(128, d[0], 3, padding=1) for d in output_dim])
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, dim, stride=1):
        layers = (ResidualBlock(self.in_planes, dim, self.norm_fn, stride=stride), ResidualBlock(dim, dim, self.norm_fn, 1))
        self.in_planes = dim
        return nn.Sequential(*layers)

    def forward(self, x, dual_inp=False, num_layers=3):
        hip = not _wants_autograd(x)
        head = (lambda f, t: hip_sequential(f, t)) if hip else (lambda f, t: f(t))
        stem = hip_conv2d(self.conv1, x, self.norm1, ACT_RELU) if hip else self.relu1(self.norm1(self.conv1(x)))
        x = self.layer3(self.layer2(self.layer1(stem)))
        v = None
        if dual_inp:
            v, x = x, x[:(x.shape[0] // 2)]
        tail = (v,) if dual_inp else ()
        outs = ([head(f, x) for f in self.outputs04],)
        if num_layers >= 2:
            y = self.layer4(x)
            outs += ([head(f, y) for f in self.outputs08],)
        if num_layers >= 3:
            z = self.layer5(y)
            outs += ([head(f, z) for f in self.outputs16],)
        return outs + tail


class Feature(nn.Module):
    """core/extractor.py:327-361.  The reference takes its stem and blocks from
    ``timm.create_model('mobilenetv2_100', pretrained=True, features_only=True)``; neither timm nor the weights
    exist offline, so the backbone object is injected: anything with ``conv_stem``, ``bn1``, ``act1`` and ``blocks``
    (7 stages with 16/24/32/64/96/160/320 output channels) -- a timm MobileNetV2 or ``synth.StubMobileNetV2``."""

    def __init__(self, backbone):
        super().__init__()
        chans = [16, 24, 32, 96, 160]
        cut = [1, 2, 3, 5, 6]
        self.conv_stem, self.bn1, self.act1 = backbone.conv_stem, backbone.bn1, backbone.act1
        blocks = list(backbone.blocks)
        self.block0 = nn.Sequential(*blocks[0:cut[0]])
        self.block1 = nn.Sequential(*blocks[cut[0]:cut[1]])
        self.block2 = nn.Sequential(*blocks[cut[1]:cut[2]])
        self.block3 = nn.Sequential(*blocks[cut[2]:cut[3]])
        self.block4 = nn.Sequential(*blocks[cut[3]:cut[4]])
        self.deconv32_16 = Conv2x_IN(chans[4], chans[3], deconv=True, concat=True)
        self.deconv16_8 = Conv2x_IN(chans[3] * 2, chans[2], deconv=True, concat=True)
        self.deconv8_4 = Conv2x_IN(chans[2] * 2, chans[1], deconv=True, concat=True)
        self.conv4 = BasicConv_IN(chans[1] * 2, chans[1] * 2, kernel_size=3, stride=1, padding=1)

    def _backbone_on_hip(self) -> bool:
        def plain(m):
            if isinstance(m, nn.Sequential):
                return all(plain(c) for c in m)
            if isinstance(m, nn.Conv2d):
                k = m.kernel_size[0]
                return (m.groups == 1 and m.dilation == (1, 1) and m.kernel_size == (k, k) and k in (1, 3)
                        and m.padding == (k // 2, k // 2) and m.stride[0] in (1, 2) and m.stride[0] == m.stride[1])
            return isinstance(m, (nn.BatchNorm2d, nn.ReLU, nn.ReLU6, nn.Identity))
        return all(plain(m) for m in (self.conv_stem, self.bn1, self.act1, self.block0, self.block1, self.block2,
                                      self.block3, self.block4))

    def forward(self, x):
        if self._backbone_on_hip() and not _wants_autograd(x):
            # a backbone made of plain [Conv2d, BatchNorm2d, ReLU / ReLU6] stages (synth.StubMobileNetV2) runs on the
            # in-tree kernels; anything else (timm's MobileNetV2: depth-wise / squeeze-excite blocks) is the injected
            # module's own business
            x2 = hip_sequential(self.block0, hip_sequential([self.conv_stem, self.bn1, self.act1], x))
            x4 = hip_sequential(self.block1, x2)
            x8 = hip_sequential(self.block2, x4)
            x16 = hip_sequential(self.block3, x8)
            x32 = hip_sequential(self.block4, x16)
        else:
            x2 = self.block0(self.act1(self.bn1(self.conv_stem(x))))
            x4 = self.block1(x2)
            x8 = self.block2(x4)
            x16 = self.block3(x8)
            x32 = self.block4(x16)
        x16 = self.deconv32_16(x32, x16)
        x8 = self.deconv16_8(x16, x8)
        x4 = self.conv4(self.deconv8_4(x8, x4))
        return [x4, x8, x16, x32]


# ---------------------------------------------------------------------------------------------------
# The 2-D front: everything IGEVStereo_ddim.forward computes before the cost volume and the GRU loop (:364-377 feature
# pyramid, stems, matching features; :395-398 context encoder and the GRU's context terms).  `_front2d` is the inference
# route (what `_front` has always run); `_front2d_train` walks the same modules on the differentiable HIP route:
# convolutions through train2d.conv2d_any / conv_transpose2d_module, InstanceNorm + activation through
# train2d.instance_norm_act, BatchNorm2d the module's own call (frozen by `freeze_bn()` an affine map whose weight and bias
# still train; in train mode batch statistics), ReLU6 / tanh / relu PyTorch.  The modules' own forwards are not used for
# training: they take the inference kernels whenever the input asks for no gradient -- images never do --, which leaves
# these weights without one, and their autograd fallback is MIOpen, whose backward-weights does not return the same bits
# twice.
# ---------------------------------------------------------------------------------------------------
def _front2d(m, image1, image2, n_gru_layers):
    """:364-377 + :395-398 on the modules of ``m`` (an IGEVFront2d or the IGEVStereo_ddim itself), inference kernels ->
    (features_left, stem_2x, match_left, match_right, net_list, inp_list)."""
    image1 = (2 * (image1 / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2 / 255.0) - 1.0).contiguous()
    features_left, features_right = m.feature(image1), m.feature(image2)
    stem_2x = hip_sequential(m.stem_2, image1)
    stem_4x = hip_sequential(m.stem_4, stem_2x)
    stem_4y = hip_sequential(m.stem_4, hip_sequential(m.stem_2, image2))
    features_left[0] = torch.cat((features_left[0], stem_4x), 1)
    features_right[0] = torch.cat((features_right[0], stem_4y), 1)
    match_left = hip_conv2d(m.desc, m.conv(features_left[0])).contiguous()
    match_right = hip_conv2d(m.desc, m.conv(features_right[0])).contiguous()
    cnet_list = m.cnet(image1, num_layers=n_gru_layers)
    net_list = [torch.tanh(x[0]) for x in cnet_list]
    inp_list = [torch.relu(x[1]) for x in cnet_list]
    inp_list = [list(hip_conv2d(conv, i).split(split_size=conv.out_channels // 3, dim=1))
                for i, conv in zip(inp_list, m.context_zqr_convs)]
    inp_list = [[t.contiguous() for t in trio] for trio in inp_list]
    return features_left, stem_2x, match_left, match_right, net_list, inp_list


def _norm_act_train(mods, j, x):
    """The [BatchNorm2d | InstanceNorm2d][ReLU | ReLU6 | LeakyReLU] members that follow a convolution at ``mods[j]`` ->
    (x, index of the first member not consumed)."""
    inorm = None
    if j < len(mods) and isinstance(mods[j], nn.BatchNorm2d):
        x, j = mods[j](x), j + 1
    elif j < len(mods) and isinstance(mods[j], nn.InstanceNorm2d):
        inorm, j = mods[j], j + 1
        if inorm.affine or inorm.track_running_stats:
            raise _lib.DiffuVolumeError("InstanceNorm2d on the HIP front: affine=False, no running statistics")
    a = mods[j] if j < len(mods) and isinstance(mods[j], (nn.ReLU, nn.ReLU6, nn.LeakyReLU)) else None
    if isinstance(a, nn.LeakyReLU) and abs(a.negative_slope - 0.01) > 1e-12:
        raise _lib.DiffuVolumeError("LeakyReLU on the HIP front: negative_slope 0.01")
    if inorm is not None:                                      # ReLU / LeakyReLU fused into the norm's launch, ReLU6 after it
        fused = ACT_NONE if a is None or isinstance(a, nn.ReLU6) else (ACT_LEAKY if isinstance(a, nn.LeakyReLU) else ACT_RELU)
        x = train2d.instance_norm_act(x, fused, inorm.eps)
        if isinstance(a, nn.ReLU6):
            x = F.relu6(x)
    elif a is not None:
        x = F.relu6(x) if isinstance(a, nn.ReLU6) else (F.leaky_relu(x, 0.01) if isinstance(a, nn.LeakyReLU) else F.relu(x))
    return x, j + (a is not None)


def _basic_in_front_train(m, x):
    """A 2-D BasicConv_IN of the front on the training route: convolution, InstanceNorm + LeakyReLU one launch each way."""
    x = train2d.conv_transpose2d_module(m.conv, x) if isinstance(m.conv, nn.ConvTranspose2d) else train2d.conv2d_any(m.conv, x)
    if m.use_in:
        return train2d.instance_norm_act(x, ACT_LEAKY if m.relu else ACT_NONE, m.IN.eps)
    return F.leaky_relu(x, 0.01) if m.relu else x


def _residual_train(m, x):
    """ResidualBlock.forward (core/extractor.py:46-56) on the training route."""
    y = F.relu(m.norm1(train2d.conv2d_any(m.conv1, x)))
    y = F.relu(m.norm2(train2d.conv2d_any(m.conv2, y)))
    if m.downsample is not None:
        x = m.downsample[1](train2d.conv2d_any(m.downsample[0], x))
    return F.relu(x + y)


def _conv2x_in_train(m, x, rem):
    """Conv2x_IN.forward (core/submodule.py:133-150) on the training route."""
    x = _basic_in_front_train(m.conv1, x)
    if x.shape != rem.shape:
        x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="nearest")
    x = torch.cat((x, rem), 1) if m.concat else x + rem
    return _basic_in_front_train(m.conv2, x)


def train_sequential(seq, x: torch.Tensor) -> torch.Tensor:
    """`hip_sequential`'s walk on the training route: [conv][BatchNorm2d | InstanceNorm2d][ReLU | ReLU6 | LeakyReLU(0.01)]
    groups, nested nn.Sequential, ResidualBlock and BasicConv_IN.  A member without a training route raises."""
    mods = list(seq) if isinstance(seq, (nn.Sequential, list, tuple)) else [seq]
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ConvTranspose2d):
            x, i = _norm_act_train(mods, i + 1, train2d.conv_transpose2d_module(m, x))
        elif isinstance(m, nn.Conv2d):
            x, i = _norm_act_train(mods, i + 1, train2d.conv2d_any(m, x))
        elif isinstance(m, nn.Sequential):
            x, i = train_sequential(m, x), i + 1
        elif isinstance(m, ResidualBlock):
            x, i = _residual_train(m, x), i + 1
        elif isinstance(m, BasicConv_IN):
            x, i = _basic_in_front_train(m, x), i + 1
        elif isinstance(m, (nn.Identity, nn.Dropout, nn.Dropout2d)):
            x, i = m(x), i + 1
        else:
            raise _lib.DiffuVolumeError(f"the 2-D front has no training route for {type(m).__name__}")
    return x


def _feature_train(m, x):
    """Feature.forward (core/extractor.py:337-361) on the training route.  A backbone that is not made of plain
    [Conv2d, BatchNorm2d, ReLU / ReLU6] stages (timm's MobileNetV2), or a feature module of another class, is called as
    is: the injected module's own business."""
    if not isinstance(m, Feature):
        return m(x)
    if m._backbone_on_hip():
        x2 = train_sequential(m.block0, train_sequential([m.conv_stem, m.bn1, m.act1], x))
        x4 = train_sequential(m.block1, x2)
        x8 = train_sequential(m.block2, x4)
        x16 = train_sequential(m.block3, x8)
        x32 = train_sequential(m.block4, x16)
    else:
        x2 = m.block0(m.act1(m.bn1(m.conv_stem(x))))
        x4 = m.block1(x2)
        x8 = m.block2(x4)
        x16 = m.block3(x8)
        x32 = m.block4(x16)
    x16 = _conv2x_in_train(m.deconv32_16, x32, x16)
    x8 = _conv2x_in_train(m.deconv16_8, x16, x8)
    x4 = _basic_in_front_train(m.conv4, _conv2x_in_train(m.deconv8_4, x8, x4))
    return [x4, x8, x16, x32]


def _cnet_train(m, x, num_layers):
    """MultiBasicEncoder.forward (core/extractor.py:258-295, dual_inp=False) on the training route."""
    if not isinstance(m, MultiBasicEncoder):
        return m(x, num_layers=num_layers)
    x = F.relu(m.norm1(train2d.conv2d_any(m.conv1, x)))
    x = train_sequential([m.layer1, m.layer2, m.layer3], x)
    outs = ([train_sequential(f, x) for f in m.outputs04],)
    if num_layers >= 2:
        y = train_sequential(m.layer4, x)
        outs += ([train_sequential(f, y) for f in m.outputs08],)
    if num_layers >= 3:
        z = train_sequential(m.layer5, y)
        outs += ([train_sequential(f, z) for f in m.outputs16],)
    return outs


def _front2d_train(m, image1, image2, n_gru_layers):
    """`_front2d` on the training route (train mode with autograd recording)."""
    for name, t in (("image1", image1), ("image2", image2)):
        if not t.is_cuda:
            raise _lib.DiffuVolumeError(f"{name} is on {t.device}: training runs on the MI355X (no CPU fallback)")
    if torch.is_autocast_enabled("cuda"):
        raise _lib.DiffuVolumeError("the 2-D front trains in float32: fp16 / bf16 autocast is not supported in train mode "
                                    "(mixed-precision training is not implemented)")
    image1 = (2 * (image1.float() / 255.0) - 1.0).contiguous()
    image2 = (2 * (image2.float() / 255.0) - 1.0).contiguous()
    features_left, features_right = _feature_train(m.feature, image1), _feature_train(m.feature, image2)
    stem_2x = train_sequential(m.stem_2, image1)
    stem_4x = train_sequential(m.stem_4, stem_2x)
    stem_4y = train_sequential(m.stem_4, train_sequential(m.stem_2, image2))
    features_left[0] = torch.cat((features_left[0], stem_4x), 1)
    features_right[0] = torch.cat((features_right[0], stem_4y), 1)
    match_left = train2d.conv2d_any(m.desc, _basic_in_front_train(m.conv, features_left[0])).contiguous()
    match_right = train2d.conv2d_any(m.desc, _basic_in_front_train(m.conv, features_right[0])).contiguous()
    cnet_list = _cnet_train(m.cnet, image1, n_gru_layers)
    net_list = [torch.tanh(x[0]) for x in cnet_list]
    inp_list = [torch.relu(x[1]) for x in cnet_list]
    inp_list = [list(train2d.conv2d_any(conv, i).split(split_size=conv.out_channels // 3, dim=1))
                for i, conv in zip(inp_list, m.context_zqr_convs)]
    inp_list = [[t.contiguous() for t in trio] for trio in inp_list]
    return features_left, stem_2x, match_left, match_right, net_list, inp_list


class IGEVFront2d(PlanCache, nn.Module):
    """The 2-D front's modules of IGEVStereo_ddim (:180-194 `feature`, `stem_2`, `stem_4`, `conv`, `desc`; :163-170 `cnet`,
    `context_zqr_convs`) under the reference's attribute names, and the parts of its forward that use them (:364-377,
    :395-398).  ``forward(image1, image2)`` (images in 0..255) returns ``(features_left, stem_2x, match_left, match_right,
    net_list, inp_list)``.  In eval mode (or under no_grad) it runs the inference kernels, the bits of
    IGEVStereo_ddim's own front; in train mode with autograd recording every layer is differentiable on the HIP kernels
    (see ``_front2d_train``).  ``feature``: ``Feature(backbone)``, as for IGEVStereo_ddim."""

    def __init__(self, args, feature: nn.Module, cnet: Optional[nn.Module] = None):
        super().__init__()
        self.args = args
        hidden = list(args.hidden_dims)
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hidden, hidden], norm_fn="batch",
                                                                    downsample=args.n_downsample)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hidden[i], hidden[i] * 3, 3, padding=1)
                                                for i in range(args.n_gru_layers)])
        self.feature = feature
        self.stem_2, self.stem_4 = _stem(3, 32), _stem(32, 48)
        self.conv = BasicConv_IN(96, 96, kernel_size=3, padding=1, stride=1)
        self.desc = nn.Conv2d(96, 96, kernel_size=1, padding=0, stride=1)

    def _build_plans(self, slot):
        return {}                   # the front's inference plans live per layer (`hip_conv2d`), training builds them per call

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    def forward(self, image1, image2):
        run = _front2d_train if _train_mode(self) else _front2d
        return run(self, image1, image2, self.args.n_gru_layers)


def _stem(cin, cout):
    return nn.Sequential(BasicConv_IN(cin, cout, kernel_size=3, stride=2, padding=1),
                         nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.InstanceNorm2d(cout), nn.ReLU())


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
                    "importable here -- pass feature=Feature(backbone) (a timm model or synth.StubMobileNetV2())")
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
        betas = cosine_beta_schedule(self.num_timesteps)
        alphas = 1.0 - betas
        ac = torch.cumprod(alphas, dim=0)
        ac_prev = F.pad(ac[:-1], (1, 0), value=1.0)
        post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
        for name, val in (("betas", betas), ("alphas_cumprod", ac), ("alphas_cumprod_prev", ac_prev),
                          ("sqrt_alphas_cumprod", torch.sqrt(ac)),
                          ("sqrt_one_minus_alphas_cumprod", torch.sqrt(1.0 - ac)),
                          ("log_one_minus_alphas_cumprod", torch.log(1.0 - ac)),
                          ("sqrt_recip_alphas_cumprod", torch.sqrt(1.0 / ac)),
                          ("sqrt_recipm1_alphas_cumprod", torch.sqrt(1.0 / ac - 1)),
                          ("posterior_variance", post_var),
                          ("posterior_log_variance_clipped", torch.log(post_var.clamp(min=1e-20))),
                          ("posterior_mean_coef1", betas * torch.sqrt(ac_prev) / (1.0 - ac)),
                          ("posterior_mean_coef2", (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac))):
            self.register_buffer(name, val)

        from .update import BasicMultiUpdateBlock
        hidden = list(args.hidden_dims)
        self.cnet = cnet if cnet is not None else MultiBasicEncoder(output_dim=[hidden, hidden], norm_fn="batch",
                                                                    downsample=args.n_downsample)
        self.update_block = BasicMultiUpdateBlock(args, hidden_dims=hidden)
        self.context_zqr_convs = nn.ModuleList([nn.Conv2d(hidden[i], hidden[i] * 3, 3, padding=1)
                                                for i in range(args.n_gru_layers)])
        self.time_embedding = DynamicHead180(180)
        self.feature = feature

        def stem(cin, cout):
            return nn.Sequential(BasicConv_IN(cin, cout, kernel_size=3, stride=2, padding=1),
                                 nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.InstanceNorm2d(cout), nn.ReLU())

        self.stem_2, self.stem_4 = stem(3, 32), stem(32, 48)
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

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

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
        b, h, w = dq.shape[0], dq.shape[-2], dq.shape[-1]
        x = torch.empty((b, 48, h, w), dtype=torch.float32, device=dq.device)
        with torch.cuda.device(dq.device):
            _lib.check(_lib.load().dv_encode_two_hot_f32(dq.data_ptr(), x.data_ptr(), b, 48, h * w, _lib.stream_ptr()),
                       "dv_encode_two_hot_f32")
        return x

    def _front(self, image1, image2):
        """:364-400 up to the GRU inputs: feature pyramid + stems, matching features, cost volume + initial disparity,
        context encoder, geometry lookup object.  Shared with the origin network (igev_stereo.py:151-194)."""
        features_left, stem_2x, match_left, match_right, net_list, inp_list = _front2d(self, image1, image2,
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
        stage runs on its differentiable HIP route: the 2-D front (``_front2d_train``), the cost volume, the spx heads, the
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
        and ``args.mixed_precision=True`` alone does not select it: both raise and point here."""
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
            self.update_block.set_train_precision("f16")
            try:
                return self._forward_train(image1, image2, flow_gt, iters, flow_init, test_mode, t, noise)
            finally:
                self.update_block.set_train_precision(before)
        return self._forward_train(image1, image2, flow_gt, iters, flow_init, test_mode, t, noise)

    def _forward_train(self, image1, image2, flow_gt, iters, flow_init, test_mode, t, noise):
        if flow_init is not None:
            raise _lib.DiffuVolumeError("flow_init: the reference's train branch does not read it (:441-457)")
        for name, ten in (("image1", image1), ("image2", image2), ("flow_gt", flow_gt)):
            if not ten.is_cuda:
                raise _lib.DiffuVolumeError(f"{name} is on {ten.device}: training runs on the MI355X (no CPU fallback)")
        n_layers = self.args.n_gru_layers
        features_left, stem_2x, match_left, match_right, net_list, inp_list = _front2d_train(self, image1, image2, n_layers)
        if self.update_block.train_precision == "f16":
            # as the inference loop under mixed_precision: the reference's front hands the block fp16 tensors (their
            # gradients pass through the same cast: rounded to fp16, Inf beyond its range -- what GradScaler watches)
            net_list, inp_list = round_gru_inputs_f16(net_list, inp_list)
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
