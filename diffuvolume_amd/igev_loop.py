"""IGEV-Stereo + DiffuVolume: the DDIM volume-filter loop (KITTI15/core/igev_stereo_ddim.py:226-359).

The time embedding with its 180 -> 48 channel interpolation (core/head.py:74-83), ``model_predictions`` (noise filter ->
`iters` GRU iterations each looking the filtered geometry volume up -> two-hot re-encoding -> noise prediction) and
``ddim_sample`` (renewal mask dif<5, output rule dif<3, fresh q_sample fill, ensemble [0.6,0.1,0.3]).  The noise filter
and the DDIM state update are HIP kernels; the geometry lookup (``corr_fn``), the ConvGRU update block and the convex
upsampling are handed in as callables (``update_block`` / ``upsample_disp``), exactly as the reference method calls them:
IGEVStereo_ddim binds its own, a test may bind an oracle's.  Batch handling: the reference head is batch-1 only
(SURVEY A.4.6); here the shift is taken per sample.
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Sequence

import torch
import torch.nn.functional as F
from torch import nn

from . import ddim
from .head import SinusoidalPositionEmbeddings
from .submodule import _dev_f32


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


def round_gru_inputs_bf16(net_list, inp_list):
    """The bf16 twin of ``round_gru_inputs_f16`` for ``forward_train(amp=torch.bfloat16)``: values rounded to bfloat16 (kept
    as float32), and through the same casts their gradients."""
    r = lambda t: t.bfloat16().float() if isinstance(t, torch.Tensor) else t
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
        # the loop holds no module: the schedule as constructed, not a checkpoint's `alphas_cumprod` buffer (ddim.Tables)
        self.tables = ddim.Tables(torch.cumprod(1.0 - ddim.cosine_beta_schedule(1000), dim=0))

    def _time_pairs(self):
        return ddim.time_pairs(self.num_timesteps, self.sampling_timesteps)

    def _filter(self, x_t, t):
        return ddim.noise_prepare(self.time_embedding, x_t, t)

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
        # renewal mask dif < 5 without an uncertainty test; clamp(pred, 0, 48-1) :265; output rule dif < 3 :323-327
        return ddim.step_coef(self.tables, time, time_next, cof, eta=self.eta, dif_thr=5.0, unc_thr=float("inf"),
                              clamp_max=47.0, ens_dif_thr=3.0)

    def _update(self, pred, used, coords0, n01, eps, fill, mask, ens, coef, want_pred_noise=False):
        return ddim.ddim_update(pred, used, n01, eps, fill, mask, ens, coef, coords0=coords0,
                                want_pred_noise=want_pred_noise)

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
        draw = ddim.make_draw(noise, generator, dev)
        img = draw("x_T", tuple(asd.shape), torch.float32)
        mask = torch.zeros((b, h, w), dtype=torch.float32, device=dev)
        ens = used2 * self.ensemble_cof[0]
        for i, (time, time_next) in enumerate(self._time_pairs()):
            eps = fill = None
            if time_next >= 0:
                eps = draw("eps", tuple(img.shape), img.dtype)
                fill = self.tables.q_fill(time, asd, draw("q", tuple(asd.shape), asd.dtype)).contiguous()
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
