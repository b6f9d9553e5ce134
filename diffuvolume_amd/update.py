"""IGEV's recurrent update block (KITTI15/core/update.py) behind the reference's module API: same classes, same
parameter names (a reference ``update_block`` state_dict loads unchanged), same ``forward`` signature and return
convention, so ``IGEVDiffusionLoop`` (or the reference's own ``ddim_sample``) can call it in place.

On HIP (csrc/conv2d.hip): every 3x3 / 1x1 convolution with its bias and ReLU / sigmoid / tanh, and the ConvGRU gate
arithmetic in the epilogues -- ``convr`` emits ``r*h`` directly, ``convq`` emits ``(1-z)*h + z*tanh(.)`` -- so a
ConvGRU is three launches; the convolutions read ``[h | x...]`` as a virtual concatenation (``dv_conv2d_cat_f32``).  The 7x7 single-channel ``convd1``, the 3x3 average
pooling and the bilinear interpolation between the three scales have their own small kernels (csrc/update_glue.hip); PyTorch
writes the disparity channel into the motion features' 128th channel (the reference's ``torch.cat``).

Under fp16 autocast (``torch.autocast("cuda", dtype=torch.float16)``: what the reference's
``autocast(enabled=args.mixed_precision)`` around the update block turns on, igev_stereo_ddim.py:242-246) every module here
runs its fp16 plans instead (csrc/conv2d_f16.hip, ``Conv2dF16Plan``; ``convd1`` on ``dv_conv2d_1in_f16``) with the rounding
points of the reference's fp16 tensors: convolution operands and outputs, and every elementwise result of the fused
epilogues, are rounded to fp16.  Storage stays float32 (fp16-exact values); fp16 input tensors are converted to float32
on entry.  The motion features' channel 127 carries the float32 ``disp`` unrounded, as the reference's
``torch.cat([out, disp])`` promotes to float32 under autocast (update.py:94).  bf16 autocast is refused.

Training (``module.train()`` with gradients enabled): ``BasicMultiUpdateBlock.forward`` takes the differentiable route of
``train2d`` -- the same forward kernels with ReLU / sigmoid / tanh fused, one ``train2d.ConvGRUFn`` per ConvGRU (gate
arithmetic and its backward on csrc/gru_gates.hip's elementwise kernels), weight gradients on
``dv_conv2d_wgrad_cat_f32`` over the virtual concatenations, input gradients on the forward kernels with flipped weights
packed once per weight key (the ``plans("train")`` slot).  ``convd1`` (7x7, one input channel) runs through autograd
there (``train2d.Conv1InFn``) so that it learns although ``disp`` is detached; ``pool2x`` / ``interp`` keep their
autograd dispatch.  ``DV_TRAIN_CONV2D=torch`` sends the convolutions and the gate arithmetic to torch expressions.
Train mode under ``torch.no_grad()`` runs the inference kernels.

Train precision: float32 by default, and then fp16 / bf16 autocast raises in train mode.
``BasicMultiUpdateBlock.set_train_precision("f16")`` (what ``IGEVStereo_ddim.forward_train(amp=True)`` sets for the call)
is the reference's ``--mixed_precision`` training (train_stereo.py:146-173): the block and its five child modules take
their ``plans("train16")`` slot -- forward and input gradients on the fp16 plans above with the reference's rounding
points (the training forward has the bits of the eval forward under fp16 autocast), weight gradients on
``dv_conv2d_wgrad_cat_f16`` (fp16 operands, fp32 accumulation; dW is kept as the unrounded float32 sum where the
reference rounds it to fp16), the gate backward in float32 on the fp16-exact saved values.  The kernels do the rounding,
so the precision holds with or without a caller's fp16 autocast; fp16 inputs are converted to float32 once on entry,
all outputs and gradients are float32, bf16 autocast is refused.  Under ``DV_TRAIN_CONV2D=torch`` that precision runs the
torch expressions under a real ``torch.autocast("cuda", dtype=torch.float16)``.

``set_train_precision(torch.bfloat16)`` (what ``forward_train(amp=torch.bfloat16)`` sets for the call; ``train_precision``
then reads "bf16") is the same route on the bf16 matrix instruction: the ``plans("trainbf16")`` slot, the same kernel bodies
instantiated for bfloat16 (csrc/conv2d_bf16.hip, csrc/conv2d_wgrad_cat_bf16.hip, csrc/gru_gates_bf16.hip,
``dv_conv2d_1in_bf16``; include/diffuvolume_hip_amp2d_bf16.h) with the rounding points above, rb16 in place of r16 -- what
``torch.autocast("cuda", dtype=torch.bfloat16)`` does to the block, apart from the unrounded dW and the float32 gate
backward.  The range is float32's: no ``GradScaler``, no skipped step.  At "bf16" a caller's bf16 autocast is accepted,
bf16 inputs are converted to float32 once on entry, and fp16 autocast raises.  The method takes "f32", "f16",
``torch.float32``, ``torch.float16`` and ``torch.bfloat16``; the bare string "bf16" raises ValueError, as on the 3-D models.
Eval under bf16 autocast stays refused: the reference has no such inference mode.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from .plans import ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, Conv2dF16Plan, Conv2dPairPlan, Conv2dPlan, PlanCache


def autocast_f16() -> bool:
    """True when the caller runs under fp16 autocast on the GPU (the reference's ``autocast(enabled=mixed_precision)``):
    the update block then computes with the fp16 rounding points.  bf16 autocast raises: the reference has no such
    mode and computing fp32 instead would be silent."""
    if not torch.is_autocast_enabled("cuda"):
        return False
    dt = torch.get_autocast_dtype("cuda")
    if dt != torch.float16:
        raise _lib.DiffuVolumeError(f"the IGEV update block supports fp16 autocast only (mixed_precision), got {dt}")
    return True


class _Planned(PlanCache, nn.Module):
    """Two plan slots (submodule.PlanCache): the fp32 plans (``plans()``) and the fp16-autocast ones (``plans("f16")``),
    each built lazily by the module's ``_build`` / ``_build16``, and the training route's (``plans("train")``,
    ``_build_train``: forward plans plus the packed weights of the input gradients; ``plans("train16")``: their fp16
    twins, taken when the module's train precision is "f16"; ``plans("trainbf16")``: the bf16 twins, at "bf16")."""

    _train_precision = "f32"

    def _build_plans(self, slot):
        if slot in _TRAIN_SLOTS.values():
            return self._build_train(**_SLOT_ARGS[slot])
        return self._build16() if slot == "f16" else self._build()

    def set_train_precision(self, precision):
        """"f32" (default: train mode refuses autocast) or "f16" (mixed-precision training on the fp16 kernels, with or
        without a caller's fp16 autocast) for this module and every module of the block below it -- each is a training
        entry of its own.  Also ``torch.float32``, ``torch.float16`` and ``torch.bfloat16``, named as ``torch.autocast``
        names them; ``train_precision`` then reads "f32", "f16" or "bf16".  ``torch.bfloat16`` is THE spelling of bf16 (the
        same route on the bf16 kernels, no ``GradScaler``): the bare string "bf16" raises ValueError, as do "fp16", None,
        16 and any other dtype -- the rule of the 3-D models (``train3d.TrainPrecision``)."""
        from .train3d import _MODEL_PRECISIONS
        if isinstance(precision, bool) or not isinstance(precision, (str, torch.dtype)) or precision not in _MODEL_PRECISIONS:
            raise ValueError('train precision must be "f32", "f16", torch.float32, torch.float16 or torch.bfloat16, '
                             f"got {precision!r}")
        for m in self.modules():
            if isinstance(m, _Planned):
                m._train_precision = _MODEL_PRECISIONS[precision]
        return self

    @property
    def train_precision(self) -> str:
        return self._train_precision


# train precision -> its plan slot, and what ``_build_train`` gets for the slot
_TRAIN_SLOTS = {"f32": "train", "f16": "train16", "bf16": "trainbf16"}
_SLOT_ARGS = {"train": {}, "train16": {"f16": True}, "trainbf16": {"elem": "bf16"}}


def _plan(conv: nn.Conv2d, act: int) -> Conv2dPlan:
    return Conv2dPlan(conv.weight, None, dilation=1, act=act, bias=conv.bias)


def _plan16(conv: nn.Conv2d, act: int) -> Conv2dF16Plan:
    return Conv2dF16Plan(conv.weight, conv.bias, act=act)


def _f32(t):
    """fp16 / bf16 tensors an autocast caller hands over, as float32 (once, on entry)."""
    return t.float() if isinstance(t, torch.Tensor) and t.dtype in (torch.float16, torch.bfloat16) else t


class DispHead(_Planned):
    """update.py:15-24."""

    def __init__(self, input_dim=128, hidden_dim=256, output_dim=1):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, output_dim, 3, padding=1)

    def _build(self):
        return _plan(self.conv1, ACT_RELU), _plan(self.conv2, ACT_NONE)

    def _build16(self):
        return _plan16(self.conv1, ACT_RELU), _plan16(self.conv2, ACT_NONE)

    def _build_train(self, f16=False, elem=None):
        from .train2d import TrainConvPlan
        return TrainConvPlan(self.conv1, ACT_RELU, f16, elem), TrainConvPlan(self.conv2, ACT_NONE, f16, elem)

    def forward(self, x):
        if _training(self):
            from .train2d import conv_cat
            e, slot = _train_entry(self)
            return conv_cat(lambda: self.plans(slot)[1], self.conv2, ACT_NONE,
                            conv_cat(lambda: self.plans(slot)[0], self.conv1, ACT_RELU, _f32(x) if e else x, elem=e), elem=e)
        c1, c2 = self.plans("f16") if autocast_f16() else self.plans()
        return c2(c1(_f32(x)))


class ConvGRU(_Planned):
    """update.py:26-40: z, r gates and candidate q from 3x3 convolutions of [h, x]; cz / cr / cq are the
    per-pair context terms added before the non-linearity."""

    def __init__(self, hidden_dim, input_dim, kernel_size=3):
        super().__init__()
        if kernel_size != 3:
            raise ValueError("ConvGRU is built with 3x3 convolutions in the reference")
        self.convz = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convr = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)
        self.convq = nn.Conv2d(hidden_dim + input_dim, hidden_dim, kernel_size, padding=kernel_size // 2)

    def _build(self):
        # convz and convr read the same [h | x]: one launch with 2 * hidden output channels
        return (Conv2dPairPlan((self.convz.weight, self.convz.bias), (self.convr.weight, self.convr.bias), ACT_SIGMOID),
                _plan(self.convq, ACT_TANH))

    def _build16(self):
        return (Conv2dF16Plan(self.convz.weight, self.convz.bias, ACT_SIGMOID, pair=(self.convr.weight, self.convr.bias)),
                _plan16(self.convq, ACT_TANH))

    def _build_train(self, f16=False, elem=None):
        from .train2d import GRUTrainPlan
        return GRUTrainPlan(self, f16, elem)

    def forward(self, h, cz, cr, cq, *x_list):
        if _training(self):
            from .train2d import conv_gru
            e, slot = _train_entry(self)
            if e:
                h, cz, cr, cq = _f32(h), _f32(cz), _f32(cr), _f32(cq)
                x_list = tuple(_f32(t) for t in x_list)
            return conv_gru(lambda: self.plans(slot), self, h, cz, cr, cq, *x_list, elem=e)
        if autocast_f16():
            # (the fp16 plans round z, r*h and the blend (1-z)*h + z*q at the reference's points; see csrc/conv2d_f16.hip)
            pzr, pq = self.plans("f16")
            h, cz, cr, cq = _f32(h), _f32(cz), _f32(cr), _f32(cq)
            x_list = tuple(_f32(t) for t in x_list)
        else:
            pzr, pq = self.plans()
        if len(x_list) > 3:                             # the kernel takes four sources: [h | x1 | x2 | x3]
            x_list = (torch.cat(x_list[:-2], dim=1),) + tuple(x_list[-2:])
        hx = [h, *x_list]                               # torch.cat([h, x]) is never materialised
        # z = sigmoid(convz(hx) + cz),  rh = sigmoid(convr(hx) + cr) * h
        z, rh = pzr(hx, residual=(cz, cr), mul=(None, h))
        return pq([rh, *x_list], residual=cq, blend=(z, h))                 # (1-z)*h + z*tanh(convq(.) + cq)


class BasicMotionEncoder(_Planned):
    """update.py:74-94."""

    def __init__(self, args):
        super().__init__()
        self.args = args
        cor_planes = args.corr_levels * (2 * args.corr_radius + 1) * (8 + 1)
        self.convc1 = nn.Conv2d(cor_planes, 64, 1, padding=0)
        self.convc2 = nn.Conv2d(64, 64, 3, padding=1)
        self.convd1 = nn.Conv2d(1, 64, 7, padding=3)
        self.convd2 = nn.Conv2d(64, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 64, 128 - 1, 3, padding=1)

    def _build(self):
        p = {n: _plan(getattr(self, n), ACT_RELU) for n in ("convc1", "convc2", "convd2")}
        # convc1 fused into the geometry lookup that feeds it (csrc/geo_lookup.hip), when the caller hands over the lookup
        # as a request instead of a tensor (this build's IGEVDiffusionLoop does)
        p["convc1_lookup"] = None
        if self.convc1.out_channels == 64 and self.convc1.in_channels == 162:
            from .geometry_ddim import pack_lookup_conv1x1
            p["convc1_lookup"] = (pack_lookup_conv1x1(self.convc1.weight, 8),
                                  None if self.convc1.bias is None else self.convc1.bias.detach().float().contiguous())
        # `conv` with one all-zero output channel appended: the launch writes the [B,128,h,w] tensor the reference builds with
        # torch.cat([out, disp]) (update.py:94) and channel 127 (relu(0) = 0) is then overwritten with the disparity.  gru04
        # reads ONE 128-channel source instead of 127 + 1, so every source of its virtual concatenation is a whole number of
        # the kernel's 8-channel chunks (csrc/conv2d_wino.hip, SRC = 1: the source queue moves once per chunk).
        w, b = self.conv.weight, self.conv.bias
        p["conv"] = Conv2dPlan(torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))]), None, dilation=1, act=ACT_RELU,
                               bias=torch.cat([b, b.new_zeros(1)]))
        return p

    def _build16(self):
        p = {n: _plan16(getattr(self, n), ACT_RELU) for n in ("convc1", "convc2", "convd2")}
        w, b = self.conv.weight, self.conv.bias        # (the appended zero channel: see _build)
        p["conv"] = Conv2dF16Plan(torch.cat([w, w.new_zeros((1,) + tuple(w.shape[1:]))]),
                                  torch.cat([b, b.new_zeros(1)]), act=ACT_RELU)
        return p

    def _build_train(self, f16=False, elem=None):
        from .train2d import TrainConvPlan
        return {n: TrainConvPlan(getattr(self, n), ACT_RELU, f16, elem) for n in ("convc1", "convc2", "convd2", "conv")}

    def forward(self, disp, corr):
        return self.features(disp, corr)                # update.py:94 (the reference's return value)

    def _features_train(self, disp, corr):
        """features() on the differentiable route: the real [127, 128, 3, 3] weight of `conv` (no padded channel, nothing
        written in place into a saved tensor) and the reference's torch.cat([out, disp]); convd1 through autograd
        (train2d.Conv1InFn: the inference kernel and a small fixed-order weight-gradient kernel), so that its weight and
        bias learn although `disp` is detached."""
        from .geometry_ddim import GeoLookupRequest
        from .train2d import conv_1in_relu, conv_cat
        e, slot = _train_entry(self)
        p = lambda n: (lambda: self.plans(slot)[n])
        if isinstance(corr, GeoLookupRequest):
            corr = corr.materialize()              # the fused lookup + 1x1 is inference-only
        if e:
            disp, corr = _f32(disp), _f32(corr)
        cor = conv_cat(p("convc2"), self.convc2, ACT_RELU, conv_cat(p("convc1"), self.convc1, ACT_RELU, corr, elem=e), elem=e)
        disp_ = conv_cat(p("convd2"), self.convd2, ACT_RELU, conv_1in_relu(self.convd1, disp, elem=e), elem=e)
        out = conv_cat(p("conv"), self.conv, ACT_RELU, [cor, disp_], elem=e)
        return torch.cat([out, disp], dim=1)       # (channel 127: the float32 disp, unrounded, as under autocast)

    def features(self, disp, corr):
        """The motion features [B,128,h,w] = [conv output (127) | disp (1)], update.py:88-94."""
        if _training(self):
            return self._features_train(disp, corr)
        if autocast_f16():
            return self._features16(_f32(disp), _f32(corr))
        p = self.plans()
        from .geometry_ddim import GeoLookupRequest
        if isinstance(corr, GeoLookupRequest):
            if p["convc1_lookup"] is not None and corr.volume.channel == 8:
                cor = corr.conv1x1(p["convc1_lookup"][0], p["convc1_lookup"][1], ACT_RELU)
            else:
                cor = p["convc1"](corr.materialize())
        else:
            cor = p["convc1"](corr)
        cor = p["convc2"](cor)
        disp_ = p["convd2"](self._convd1(disp))
        out = p["conv"]([cor, disp_])                   # virtual concatenation: torch.cat([cor, disp_]) is never materialised
        out[:, -1:].copy_(disp)
        return out

    def _features16(self, disp, corr):
        """features() under fp16 autocast: convc1 on the materialised lookup (the fused lookup + 1x1 of geo_lookup.hip
        is the fp32 path's), every convolution on its fp16 plan; channel 127 = the float32 disp, unrounded."""
        p = self.plans("f16")
        from .geometry_ddim import GeoLookupRequest
        if isinstance(corr, GeoLookupRequest):
            corr = corr.materialize()
        cor = p["convc2"](p["convc1"](corr))
        disp_ = p["convd2"](self._convd1(disp, f16=True))
        out = p["conv"]([cor, disp_])
        out[:, -1:].copy_(disp)
        return out

    def _convd1(self, disp, f16=False):
        """relu(convd1(disp)): the 7x7 single-input-channel convolution on its own VALU kernel (MIOpen picks a naive
        solver for this shape: 0.7 ms per call at batch 4)."""
        if not _hip_ok(disp, "convd1"):
            return F.relu(self.convd1(disp))                 # autograd dispatch (training graphs only)
        disp = disp.contiguous()
        b, _, h, w = disp.shape
        out = torch.empty((b, self.convd1.out_channels, h, w), dtype=torch.float32, device=disp.device)
        wt, bias = self.convd1.weight.contiguous(), self.convd1.bias
        _lib.launch("dv_conv2d_1in_f16" if f16 else "dv_conv2d_1in_f32", disp.device, disp.data_ptr(), wt.data_ptr(),
                    _lib.ptr(bias), out.data_ptr(), b, h, w, out.shape[1], int(wt.shape[-1]), ACT_RELU)
        return out


def _training(m) -> bool:
    """The differentiable route: train mode AND gradients enabled (train mode under no_grad runs the inference kernels:
    the block has no layer that behaves differently in training)."""
    return m.training and torch.is_grad_enabled()


def _train_entry(m):
    """Every module of the block is a training entry of its own (ConvGRU, DispHead, BasicMotionEncoder called directly):
    its train precision decides the route -- "f32" refuses autocast, "f16" takes the fp16 plans with or without the
    caller's fp16 autocast (bf16 raises), "bf16" takes the bf16 plans with or without the caller's bf16 autocast (fp16
    raises) -- and the packed weights follow the weight key, so an optimizer step since the last call drops them here.
    Returns (the 16-bit element type "f16" / "bf16" or None, the plan slot)."""
    precision = m._train_precision
    if precision == "f16":
        autocast_f16()                      # (raises on bf16)
    elif precision == "bf16":
        if torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") != torch.bfloat16:
            raise _lib.DiffuVolumeError("the update block at train precision 'bf16' takes a caller's bf16 autocast only, got "
                                        f"{torch.get_autocast_dtype('cuda')}")
    else:
        _no_autocast()
    m.refresh_plans()
    return (None if precision == "f32" else precision), _TRAIN_SLOTS[precision]


def _no_autocast():
    if torch.is_autocast_enabled("cuda"):
        raise _lib.DiffuVolumeError("the update block trains in float32 at its default train precision: fp16 / bf16 "
                                    "autocast is not supported in train mode (mixed-precision training: "
                                    "set_train_precision('f16') / set_train_precision(torch.bfloat16), or "
                                    "IGEVStereo_ddim.forward_train(amp=True) / (amp=torch.bfloat16))")


def _hip_ok(x, what):
    """True: the HIP kernel runs.  False: the caller asked for gradients (grad enabled AND the tensor requires grad), the
    one case that is dispatched to the differentiable torch expression -- explicitly, like submodule.py's builders.
    Anything else (a CPU tensor, another dtype) RAISES: there is no silent eager / CPU fallback on the product path."""
    if torch.is_grad_enabled() and x.requires_grad:
        return False
    if not x.is_cuda:
        raise _lib.DiffuVolumeError(f"{what}: input is on {x.device}; the DiffuVolume hot path only runs on the MI355X "
                                    "(HIP kernels, no CPU fallback)")
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: input must be float32, got {x.dtype}")
    return True


def pool2x(x):
    """update.py:96-97.  HIP (`dv_avg_pool3s2_f32`); the torch expression only when gradients are asked for."""
    if not _hip_ok(x, "pool2x"):
        return F.avg_pool2d(x, 3, stride=2, padding=1)     # autograd dispatch
    x = x.contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1), dtype=torch.float32, device=x.device)
    _lib.launch("dv_avg_pool3s2_f32", x.device, x.data_ptr(), out.data_ptr(), b * c, h, w)
    return out


def pool4x(x):
    return F.avg_pool2d(x, 5, stride=4, padding=1)


def interp(x, dest):
    """update.py:100-102.  HIP (`dv_resize_bilinear_ac_f32`); the torch expression only when gradients are asked for."""
    if not _hip_ok(x, "interp"):
        return F.interpolate(x, dest.shape[2:], mode="bilinear", align_corners=True)     # autograd dispatch
    x = x.contiguous()
    b, c, h, w = x.shape
    H, W = int(dest.shape[2]), int(dest.shape[3])
    out = torch.empty((b, c, H, W), dtype=torch.float32, device=x.device)
    _lib.launch("dv_resize_bilinear_ac_f32", x.device, x.data_ptr(), out.data_ptr(), b * c, h, w, H, W)
    return out


class BasicMultiUpdateBlock(_Planned):
    """update.py:104-142."""

    def __init__(self, args, hidden_dims=()):
        super().__init__()
        self.args = args
        self.encoder = BasicMotionEncoder(args)
        encoder_output_dim = 128
        self.gru04 = ConvGRU(hidden_dims[2], encoder_output_dim + hidden_dims[1] * (args.n_gru_layers > 1))
        self.gru08 = ConvGRU(hidden_dims[1], hidden_dims[0] * (args.n_gru_layers == 3) + hidden_dims[2])
        self.gru16 = ConvGRU(hidden_dims[0], hidden_dims[1])
        self.disp_head = DispHead(hidden_dims[2], hidden_dim=256, output_dim=1)
        self.mask_feat_4 = nn.Sequential(nn.Conv2d(hidden_dims[2], 32, 3, padding=1), nn.ReLU(inplace=True))

    def _build(self):
        return _plan(self.mask_feat_4[0], ACT_RELU)

    def _build16(self):
        return _plan16(self.mask_feat_4[0], ACT_RELU)

    def _build_train(self, f16=False, elem=None):
        from .train2d import TrainConvPlan
        return TrainConvPlan(self.mask_feat_4[0], ACT_RELU, f16, elem)

    def _forward_train(self, net, inp, corr, disp, iter04, iter08, iter16, update, mask):
        """The reference's forward (update.py:121-142) on the differentiable route, one stream.  The plans of the whole
        block follow the weight key: an optimizer step between two calls drops them here."""
        from .train2d import conv_cat
        e, slot = _train_entry(self)
        if e:                     # an autocast caller's fp16 / bf16 tensors: float32 once, here (the list objects are kept)
            for i in range(len(net)):
                net[i] = _f32(net[i])
            inp = [[_f32(t) for t in level] for level in inp]
            corr, disp = _f32(corr), _f32(disp)
        for t in (*net, *(t for level in inp for t in level), disp):
            if isinstance(t, torch.Tensor):
                _lib.check_f32(t, "update block input")
        if isinstance(corr, torch.Tensor):
            _lib.check_f32(corr, "corr")
        if iter16:
            net[2] = self.gru16(net[2], *(inp[2]), pool2x(net[1]))
        if iter08:
            if self.args.n_gru_layers > 2:
                net[1] = self.gru08(net[1], *(inp[1]), pool2x(net[0]), interp(net[2], net[1]))
            else:
                net[1] = self.gru08(net[1], *(inp[1]), pool2x(net[0]))
        if iter04:
            mf = self.encoder(disp, corr)
            if self.args.n_gru_layers > 1:
                net[0] = self.gru04(net[0], *(inp[0]), mf, interp(net[1], net[0]))
            else:
                net[0] = self.gru04(net[0], *(inp[0]), mf)
        if not update:
            return net
        delta_disp = self.disp_head(net[0])
        mask_feat_4 = conv_cat(lambda: self.plans(slot), self.mask_feat_4[0], ACT_RELU, net[0], elem=e) if mask else None
        return net, mask_feat_4, delta_disp

    import os as _os
    OVERLAP = _os.environ.get("DV_IGEV_OVERLAP", "1") != "0"
    _streams = None

    def _side_stream(self, device):
        if self._streams is None:
            object.__setattr__(self, "_streams", {})
        if device not in self._streams:
            self._streams[device] = torch.cuda.Stream(device=device)
        return self._streams[device]

    def forward(self, net, inp, corr=None, disp=None, iter04=True, iter08=True, iter16=True, update=True,
                mask=True):
        """The reference's call (update.py:119-142) plus `mask=False` to skip `mask_feat_4`, which the reference computes
        in every iteration and reads only after the last one (igev_stereo_ddim.py:255-259)."""
        if _training(self):
            return self._forward_train(net, inp, corr, disp, iter04, iter08, iter16, update, mask)
        with torch.no_grad():
            mixed = autocast_f16()
            if mixed:             # an autocast caller's fp16 tensors: float32 once, here (the list objects are kept)
                for i in range(len(net)):
                    net[i] = _f32(net[i])
                inp = [[_f32(t) for t in level] for level in inp]
                corr, disp = _f32(corr), _f32(disp)
            mf = None
            if self.OVERLAP and iter04 and iter08 and corr is not None and disp.is_cuda and \
                    not torch.cuda.is_current_stream_capturing():
                # The motion encoder (lookup + five convolutions) does not depend on gru16 / gru08: it runs on a side stream
                # beside them, filling their ramp-up / tail gaps and the half-empty 1/16-scale launches.  Same kernels on the
                # same inputs: bit-identical.  Round 5, batch 4, 1248x384, 20 x 32 iterations, same box, alternating:
                # 1 806-1 807 ms on one stream, 1 775 ms with the encoder on the side stream (-1.8 %; the same experiment was
                # 3.5 % SLOWER before the lookup was coalesced and the small launches K-split).  Measured and NOT kept: gru16 of
                # the next iteration on the side stream beside gru04 and the disparity head (it only needs net[2] and
                # pool2x(net[1]), final after gru08): 1 786-1 789 ms -- gru04 fills the chip, the extra launches only contend.
                # DV_IGEV_OVERLAP=0 puts everything back on one stream.
                main = torch.cuda.current_stream(disp.device)
                side = self._side_stream(disp.device)
                side.wait_stream(main)
                for t in (disp, *(getattr(corr, n, None) for n in ("disp", "coords", "noisy"))):
                    if isinstance(t, torch.Tensor):
                        t.record_stream(side)                    # (main-stream tensors the side stream reads)
                with torch.cuda.stream(side):
                    mf = self.encoder.features(disp, corr)
                mf.record_stream(main)
            if iter16:
                net[2] = self.gru16(net[2], *(inp[2]), pool2x(net[1]))
            if iter08:
                if self.args.n_gru_layers > 2:
                    net[1] = self.gru08(net[1], *(inp[1]), pool2x(net[0]), interp(net[2], net[1]))
                else:
                    net[1] = self.gru08(net[1], *(inp[1]), pool2x(net[0]))
            if iter04:
                if mf is None:
                    mf = self.encoder.features(disp, corr)           # [h | mf+disp | interp]: three sources, no cat
                else:
                    torch.cuda.current_stream(disp.device).wait_stream(self._side_stream(disp.device))
                if self.args.n_gru_layers > 1:
                    net[0] = self.gru04(net[0], *(inp[0]), mf, interp(net[1], net[0]))
                else:
                    net[0] = self.gru04(net[0], *(inp[0]), mf)
            if not update:
                return net
            delta_disp = self.disp_head(net[0])
            mask_feat_4 = (self.plans("f16") if mixed else self.plans())(net[0]) if mask else None
        return net, mask_feat_4, delta_disp
