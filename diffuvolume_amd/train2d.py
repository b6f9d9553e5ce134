"""Differentiable 2-D convolutions on the HIP kernels (training of PWCNet_ddim's refinement network ``refinenet3``).

``conv2d(x, w, bias=None, dilation=1)`` (k in {1, 3}, stride 1, padding = dilation for k = 3, dilation 1..16) is a
``torch.autograd.Function`` whose three products all run on libdiffuvolume_hip.so:
  * forward: the inference kernels through ``Conv2dPlan`` (no BN folding, no activation; Winograd routing applies);
  * input gradient: the same forward kernels on the output gradient, with the weights repacked on every call
        3x3, dilation d   conv of g with w.flip(2,3).transpose(0,1), dilation d
        1x1               conv of g with w^T
    The kernels pad channel counts internally (to 32 output and 8 input channels), so conv1's input gradient
    (128 -> 146 channels) needs no padding here.  A single-channel output gradient (conv8's, 1 -> 32 channels, 3x3,
    dilation 1) runs on ``dv_conv2d_1in_f32``, the direct kernel for single-channel inputs;
  * weight gradient: ``dv_conv2d_wgrad_f32`` (csrc/conv2d_wgrad.hip); bias gradient ``g.sum((0, 2, 3))``.
BatchNorm and Mish stay PyTorch.  ``DV_TRAIN_CONV2D=torch`` routes the function to ``F.conv2d`` instead (A/B runs,
tests).  CPU tensors raise, as everywhere on the hot path.  ``refinenet3`` uses this route.

IGEV's recurrent update block (``update.BasicMultiUpdateBlock`` in train mode) uses the second half of this module:
``TrainConvPlan`` / ``conv_cat`` (a biased 3x3 / 1x1 convolution over a virtual channel concatenation with its
activation fused), ``GRUTrainPlan`` / ``conv_gru`` (one ``ConvGRUFn`` per ConvGRU call) and ``conv_1in_relu`` (the 7x7
single-input-channel ``convd1``).  Their weight gradients run
on ``dv_conv2d_wgrad_cat_f32`` (csrc/conv2d_wgrad_cat.hip) over the un-materialised concatenation; their input gradients
are ONE forward launch on the output gradient with the flipped / transposed weights, cut into channel views per
source; the flipped weights are packed once per plan (the module's ``plans("train")`` slot, dropped with the weight
key), not per call.  Mixed precision (``BasicMultiUpdateBlock.set_train_precision("f16")``, ``forward_train(amp=True)``):
every plan has an fp16 twin (``f16=True``, the ``plans("train16")`` slot) whose forward and input gradient run on
``Conv2dF16Plan`` (csrc/conv2d_f16.hip: operands and results rounded to fp16, fp32 accumulation on the fp16 MFMA), whose
weight gradient runs on ``dv_conv2d_wgrad_cat_f16`` (csrc/conv2d_wgrad_cat_f16.hip, an unrounded float32 dW) and whose gate
arithmetic rounds like the fp16 epilogues (``dv_gru_reset_mul_f16`` / ``dv_gru_blend_f16``); tensors stay float32 holding
fp16-exact values, bias gradients stay float32 sums.  ``DV_TRAIN_CONV2D=torch`` at that precision runs the torch
expressions under a real ``torch.autocast("cuda", dtype=torch.float16)``.  Train precision "bf16"
(``set_train_precision(torch.bfloat16)``, ``forward_train(amp=torch.bfloat16)``) is the same route with the other element
type: every 16-bit plan and function here takes ``elem="bf16"`` beside the ``f16`` flag (``f16=True`` alone means
``elem="f16"``), the plans live in the ``plans("trainbf16")`` slot and run the bf16 instantiations of the same kernel
bodies (``Conv2dF16Plan(elem="bf16")``, ``dv_conv2d_wgrad_cat_bf16``, ``dv_gru_reset_mul_bf16`` / ``dv_gru_blend_bf16``,
``dv_conv2d_1in_bf16``; include/diffuvolume_hip_amp2d_bf16.h); the torch route runs under a real bf16 autocast.

IGEV's convex-upsampling head (``igev_upsample.IGEVUpsampler`` in train mode) uses the third part:
``conv_transpose2d_k4`` / ``conv_transpose2d_module``, a ConvTranspose2d(kernel 4, stride 2, padding 1) whose forward is
``Deconv2dK4S2Plan``'s (four parity 3x3 convolutions + pixel shuffle), whose input gradient is ONE 3x3 forward launch on
the pixel-unshuffled output gradient with the flipped parity weights (``TrainDeconvPlan``, packed once per plan) and
whose weight gradient is ``dv_deconv2d_k4s2_wgrad_f32`` (csrc/deconv2d_k4_bwd.hip).

IGEV's once-per-pair 2-D front (``igev_front2d.IGEVFront2d`` / ``IGEVStereo_ddim.forward_train``) uses the fourth
part: ``conv2d_s2`` (3x3, stride 2: forward on ``Conv2dPlan(stride=2)``, both gradients on the k4 transposed-convolution
kernels above through an exact identity), ``conv2d_k1s2`` (the 1x1 stride-2 ``downsample``), ``conv2d_fewin`` (the image
convolutions: weight gradient on ``dv_conv2d_fewin_wgrad_f32``, no input gradient), ``instance_norm_act`` (backward on
``dv_instance_norm_act_bwd_f32``, both csrc/igev_front_bwd.hip) and the dispatcher ``conv2d_any``.  Plans are built per
call: these layers run once per pair.

The MobileNetV2 backbone of that front (``mobilenetv2.MobileNetV2Features``) adds ``dwconv2d``, the depthwise 3x3
convolution of its blocks (csrc/dwconv2d.hip, forward and backward).  ``conv2d_any`` keeps refusing grouped
convolutions: a depthwise layer reaches ``dwconv2d`` through the backbone's block classes only."""
from __future__ import annotations

import functools
from typing import Optional

import torch
import torch.nn.functional as F

from . import _env, _lib
from .plans import (ACT_LEAKY, ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH, Conv2dF16Plan, Conv2dPairPlan, Conv2dPlan,
                    Deconv2dK4S2Plan, cat_args)

route = functools.partial(_env.route, "DV_TRAIN_CONV2D")


def conv2d_weight_grad(x: torch.Tensor, g: torch.Tensor, k: int, dilation: int, cout: int) -> torch.Tensor:
    """dW [Cout,Cin,k,k] of a stride-1 convolution (padding = dilation for k = 3) with input ``x`` and output
    gradient ``g``."""
    x, g = x.contiguous(), g.contiguous()
    b, cin, h, w = x.shape
    ws = _lib.workspace("dv_conv2d_wgrad_workspace_floats", x.device, b, cin, h, w, cout, k, dilation)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_conv2d_wgrad_f32 does not take k={k} dilation={dilation}")
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    _lib.launch("dv_conv2d_wgrad_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, h, w,
                cout, k, dilation)
    return dw


def _input_grad(g: torch.Tensor, w: torch.Tensor, dilation: int) -> torch.Tensor:
    k = w.shape[2]
    wt = (w.transpose(0, 1) if k == 1 else w.flip(2, 3).transpose(0, 1)).contiguous()      # [Cin, Cout, k, k]
    if g.shape[1] == 1 and k == 3 and dilation == 1:
        b, _, h, wd = g.shape
        dx = torch.empty((b, wt.shape[0], h, wd), dtype=torch.float32, device=g.device)
        _lib.launch("dv_conv2d_1in_f32", g.device, g.data_ptr(), wt.data_ptr(), 0, dx.data_ptr(), b, h, wd, wt.shape[0], 3,
                    ACT_NONE)
        return dx
    return Conv2dPlan(wt, None, dilation=dilation, act=ACT_NONE)(g)


class Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        k = weight.shape[2]
        if tuple(weight.shape[2:]) != (k, k) or k not in (1, 3) or not 1 <= dilation <= 16:
            raise _lib.DiffuVolumeError(f"unsupported Conv2d: kernel {tuple(weight.shape[2:])}, dilation {dilation}")
        dilation = dilation if k == 3 else 1
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.dilation, ctx.has_bias = dilation, bias is not None
        b = None if bias is None else bias.detach()
        return Conv2dPlan(weight.detach().contiguous(), None, dilation=dilation, act=ACT_NONE, bias=b)(x)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        d, k = ctx.dilation, w.shape[2]
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _input_grad(g, w.detach(), d)
        if ctx.needs_input_grad[1]:
            dw = conv2d_weight_grad(x, g, k, d, w.shape[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3))
        return dx, dw, db, None


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, dilation: int = 1) -> torch.Tensor:
    k = weight.shape[2]
    if route() == "torch":
        return F.conv2d(x, weight, bias, padding=dilation if k == 3 else 0, dilation=dilation if k == 3 else 1)
    return Conv2dFn.apply(x, weight, bias, dilation)


def conv2d_module(m: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """An nn.Conv2d of refinenet3 (stride 1, padding equal to its dilation; 1x1: no padding) on the differentiable HIP
    route."""
    k, d = m.kernel_size[0], m.dilation[0]
    if m.stride != (1, 1) or m.kernel_size != (k, k) or m.padding != ((d, d) if k == 3 else (0, 0)) or m.groups != 1:
        raise _lib.DiffuVolumeError(f"conv2d_module: stride 1 and padding = dilation only, got {m}")
    return conv2d(x, m.weight, m.bias, dilation=d)


# ---- IGEV's update block: convolutions over a virtual concatenation, ConvGRU ----------------------------------------

_ELEM_DTYPE = {"f16": torch.float16, "bf16": torch.bfloat16}


def _elem(f16: bool = False, elem: Optional[str] = None) -> Optional[str]:
    """The 16-bit element type of a plan or call: None (float32), "f16" or "bf16".  ``f16=True`` alone is "f16"; ``elem``
    names the type beside it."""
    if elem is None:
        return "f16" if f16 else None
    if elem not in _ELEM_DTYPE or (f16 and elem != "f16"):
        raise ValueError(f"elem must be 'f16' or 'bf16' (and agree with f16={f16!r}), got {elem!r}")
    return elem


def conv2d_cat_weight_grad(sources, g: torch.Tensor, k: int, f16: bool = False, elem: Optional[str] = None) -> torch.Tensor:
    """dW [Cout, sum(c_i), k, k] of a stride-1, dilation-1 convolution (k 3: padding 1) whose input is the channel
    concatenation of ``sources`` (1..4 tensors, never materialised) and whose output gradient is ``g``.  ``f16``: on
    ``dv_conv2d_wgrad_cat_f16`` (both operands rounded to fp16 while staged, fp32 accumulation on the fp16 MFMA, float32
    result) instead of ``dv_conv2d_wgrad_cat_f32``; ``elem="bf16"``: on ``dv_conv2d_wgrad_cat_bf16``."""
    e = _elem(f16, elem)
    name = f"dv_conv2d_wgrad_cat_{e}" if e else "dv_conv2d_wgrad_cat_f32"
    sources = [t.contiguous() for t in sources]
    g = g.contiguous()
    b, cout, h, w = g.shape
    if not 1 <= len(sources) <= 4 or any(t.shape[0] != b or tuple(t.shape[2:]) != (h, w) for t in sources):
        raise _lib.DiffuVolumeError("conv2d_cat_weight_grad: 1..4 sources with the batch and plane of the gradient")
    for t in (*sources, g):
        _lib.check_f32(t, "conv2d_cat_weight_grad operand")
    ptrs, chans, n = cat_args(sources)
    size = f"dv_conv2d_wgrad_cat_{e}_workspace_floats" if e else "dv_conv2d_wgrad_cat_workspace_floats"
    ws = _lib.workspace(size, g.device, chans, n, b, h, w, cout, k)
    if ws is None:
        raise _lib.DiffuVolumeError(f"{name} does not take k={k}, channels {list(chans)}, Cout {cout}")
    dw = torch.empty((cout, sum(chans), k, k), dtype=torch.float32, device=g.device)
    _lib.launch(name, g.device, ptrs, chans, n, g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, h, w, cout, k)
    return dw


class _InputGradPlan:
    """The input gradient of a stride-1, dilation-1 convolution as a forward launch: the weights flipped and transposed
    ([Cin, Cout, k, k]) and packed ONCE.  ``weights``: one tensor, or several whose outputs are concatenated (ConvGRU's
    z | r pair: the gradient then arrives as one tensor per convolution, read as a virtual concatenation).  A
    single-channel gradient (DispHead.conv2, 256 -> 1) runs on ``dv_conv2d_1in_f32``.  ``f16``: the same launch on
    ``Conv2dF16Plan`` / ``dv_conv2d_1in_f16`` -- gradient and weights rounded to fp16, fp32 accumulation, the input gradient
    rounded to fp16 as the reference's fp16 input gradients are.  ``elem="bf16"``: the bf16 twins."""

    def __init__(self, weights, f16: bool = False, elem: Optional[str] = None):
        e = _elem(f16, elem)
        w = torch.cat([t.detach() for t in weights], dim=0) if len(weights) > 1 else weights[0].detach()
        self.k = int(w.shape[2])
        wt = (w.transpose(0, 1) if self.k == 1 else w.flip(2, 3).transpose(0, 1)).contiguous()
        self.cin = int(wt.shape[0])
        self.one_in = w.shape[0] == 1 and self.k == 3
        self.wt = wt if self.one_in else None
        self.fn1 = f"dv_conv2d_1in_{e}" if e else "dv_conv2d_1in_f32"
        self.plan = None if self.one_in else (Conv2dF16Plan(wt, None, act=ACT_NONE, elem=e) if e else
                                              Conv2dPlan(wt, None, dilation=1, act=ACT_NONE))

    def __call__(self, grads):
        if self.one_in:
            g = grads[0].contiguous()
            b, _, h, wd = g.shape
            dx = torch.empty((b, self.cin, h, wd), dtype=torch.float32, device=g.device)
            _lib.launch(self.fn1, g.device, g.data_ptr(), self.wt.data_ptr(), 0, dx.data_ptr(), b, h, wd, self.cin, 3,
                        ACT_NONE)
            return dx
        return self.plan(list(grads) if len(grads) > 1 else grads[0])


def _split_channels(t: torch.Tensor, sources):
    """Channel views of ``t`` with the channel counts of ``sources``."""
    out, c0 = [], 0
    for s in sources:
        out.append(t[:, c0:c0 + s.shape[1]])
        c0 += s.shape[1]
    return out


def _act_grad(g: torch.Tensor, out: torch.Tensor, act: int) -> torch.Tensor:
    """Gradient before the fused activation, from the activation's saved OUTPUT."""
    if act == ACT_NONE:
        return g.contiguous()
    if act == ACT_RELU:
        return g * (out > 0)
    if act == ACT_SIGMOID:
        return g * out * (1.0 - out)
    if act == ACT_TANH:
        return g * (1.0 - out * out)
    raise _lib.DiffuVolumeError(f"no derivative for activation {act}")


class TrainConvPlan:
    """One nn.Conv2d (3x3 padding 1, or 1x1; stride 1) of the update block for the training route: the forward plan with
    bias and activation fused, and the packed weights of its input gradient.  ``f16``: the mixed-precision twin (the
    module's ``plans("train16")`` slot) -- forward and input gradient on ``Conv2dF16Plan``, the weight gradient on
    ``dv_conv2d_wgrad_cat_f16``.  ``elem="bf16"``: the bf16 twin (``plans("trainbf16")``)."""

    def __init__(self, conv: torch.nn.Conv2d, act: int, f16: bool = False, elem: Optional[str] = None):
        e = _elem(f16, elem)
        k = conv.kernel_size[0]
        if conv.kernel_size != (k, k) or k not in (1, 3) or conv.stride != (1, 1) or conv.dilation != (1, 1) or \
                conv.padding != ((k - 1) // 2,) * 2 or conv.groups != 1:
            raise _lib.DiffuVolumeError(f"TrainConvPlan: 3x3 (padding 1) or 1x1, stride 1, dilation 1 only, got {conv}")
        _lib.check_f32(conv.weight, "weight")
        self.k, self.act, self.cout, self.f16, self.elem = k, act, conv.out_channels, e == "f16", e
        self.fwd = Conv2dF16Plan(conv.weight, conv.bias, act=act, elem=e) if e else \
            Conv2dPlan(conv.weight, None, dilation=1, act=act, bias=conv.bias)
        self.bwd = _InputGradPlan([conv.weight], elem=e)


class ConvCatFn(torch.autograd.Function):
    """act(conv(cat(sources)) + bias) on the HIP kernels, all three gradients on the HIP kernels."""

    @staticmethod
    def forward(ctx, plan, weight, bias, *sources):
        for t in sources:
            _lib.check_f32(t, "source")
        sources = [t.contiguous() for t in sources]
        out = plan.fwd(sources if len(sources) > 1 else sources[0])
        ctx.plan = plan
        ctx.save_for_backward(out, *sources)
        return out

    @staticmethod
    def backward(ctx, g):
        out, *sources = ctx.saved_tensors
        plan = ctx.plan
        gp = _act_grad(g, out, plan.act)
        dw = db = None
        if ctx.needs_input_grad[1]:
            # (DispHead.conv2, 256 -> 1, idles 63 of the tile's 64 rows; measured at batch 4, 80x184: 0.205 ms here against
            # 0.261 ms on dv_conv2d_wgrad_f32, so it stays on this kernel: a 1 x 2304 reduction is not worth a route)
            dw = conv2d_cat_weight_grad(sources, gp, plan.k, elem=plan.elem)
        if ctx.needs_input_grad[2]:
            db = gp.sum(dim=(0, 2, 3))
        dsrc = [None] * len(sources)
        if any(ctx.needs_input_grad[3:]):
            dx = plan.bwd([gp])
            dsrc = [v if need else None for v, need in zip(_split_channels(dx, sources), ctx.needs_input_grad[3:])]
        return (None, dw, db, *dsrc)


class Conv1InFn(torch.autograd.Function):
    """relu(conv(x) + bias) of a single-input-channel k x k convolution (BasicMotionEncoder.convd1, 7x7): forward on
    ``dv_conv2d_1in_f32`` (the inference kernel), weight gradient on ``dv_conv2d_1in_wgrad_f32`` (fixed summation order:
    MIOpen's backward-weights of this shape does not return the same bits twice).  The input gradient -- the reference
    always detaches ``disp`` -- is a 64 -> 1 convolution left to PyTorch.  ``f16``: the forward on ``dv_conv2d_1in_f16``;
    the weight gradient stays on the float32 kernel, fed the fp16-rounded ``disp`` (one channel by 49 taps is not an MFMA
    shape).  ``elem="bf16"``: the forward on ``dv_conv2d_1in_bf16``, the weight gradient fed the bf16-rounded ``disp``."""

    @staticmethod
    def forward(ctx, x, weight, bias, f16=False, elem=None):
        e = _elem(f16, elem)
        _lib.check_f32(x, "disp")
        _lib.check_f32(weight, "weight")
        x, wt = x.contiguous(), weight.detach().contiguous()
        b, cin, h, w = x.shape
        k = int(wt.shape[-1])
        if cin != 1 or wt.shape[1] != 1 or k != 7:
            raise _lib.DiffuVolumeError(f"Conv1InFn: one input channel, k = 7, got {tuple(wt.shape)}")
        out = torch.empty((b, wt.shape[0], h, w), dtype=torch.float32, device=x.device)
        fn = f"dv_conv2d_1in_{e}" if e else "dv_conv2d_1in_f32"
        _lib.launch(fn, x.device, x.data_ptr(), wt.data_ptr(), _lib.ptr(bias), out.data_ptr(), b, h, w, out.shape[1], k,
                    ACT_RELU)
        ctx.save_for_backward(x.to(_ELEM_DTYPE[e]).float() if e else x, weight, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, out = ctx.saved_tensors
        gp = _act_grad(g, out, ACT_RELU)
        b, _, h, w = x.shape
        k = int(weight.shape[-1])
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            _lib.launch("dv_conv2d_1in_wgrad_f32", x.device, x.data_ptr(), gp.data_ptr(), dw.data_ptr(), b, h, w,
                        weight.shape[0], k)
        if ctx.needs_input_grad[2]:
            db = gp.sum(dim=(0, 2, 3))
        if ctx.needs_input_grad[0]:
            dx = F.conv2d(gp, weight.detach().flip(2, 3).transpose(0, 1), None, padding=k // 2)
        return dx, dw, db, None, None


def _autocast16(fn, elem="f16"):
    """The torch route at "f16" / "bf16" precision: the expression under a real autocast of that dtype, the result as
    float32."""
    with torch.autocast("cuda", dtype=_ELEM_DTYPE[elem]):
        return fn().float()


def conv_1in_relu(conv: torch.nn.Conv2d, x: torch.Tensor, f16: bool = False, elem: Optional[str] = None) -> torch.Tensor:
    """relu(conv(x)) for a single-input-channel layer on the training route."""
    e = _elem(f16, elem)
    if route() == "torch":
        return _autocast16(lambda: F.relu(conv(x)), e) if e else F.relu(conv(x))
    return Conv1InFn.apply(x, conv.weight, conv.bias, e == "f16", e)


def conv_cat(plan, conv: torch.nn.Conv2d, act: int, sources, f16: bool = False, elem: Optional[str] = None) -> torch.Tensor:
    """act(conv(cat(sources))) for the training route of the update block.  ``plan``: a callable that returns the
    layer's TrainConvPlan; it is only called (and the plan only built) on the HIP route.  ``f16``: the module's train
    precision is "f16" (the plan is then its fp16 twin; the torch route runs under a real fp16 autocast); ``elem="bf16"``:
    the same at "bf16"."""
    e = _elem(f16, elem)
    sources = list(sources) if isinstance(sources, (list, tuple)) else [sources]
    if route() == "torch":
        def expr():
            x = torch.cat(sources, dim=1) if len(sources) > 1 else sources[0]
            y = F.conv2d(x, conv.weight, conv.bias, padding=(conv.kernel_size[0] - 1) // 2)
            return {ACT_NONE: lambda t: t, ACT_RELU: F.relu, ACT_SIGMOID: torch.sigmoid, ACT_TANH: torch.tanh}[act](y)
        return _autocast16(expr, e) if e else expr()
    p = plan()
    assert p.act == act and p.elem == e
    return ConvCatFn.apply(p, conv.weight, conv.bias, *sources)


def _gates(fn: str, *args) -> None:
    _lib.launch(fn, args[0].device, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


class GRUTrainPlan:
    """A ConvGRU for the training route: the z | r pair launch (sigmoid fused, no ``mul``), the candidate's plan (tanh
    fused, no blend) and the packed weights of the two input gradients.  ``f16``: the mixed-precision twin on
    ``Conv2dF16Plan`` (the z | r pair without ``mul``, the candidate without ``blend``); ``elem="bf16"``: the bf16 twin."""

    def __init__(self, gru, f16: bool = False, elem: Optional[str] = None):
        e = _elem(f16, elem)
        for c in (gru.convz, gru.convr, gru.convq):
            _lib.check_f32(c.weight, "weight")
        self.hidden, self.f16, self.elem = gru.convz.out_channels, e == "f16", e
        if e:
            self.zr = Conv2dF16Plan(gru.convz.weight, gru.convz.bias, ACT_SIGMOID, pair=(gru.convr.weight, gru.convr.bias),
                                    elem=e)
            self.q = Conv2dF16Plan(gru.convq.weight, gru.convq.bias, ACT_TANH, elem=e)
        else:
            self.zr = Conv2dPairPlan((gru.convz.weight, gru.convz.bias), (gru.convr.weight, gru.convr.bias), ACT_SIGMOID)
            self.q = Conv2dPlan(gru.convq.weight, None, dilation=1, act=ACT_TANH, bias=gru.convq.bias)
        self.zr_bwd = _InputGradPlan([gru.convz.weight, gru.convr.weight], elem=e)
        self.q_bwd = _InputGradPlan([gru.convq.weight], elem=e)
        self.mul, self.blend = f"dv_gru_reset_mul_{e or 'f32'}", f"dv_gru_blend_{e or 'f32'}"


class ConvGRUFn(torch.autograd.Function):
    """One ConvGRU call (update.py:33-40).  Saved for the backward: h, the x sources, z, r, q -- no concatenation, no
    r*h, no 1-z or z*q.  Inputs: plan, six parameters, h, cz, cr, cq, then the x sources.  The precision is the plan's:
    with an fp16 plan the gate kernels round like conv2d_f16.hip's epilogues (the eval forward's bits under fp16
    autocast), the gate backward stays float32 arithmetic on the fp16-exact saved values (the convolutions that consume
    its outputs round their operands anyway) and the weight gradients run on ``dv_conv2d_wgrad_cat_f16``; a bf16 plan is the
    same with the bf16 entries."""

    @staticmethod
    def forward(ctx, plan, wz, bz, wr, br, wq, bq, h, cz, cr, cq, *xs):
        for t in (h, cz, cr, cq, *xs):
            _lib.check_f32(t, "ConvGRU input")
        h, cz, cr, cq = (t.contiguous() for t in (h, cz, cr, cq))
        xs = [t.contiguous() for t in xs]
        z, r = plan.zr([h, *xs], residual=(cz, cr), mul=(None, None))
        rh = torch.empty_like(h)
        _gates(plan.mul, r, h, rh, h.numel())
        q = plan.q([rh, *xs], residual=cq)
        out = torch.empty_like(h)
        _gates(plan.blend, z, q, h, out, h.numel())
        ctx.plan = plan
        ctx.save_for_backward(h, z, r, q, *xs)
        return out

    @staticmethod
    def backward(ctx, g):
        h, z, r, q, *xs = ctx.saved_tensors
        plan = ctx.plan
        need = ctx.needs_input_grad
        g = g.contiguous()
        n = h.numel()
        dq, dz, dh = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)
        _gates("dv_gru_gates_bwd_blend_f32", g, z, q, h, dq, dz, dh, n)
        rh = torch.empty_like(h)
        _gates(plan.mul, r, h, rh, n)                                 # (recomputed: the forward's bits)
        dq_in = plan.q_bwd([dq])                                      # d[rh | x...]
        dr = torch.empty_like(h)
        _gates("dv_gru_gates_bwd_reset_f32", dq_in[:, :plan.hidden].contiguous(), r, h, dr, dh, n)
        dzr_in = plan.zr_bwd([dz, dr])                                # d[h | x...]
        dh += dzr_in[:, :plan.hidden]
        hx = [h, *xs]
        dwz = conv2d_cat_weight_grad(hx, dz, 3, elem=plan.elem) if need[1] else None
        dwr = conv2d_cat_weight_grad(hx, dr, 3, elem=plan.elem) if need[3] else None
        dwq = conv2d_cat_weight_grad([rh, *xs], dq, 3, elem=plan.elem) if need[5] else None
        dbz = dz.sum(dim=(0, 2, 3)) if need[2] else None
        dbr = dr.sum(dim=(0, 2, 3)) if need[4] else None
        dbq = dq.sum(dim=(0, 2, 3)) if need[6] else None
        dxs, c0 = [], plan.hidden
        for t, nd in zip(xs, need[11:]):
            c1 = c0 + t.shape[1]
            dxs.append(dq_in[:, c0:c1] + dzr_in[:, c0:c1] if nd else None)
            c0 = c1
        return (None, dwz, dbz, dwr, dbr, dwq, dbq, dh if need[7] else None, dz if need[8] else None,
                dr if need[9] else None, dq if need[10] else None, *dxs)


def conv_gru(plan, gru, h, cz, cr, cq, *xs, f16: bool = False, elem: Optional[str] = None) -> torch.Tensor:
    """ConvGRU.forward for the training route (the reference's expression under DV_TRAIN_CONV2D=torch; at "f16"
    precision that expression under a real fp16 autocast, on fp16 tensors like the reference's).  ``plan``: a callable
    that returns the GRUTrainPlan, only called on the HIP route.  ``elem="bf16"``: the same at "bf16"."""
    e = _elem(f16, elem)
    if route() == "torch":
        def expr():
            hh, zz, rr, qq = (t.to(_ELEM_DTYPE[e]) for t in (h, cz, cr, cq)) if e else (h, cz, cr, cq)
            x = torch.cat([t.to(_ELEM_DTYPE[e]) for t in xs] if e else xs, dim=1)
            hx = torch.cat([hh, x], dim=1)
            z = torch.sigmoid(gru.convz(hx) + zz)
            r = torch.sigmoid(gru.convr(hx) + rr)
            q = torch.tanh(gru.convq(torch.cat([r * hh, x], dim=1)) + qq)
            return (1 - z) * hh + z * q
        return _autocast16(expr, e) if e else expr()
    if len(xs) > 3:                                     # the kernels take four sources: [h | x1 | x2 | x3]
        xs = (torch.cat(xs[:-2], dim=1),) + tuple(xs[-2:])
    c = gru.convz, gru.convr, gru.convq
    p = plan()
    assert p.elem == e
    return ConvGRUFn.apply(p, c[0].weight, c[0].bias, c[1].weight, c[1].bias, c[2].weight, c[2].bias, h, cz, cr, cq, *xs)


# ---- IGEV's convex-upsampling head: ConvTranspose2d(kernel 4, stride 2, padding 1) -----------------------------------

def deconv2d_k4_weight_grad(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dW [Cin, Cout, 4, 4] of a ConvTranspose2d(4, stride 2, padding 1) with input ``x`` [B,Cin,H,W] and output gradient
    ``g`` [B,Cout,2H,2W]."""
    _lib.check_f32(x, "x")
    _lib.check_f32(g, "output gradient")
    x, g = x.contiguous(), g.contiguous()
    b, cin, h, w = x.shape
    cout = g.shape[1]
    if g.shape[0] != b or tuple(g.shape[2:]) != (2 * h, 2 * w):
        raise _lib.DiffuVolumeError(f"deconv2d_k4_weight_grad: x {tuple(x.shape)} against g {tuple(g.shape)}")
    ws = _lib.workspace("dv_deconv2d_k4s2_wgrad_workspace_floats", x.device, b, cin, h, w, cout)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_deconv2d_k4s2_wgrad_f32 does not take x {tuple(x.shape)}, Cout {cout}")
    dw = torch.empty((cin, cout, 4, 4), dtype=torch.float32, device=x.device)
    _lib.launch("dv_deconv2d_k4s2_wgrad_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, h, w,
                cout)
    return dw


class TrainDeconvPlan:
    """A ConvTranspose2d(4, stride 2, padding 1) [+ bias] for the training route: the forward plan (no BatchNorm, no
    activation) and the packed weights of its input gradient -- the 3x3 convolution of the pixel-unshuffled output gradient
    with the flipped, transposed parity weights."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None):
        _lib.check_f32(weight, "weight")
        if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4):
            raise _lib.DiffuVolumeError(f"TrainDeconvPlan: a [Cin, Cout, 4, 4] weight, got {tuple(weight.shape)}")
        self.cin, self.cout = int(weight.shape[0]), int(weight.shape[1])
        self.fwd = Deconv2dK4S2Plan(weight, None, bias=bias)
        self.bwd = _InputGradPlan([Deconv2dK4S2Plan.parity_weights(weight)])


class ConvTranspose2dK4Fn(torch.autograd.Function):
    """conv_transpose2d(x, weight, bias, stride 2, padding 1) on the HIP kernels, all three gradients too."""

    @staticmethod
    def forward(ctx, plan, x, weight, bias):
        _lib.check_f32(x, "x")
        x = x.contiguous()
        if x.dim() != 4 or x.shape[1] != plan.cin or tuple(weight.shape) != (plan.cin, plan.cout, 4, 4):
            raise _lib.DiffuVolumeError(f"conv_transpose2d_k4: x {tuple(x.shape)} against weight {tuple(weight.shape)}")
        ctx.plan, ctx.has_bias = plan, bias is not None
        ctx.save_for_backward(x)
        return plan.fwd(x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[1]:
            dx = ctx.plan.bwd([F.pixel_unshuffle(g, 2)])
        if ctx.needs_input_grad[2]:
            dw = deconv2d_k4_weight_grad(x, g)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = g.sum(dim=(0, 2, 3))
        return None, dx, dw, db


def conv_transpose2d_k4(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, plan=None) -> torch.Tensor:
    """F.conv_transpose2d(x, weight, bias, stride=2, padding=1) for a [Cin, Cout, 4, 4] weight on the training route.
    ``plan``: a callable that returns the layer's TrainDeconvPlan (a module's ``plans("train")`` slot), only called on the
    HIP route; without one the plan is built for this call."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (4, 4):
        raise _lib.DiffuVolumeError(f"conv_transpose2d_k4: kernel 4 x 4 only, got a weight of {tuple(weight.shape)}")
    if route() == "torch":
        return F.conv_transpose2d(x, weight, bias, stride=2, padding=1)
    return ConvTranspose2dK4Fn.apply(plan() if plan is not None else TrainDeconvPlan(weight, bias), x, weight, bias)


def conv_transpose2d_module(m: torch.nn.ConvTranspose2d, x: torch.Tensor, plan=None) -> torch.Tensor:
    """An nn.ConvTranspose2d (kernel 4, stride 2, padding 1: IGEV's spx heads) on the differentiable HIP route."""
    if not isinstance(m, torch.nn.ConvTranspose2d) or m.kernel_size != (4, 4) or m.stride != (2, 2) or \
            m.padding != (1, 1) or m.output_padding != (0, 0) or m.dilation != (1, 1) or m.groups != 1:
        raise _lib.DiffuVolumeError(f"conv_transpose2d_module: kernel 4, stride 2, padding 1, no output padding, "
                                    f"groups 1 only, got {m}")
    return conv_transpose2d_k4(x, m.weight, m.bias, plan)


# ---- IGEV's once-per-pair 2-D front: stride-2 and few-input-channel convolutions, InstanceNorm + activation -----------

def _embed_k4(w: torch.Tensor) -> torch.Tensor:
    """A [Cout,Cin,3,3] convolution weight as the [in = Cout, out = Cin, 4, 4] weight of the transposed convolution that is
    the stride-2 convolution's adjoint: the 3x3 taps top-left, a zero last row and column."""
    return F.pad(w.detach(), (0, 1, 0, 1)).contiguous()


class Conv2dS2Fn(torch.autograd.Function):
    """conv2d(x, weight, bias, stride 2, padding 1) for a 3x3 kernel.  Forward: ``Conv2dPlan(stride=2)``.  The backward
    needs no kernel of its own: output pixel (i, j) reads input pixel (2i - 1 + ky, 2j - 1 + kx), which is the index map
    of ConvTranspose2d(4, stride 2, padding 1) restricted to ky, kx < 3.  So, with the filter embedded in a 4x4 one,
      * dx = conv_transpose2d_k4(g, w4) cropped to H x W (``Deconv2dK4S2Plan``: [Cout,Cin,3,3] is already its [in,out]
        layout);
      * dw = dv_deconv2d_k4s2_wgrad_f32 with the roles swapped (x := g, g := x zero-padded to 2Ho x 2Wo), [:, :, :3, :3].
    Both are exact (the fourth row / column multiplies zeros or is dropped)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or x.dim() != 4 or x.shape[1] != weight.shape[1]:
            raise _lib.DiffuVolumeError(f"conv2d_s2: x {tuple(x.shape)} against weight {tuple(weight.shape)} (3x3 only)")
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        b = None if bias is None else bias.detach()
        return Conv2dPlan(weight.detach().contiguous(), None, act=ACT_NONE, bias=b, stride=2)(x)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        h, wd = x.shape[2:]
        ho, wo = g.shape[2:]
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = Deconv2dK4S2Plan(_embed_k4(w), None)(g)[:, :, :h, :wd]
        if ctx.needs_input_grad[1]:
            xp = x if (h, wd) == (2 * ho, 2 * wo) else F.pad(x, (0, 2 * wo - wd, 0, 2 * ho - h))    # odd H or W only
            dw = deconv2d_k4_weight_grad(g, xp)[:, :, :3, :3].contiguous()
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3))
        return dx, dw, db


def conv2d_s2(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(x, weight, bias, stride=2, padding=1) for a 3x3 kernel on the training route."""
    if route() == "torch":
        return F.conv2d(x, weight, bias, stride=2, padding=1)
    return Conv2dS2Fn.apply(x, weight, bias)


def conv2d_k1s2(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(x, weight, bias, stride=2) for a 1x1 kernel (the `downsample` of ResidualBlock, core/extractor.py:40-44):
    the stride-1 function on every second row and column."""
    if route() == "torch":
        return F.conv2d(x, weight, bias, stride=2)
    _lib.check_f32(x, "x")
    return Conv2dFn.apply(x[:, :, ::2, ::2].contiguous(), weight, bias, 1)


def conv2d_fewin_weight_grad(x: torch.Tensor, g: torch.Tensor, k: int, stride: int) -> torch.Tensor:
    """dW [Cout,Cin,k,k] of a convolution with <= 4 input channels (k in {3,5,7}, stride in {1,2}, padding k/2) with input
    ``x`` and output gradient ``g``."""
    _lib.check_f32(x, "x")
    _lib.check_f32(g, "output gradient")
    x, g = x.contiguous(), g.contiguous()
    b, cin, h, w = x.shape
    cout = g.shape[1]
    if g.shape[0] != b or tuple(g.shape[2:]) != ((h - 1) // stride + 1, (w - 1) // stride + 1):
        raise _lib.DiffuVolumeError(f"conv2d_fewin_weight_grad: x {tuple(x.shape)} against g {tuple(g.shape)}, stride {stride}")
    ws = _lib.workspace("dv_conv2d_fewin_wgrad_workspace_floats", x.device, b, cin, h, w, cout, k, stride)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_conv2d_fewin_wgrad_f32 does not take Cin={cin} k={k} stride={stride}")
    dw = torch.empty((cout, cin, k, k), dtype=torch.float32, device=x.device)
    _lib.launch("dv_conv2d_fewin_wgrad_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, h, w,
                cout, k, stride)
    return dw


class Conv2dFewInFn(torch.autograd.Function):
    """A convolution of an IMAGE (<= 4 channels; k in {3,5,7}, stride in {1,2}, padding k/2): forward on
    ``dv_conv2d_fewin_f32`` (the inference kernel), weight gradient on ``dv_conv2d_fewin_wgrad_f32``.  Images are data:
    there is no input gradient, and an input that asks for one is refused."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        k = int(weight.shape[-1])
        if x.dim() != 4 or weight.dim() != 4 or x.shape[1] != weight.shape[1] or weight.shape[1] > 4 or \
                tuple(weight.shape[2:]) != (k, k) or k not in (3, 5, 7) or stride not in (1, 2):
            raise _lib.DiffuVolumeError(f"conv2d_fewin: x {tuple(x.shape)}, weight {tuple(weight.shape)}, stride {stride}")
        x, wt = x.contiguous(), weight.detach().contiguous()
        b, cin, h, w = x.shape
        out = torch.empty((b, wt.shape[0], (h - 1) // stride + 1, (w - 1) // stride + 1), dtype=torch.float32, device=x.device)
        _lib.launch("dv_conv2d_fewin_f32", x.device, x.data_ptr(), wt.data_ptr(), _lib.ptr(None if bias is None else bias.detach()),
                    0, 0, out.data_ptr(), b, cin, h, w, wt.shape[0], k, stride, ACT_NONE)
        ctx.save_for_backward(x)
        ctx.k, ctx.stride, ctx.has_bias = k, stride, bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        dw = db = None
        if ctx.needs_input_grad[1]:
            dw = conv2d_fewin_weight_grad(x, g, ctx.k, ctx.stride)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3))
        return None, dw, db, None


def conv2d_fewin(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1) -> torch.Tensor:
    """F.conv2d(x, weight, bias, stride, padding=k//2) of an image (<= 4 channels) on the training route."""
    if x.requires_grad:
        raise _lib.DiffuVolumeError("conv2d_fewin: the input is an image (data); it has no input gradient")
    if route() == "torch":
        return F.conv2d(x, weight, bias, stride=stride, padding=weight.shape[-1] // 2)
    return Conv2dFewInFn.apply(x, weight, bias, stride)


class InstanceNormActFn(torch.autograd.Function):
    """nn.InstanceNorm2d (affine=False) + activation: the forward is the inference launch out of place (its bits), the
    backward ``dv_instance_norm_act_bwd_f32`` on the saved pre-norm tensor."""

    @staticmethod
    def forward(ctx, x, act, eps):
        _lib.check_f32(x, "x")
        x = x.contiguous()
        b, c, h, w = x.shape
        out = torch.empty_like(x)
        _lib.launch("dv_instance_norm_act_f32", x.device, x.data_ptr(), out.data_ptr(), b * c, h * w, float(eps), act)
        ctx.save_for_backward(x)
        ctx.act, ctx.eps = act, float(eps)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()
        b, c, h, w = x.shape
        dx = torch.empty_like(x)
        _lib.launch("dv_instance_norm_act_bwd_f32", x.device, x.data_ptr(), g.data_ptr(), dx.data_ptr(), b * c, h * w, ctx.eps,
                    ctx.act)
        return dx, None, None


def instance_norm_act(x: torch.Tensor, act: int = ACT_NONE, eps: float = 1e-5) -> torch.Tensor:
    """act(F.instance_norm(x, eps=eps)) for act in {ACT_NONE, ACT_RELU, ACT_LEAKY} on the training route."""
    if act not in (ACT_NONE, ACT_RELU, ACT_LEAKY):
        raise _lib.DiffuVolumeError(f"instance_norm_act: none, ReLU or LeakyReLU(0.01) only, got activation {act}")
    if x.dim() != 4:
        raise _lib.DiffuVolumeError(f"instance_norm_act: a [B,C,H,W] tensor, got {tuple(x.shape)}")
    if route() == "torch":
        y = F.instance_norm(x, eps=eps)
        return y if act == ACT_NONE else (F.relu(y) if act == ACT_RELU else F.leaky_relu(y, 0.01))
    return InstanceNormActFn.apply(x, act, eps)


class DepthwiseConv2dFn(torch.autograd.Function):
    """The bare depthwise 3x3 convolution (padding 1, stride 1 / 2, no bias): forward on ``dv_dwconv3x3_f32`` without scale,
    shift or activation, both gradients on ``dv_dwconv3x3_bwd_f32`` (csrc/dwconv2d.hip).  Only ``x`` is kept for the
    backward (beside the weight, which is the parameter itself): the output is not."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        if x.dim() != 4 or tuple(weight.shape) != (x.shape[1], 1, 3, 3) or stride not in (1, 2):
            raise _lib.DiffuVolumeError(f"dwconv2d: x {tuple(x.shape)}, weight {tuple(weight.shape)}, stride {stride}")
        x, wt = x.contiguous(), weight.detach().contiguous()
        b, c, h, w = x.shape
        out = torch.empty((b, c, (h - 1) // stride + 1, (w - 1) // stride + 1), dtype=torch.float32, device=x.device)
        _lib.launch("dv_dwconv3x3_f32", x.device, x.data_ptr(), wt.data_ptr(), 0, 0, out.data_ptr(), b, c, h, w, stride,
                    ACT_NONE, 0.0)
        ctx.save_for_backward(x, weight)
        ctx.stride = stride
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g, wt = g.contiguous(), weight.detach().contiguous()
        b, c, h, w = x.shape
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        dw = ws = None
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(wt)
            ws = _lib.workspace("dv_dwconv3x3_bwd_workspace_floats", x.device, b, c, h, w, ctx.stride)
        if dx is not None or dw is not None:
            _lib.launch("dv_dwconv3x3_bwd_f32", x.device, x.data_ptr(), wt.data_ptr(), g.data_ptr(), _lib.ptr(dx), _lib.ptr(dw),
                        _lib.ptr(ws), b, c, h, w, ctx.stride)
        return dx, dw, None


def dwconv2d(x: torch.Tensor, weight: torch.Tensor, stride: int = 1) -> torch.Tensor:
    """F.conv2d(x, weight, None, stride, padding=1, groups=C) for a depthwise 3x3 ``weight`` [C,1,3,3] on the training
    route."""
    if route() == "torch":
        _lib.check_f32(x, "x")
        return F.conv2d(x, weight, None, stride=stride, padding=1, groups=x.shape[1])
    return DepthwiseConv2dFn.apply(x, weight, stride)


def conv2d_any(m: torch.nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """An nn.Conv2d of IGEV's 2-D front on the differentiable HIP route, picked by its geometry:
      <= 4 input channels, k in {3,5,7}, stride 1 / 2, padding k/2   conv2d_fewin (no input gradient)
      k in {1,3}, stride 1, padding = dilation (k3) / 0 (k1)          conv2d
      k3, stride 2, padding 1                                         conv2d_s2
      k1, stride 2, padding 0                                         conv2d_k1s2
    Anything else raises."""
    if not isinstance(m, torch.nn.Conv2d) or isinstance(m, torch.nn.ConvTranspose2d):
        raise _lib.DiffuVolumeError(f"conv2d_any: an nn.Conv2d, got {type(m).__name__}")
    k, st, d = m.kernel_size[0], m.stride[0], m.dilation[0]
    square = m.kernel_size == (k, k) and m.stride == (st, st) and m.dilation == (d, d) and m.groups == 1 and \
        m.padding_mode == "zeros" and not isinstance(m.padding, str)
    if square and m.in_channels <= 4 and k in (3, 5, 7) and st in (1, 2) and d == 1 and m.padding == (k // 2, k // 2):
        return conv2d_fewin(x, m.weight, m.bias, st)
    if square and st == 1 and k in (1, 3) and m.padding == ((d, d) if k == 3 else (0, 0)):
        return conv2d(x, m.weight, m.bias, dilation=d)
    if square and st == 2 and k == 3 and d == 1 and m.padding == (1, 1):
        return conv2d_s2(x, m.weight, m.bias)
    if square and st == 2 and k == 1 and m.padding == (0, 0):
        return conv2d_k1s2(x, m.weight, m.bias)
    raise _lib.DiffuVolumeError(f"conv2d_any: no training route for {m}")
