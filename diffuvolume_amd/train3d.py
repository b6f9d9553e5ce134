"""Differentiable 3-D convolutions on the HIP kernels (training of ACVNet_DDIM's aggregation stack).

``conv3d(x, w, bias=None, stride=1)`` (cubic k in {1, 3}, pad (k-1)/2, stride 1 | 2) and ``conv_transpose3d(x, w)``
(k3 s2 p1 op1, bias-free) are ``torch.autograd.Function``s whose three products all run on libdiffuvolume_hip.so:
  * forward: the inference kernels through ``Conv3dPlan`` / ``Deconv3dPlan`` (no BN folding, no activation);
  * input gradient: the same forward kernels on the output gradient, with the weights repacked on every call
        stride-1 3x3x3   conv of g with w.flip(2,3,4).transpose(0,1)   (Winograd routing applies)
        stride-2 3x3x3   transposed conv of g with w as is              (dims must be even)
        transposed conv  stride-2 conv of g with w as is                (polyphase / direct)
        1x1x1            conv of g with w^T
    (the kernels pad channel counts internally, so 40 -> 32 layers and the 32 -> 1 head need no padding here);
  * weight gradient: ``dv_conv3d_wgrad_f32`` (csrc/conv3d_wgrad.hip), the transposed form with x and g exchanged.
``conv_transpose3d_k4(x, w)`` (k4 s2 p1, bias-free: the IGEV hourglass's conv3_up / conv2_up / conv1_up) has kernels of
its own for both gradients (csrc/deconv3d_k4_bwd.hip); ``feature_gate_train(cv, logit)`` is FeatureAtt's
``sigmoid(logit) * cv`` with ``dv_feature_gate_bwd_f32`` as its backward.
BatchNorm3d and the activation behind it are ``train_norm.py``'s.  ``DV_TRAIN_CONV3D=torch`` routes every function to its torch expression (``F.conv3d``,
``F.conv_transpose3d``, ``torch.sigmoid(logit).unsqueeze(2) * cv``) instead (A/B runs, tests).  CPU tensors raise, as
everywhere on the hot path.

Train precision ``"f16"`` (``conv3d(..., precision=)``; ``ACVNet_DDIM`` / ``PWCNet_ddim.set_train_precision`` set it for
their ``train_forward`` through ``precision_scope``; default ``"f32"``, where nothing changes): the 3x3x3 stride-1
convolutions with more than one output channel run all three products on the fp16 matrix instruction --
``dv_conv3d_k3s1_f16_f32`` (csrc/conv3d_f16.hip: forward, and with ``transpose_flip`` the input gradient, on the raw
weight, no packed copy) and ``dv_conv3d_wgrad_f16_f32`` (csrc/conv3d_wgrad_f16.hip), include/diffuvolume_hip_amp3d.h:
float32 tensors, operands rounded to fp16 while staged, fp32 sums, no result rounded.  Every other layer class keeps its
float32 kernels.  Under ``DV_TRAIN_CONV3D=torch`` those layers run ``F.conv3d`` under a real fp16 ``torch.autocast``
and return float32 (the reference route of the tests).

Train precision ``"bf16"`` (``set_train_precision(torch.bfloat16)``) is the same route on the bf16 matrix instruction:
``dv_conv3d_k3s1_bf16_f32`` (csrc/conv3d_bf16.hip) and ``dv_conv3d_wgrad_bf16_f32`` (csrc/conv3d_wgrad_bf16.hip),
include/diffuvolume_hip_amp3d_bf16.h -- the kernels of ``"f16"`` (csrc/conv3d_mp.h, csrc/conv3d_wgrad_mp.h) instantiated
for the other element type: operands rounded to bfloat16 while staged, fp32 sums, no result rounded.  bfloat16 has
float32's exponent range, so there is no loss scaling and no skipped step.  Under ``DV_TRAIN_CONV3D=torch`` the layers run
``F.conv3d`` under a real bf16 ``torch.autocast`` and return float32."""
from __future__ import annotations

import contextlib
import contextvars
import functools
from typing import Optional

import torch
import torch.nn.functional as F

from . import _env, _lib
from .submodule import ACT_NONE, Conv3dPlan, Deconv3dPlan, feature_gate


route = functools.partial(_env.route, "DV_TRAIN_CONV3D")

PRECISIONS = ("f32", "f16", "bf16")
# the reduced precisions (each also the infix of its ABI table's entries) -> the dtype torch.autocast names it by
REDUCED = {"f16": torch.float16, "bf16": torch.bfloat16}
# what ``TrainPrecision.set_train_precision`` takes: the two names it has always taken, and the dtypes as torch.autocast
# names them.  "bf16" has no string spelling on the model method: the dtype is its documented one.
_MODEL_PRECISIONS = {"f32": "f32", "f16": "f16", torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}
# The train precision of the model call in progress: ``ACVNet_DDIM.train_forward`` / ``PWCNet_ddim.train_forward`` set it
# for their own call (``precision_scope``), ``conv3d(..., precision=None)`` reads it.  A ContextVar: every thread (two
# replicas training side by side) and every nested call has its own value, and nothing outside a model call ever sees
# anything but "f32".  The backward never reads it -- the autograd engine runs on threads of its own -- but the precision
# ``Conv3dFn.forward`` saved on ``ctx``.
_ambient_precision = contextvars.ContextVar("dv_train3d_precision", default="f32")


def check_precision(precision: str) -> str:
    if precision not in PRECISIONS:
        raise ValueError(f"train precision must be one of {PRECISIONS}, got {precision!r}")
    return precision


@contextlib.contextmanager
def precision_scope(precision: str):
    """Every ``conv3d`` / ``conv3d_module`` call of this thread inside the block that names no precision runs at
    ``precision``."""
    token = _ambient_precision.set(check_precision(precision))
    try:
        yield
    finally:
        _ambient_precision.reset(token)


def ambient_precision() -> str:
    return _ambient_precision.get()


class TrainPrecision:
    """What ``ACVNet_DDIM`` and ``PWCNet_ddim`` add to nn.Module for mixed-precision training (modelled on
    ``update._Planned``): ``set_train_precision("f32" | "f16" | torch.float32 | torch.float16 | torch.bfloat16)``, the
    ``train_precision`` property (``"f32"``, ``"f16"`` or ``"bf16"``), and
    ``_train_scope()``, which their ``train_forward`` runs under.  Eval and ``no_grad`` inference never look at it."""

    _train_precision = "f32"

    def set_train_precision(self, precision):
        """"f32" (default) or "f16": the 3x3x3 stride-1 convolutions of the model's 3-D stack with more than one output
        channel run their three products on the fp16 matrix instruction (operands rounded to fp16, fp32 sums, float32
        results); every other layer keeps its float32 kernels.

        Also ``torch.float32``, ``torch.float16`` and ``torch.bfloat16``, named as ``torch.autocast`` names them;
        ``train_precision`` then reads "f32", "f16" or "bf16".  ``torch.bfloat16`` is THE spelling of bf16 here: the same
        layers on the bf16 matrix instruction (operands rounded to bfloat16), no ``GradScaler`` needed.  The bare string
        "bf16" raises ValueError on this method, as do "fp16", "", None, 16 and any other dtype
        (``train3d.precision_scope("bf16")`` and ``conv3d(..., precision="bf16")`` take the name)."""
        if isinstance(precision, bool) or not isinstance(precision, (str, torch.dtype)) or precision not in _MODEL_PRECISIONS:
            raise ValueError('train precision must be "f32", "f16", torch.float32, torch.float16 or torch.bfloat16, '
                             f"got {precision!r}")
        self._train_precision = _MODEL_PRECISIONS[precision]
        return self

    @property
    def train_precision(self) -> str:
        return self._train_precision

    def _train_scope(self):
        return precision_scope(self._train_precision)


def takes_f16(k: int, stride: int, cout: int) -> bool:
    """The layer class that "f16" / "bf16" move to the fp16 / bf16 matrix instruction; every other one keeps its float32
    kernels."""
    return k == 3 and stride == 1 and cout > 1


def _conv3d_k3s1_mp(elem: str, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], transpose_flip: bool):
    """``dv_conv3d_k3s1_<elem>_f32``, ``elem`` in ("f16", "bf16")."""
    x, w = x.contiguous(), w.contiguous()
    b, cin, d, h, wd = x.shape
    cout = w.shape[1] if transpose_flip else w.shape[0]
    if tuple(w.shape) != ((cin, cout, 3, 3, 3) if transpose_flip else (cout, cin, 3, 3, 3)):
        raise _lib.DiffuVolumeError(f"conv3d {elem}: weight {tuple(w.shape)} against input {tuple(x.shape)}")
    y = torch.empty((b, cout, d, h, wd), dtype=torch.float32, device=x.device)
    _lib.launch(f"dv_conv3d_k3s1_{elem}_f32", x.device, x.data_ptr(), w.data_ptr(),
                _lib.ptr(None if bias is None else bias.contiguous()), y.data_ptr(), b, cin, d, h, wd, cout, 3,
                int(transpose_flip))
    return y


def _conv3d_weight_grad_mp(elem: str, x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``dv_conv3d_wgrad_<elem>_f32``, ``elem`` in ("f16", "bf16")."""
    x, g = x.contiguous(), g.contiguous()
    b, cin, d, h, w = x.shape
    cout = g.shape[1]
    if tuple(g.shape) != (b, cout, d, h, w):
        raise _lib.DiffuVolumeError(f"conv3d {elem} weight gradient: input {tuple(x.shape)} against gradient {tuple(g.shape)}")
    ws = _lib.workspace(f"dv_conv3d_wgrad_{elem}_workspace_floats", x.device, b, cin, d, h, w, cout)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_conv3d_wgrad_{elem}_f32 does not take the shape {tuple(x.shape)} -> {cout} channels")
    dw = torch.empty((cout, cin, 3, 3, 3), dtype=torch.float32, device=x.device)
    _lib.launch(f"dv_conv3d_wgrad_{elem}_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, d,
                h, w, cout)
    return dw


def conv3d_k3s1_f16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                    transpose_flip: bool = False) -> torch.Tensor:
    """conv(r16(x), r16(w)) + bias of a 3x3x3 stride-1 convolution, unrounded float32 (csrc/conv3d_f16.hip).  ``w`` is the
    raw weight [Cout,Cin,3,3,3]; with ``transpose_flip`` it is [Cin,Cout,3,3,3] and read as w.flip(2,3,4).transpose(0,1)
    (the input gradient, ``x`` being the output gradient)."""
    return _conv3d_k3s1_mp("f16", x, w, bias, transpose_flip)


def conv3d_k3s1_bf16(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                     transpose_flip: bool = False) -> torch.Tensor:
    """``conv3d_k3s1_f16`` with both operands rounded to bfloat16 instead (csrc/conv3d_bf16.hip)."""
    return _conv3d_k3s1_mp("bf16", x, w, bias, transpose_flip)


def conv3d_weight_grad_f16(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dW [Cout,Cin,3,3,3] = sum r16(g) r16(x) of a 3x3x3 stride-1 convolution, unrounded float32
    (csrc/conv3d_wgrad_f16.hip)."""
    return _conv3d_weight_grad_mp("f16", x, g)


def conv3d_weight_grad_bf16(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """``conv3d_weight_grad_f16`` with both operands rounded to bfloat16 instead (csrc/conv3d_wgrad_bf16.hip)."""
    return _conv3d_weight_grad_mp("bf16", x, g)


def conv3d_weight_grad(x: torch.Tensor, g: torch.Tensor, k: int, stride: int, cout: int) -> torch.Tensor:
    """dW [Cout,Cin,k,k,k] of a cubic convolution (pad (k-1)/2) with input ``x`` and output gradient ``g``."""
    x, g = x.contiguous(), g.contiguous()
    b, cin, d, h, w = x.shape
    ws = _lib.workspace("dv_conv3d_wgrad_workspace_floats", x.device, b, cin, d, h, w, cout, k, stride)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_conv3d_wgrad_f32 does not take k={k} stride={stride}")
    dw = torch.empty((cout, cin, k, k, k), dtype=torch.float32, device=x.device)
    _lib.launch("dv_conv3d_wgrad_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, cin, d, h, w,
                cout, k, stride)
    return dw


def _plan(w: torch.Tensor, stride: int, bias: Optional[torch.Tensor] = None) -> Conv3dPlan:
    return Conv3dPlan(w.contiguous(), None, stride=stride, act=ACT_NONE, bias=bias, precision="f32")


class Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride, precision="f32"):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        check_precision(precision)
        k = weight.shape[2]
        if tuple(weight.shape[2:]) != (k, k, k) or k not in (1, 3) or stride not in (1, 2) or (k == 1 and stride != 1):
            raise _lib.DiffuVolumeError(f"unsupported Conv3d: kernel {tuple(weight.shape[2:])}, stride {stride}")
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.has_bias = stride, bias is not None
        # the element type of this layer's three products: "f16" | "bf16", or None for the float32 kernels
        ctx.elem = precision if precision in REDUCED and takes_f16(k, stride, weight.shape[0]) else None
        if ctx.elem:
            return _conv3d_k3s1_mp(ctx.elem, x.detach(), weight.detach(), None if bias is None else bias.detach(), False)
        return _plan(weight.detach(), stride, None if bias is None else bias.detach())(x)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        stride, k = ctx.stride, w.shape[2]
        g = g.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # the precision saved by forward, never an ambient value.  A layer with ONE input channel has a one-channel
            # input gradient, which the fp16 and bf16 entries refuse as they do the 32 -> 1 heads: float32 kernel, as at "f32"
            if ctx.elem and w.shape[1] > 1:
                dx = _conv3d_k3s1_mp(ctx.elem, g, w.detach(), None, True)
            elif k == 1:
                dx = _plan(w.detach().transpose(0, 1), 1)(g)
            elif stride == 1:
                dx = _plan(w.detach().flip(2, 3, 4).transpose(0, 1), 1)(g)
            else:
                if any(n % 2 for n in x.shape[2:]):
                    raise _lib.DiffuVolumeError(f"stride-2 input gradient needs even dims, got {tuple(x.shape[2:])}")
                dx = Deconv3dPlan(w.detach().contiguous(), None, act=ACT_NONE)(g)
        if ctx.needs_input_grad[1]:
            dw = _conv3d_weight_grad_mp(ctx.elem, x, g) if ctx.elem else conv3d_weight_grad(x, g, k, stride, w.shape[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = g.sum(dim=(0, 2, 3, 4))
        return dx, dw, db, None, None


class ConvTranspose3dFn(torch.autograd.Function):
    """nn.ConvTranspose3d(k=3, stride=2, padding=1, output_padding=1, bias=False); weight [Cin,Cout,3,3,3]."""

    @staticmethod
    def forward(ctx, x, weight):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        if tuple(weight.shape[2:]) != (3, 3, 3):
            raise _lib.DiffuVolumeError(f"unsupported ConvTranspose3d kernel {tuple(weight.shape[2:])}")
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        return Deconv3dPlan(weight.detach().contiguous(), None, act=ACT_NONE)(x)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = _plan(w.detach(), 2)(g)
        if ctx.needs_input_grad[1]:
            dw = conv3d_weight_grad(g, x, 3, 2, w.shape[0])          # x and g exchanged
        return dx, dw


def deconv3d_k4_input_grad(g: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """dx [B,Ci,D,H,W] of ConvTranspose3d(k4, s2, p1) with weight ``w`` [Ci,Co,4,4,4] from the output gradient
    ``g`` [B,Co,2D,2H,2W]."""
    g, w = g.contiguous(), w.contiguous()
    b, co, d2, h2, w2 = g.shape
    ci = w.shape[0]
    if tuple(w.shape[1:]) != (co, 4, 4, 4) or d2 % 2 or h2 % 2 or w2 % 2:
        raise _lib.DiffuVolumeError(f"k4 input gradient: weight {tuple(w.shape)} against gradient {tuple(g.shape)}")
    wp = _lib.workspace("dv_deconv3d_k4s2_dgrad_packed_floats", g.device, ci, co)
    dx = torch.empty((b, ci, d2 // 2, h2 // 2, w2 // 2), dtype=torch.float32, device=g.device)
    _lib.launch("dv_deconv3d_k4s2_dgrad_pack_weights_f32", g.device, w.data_ptr(), wp.data_ptr(), ci, co)
    _lib.launch("dv_deconv3d_k4s2_dgrad_f32", g.device, g.data_ptr(), wp.data_ptr(), dx.data_ptr(), b, ci, d2 // 2, h2 // 2,
                w2 // 2, co)
    return dx


def deconv3d_k4_weight_grad(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dW [Ci,Co,4,4,4] of ConvTranspose3d(k4, s2, p1) with input ``x`` [B,Ci,D,H,W] and output gradient ``g``."""
    x, g = x.contiguous(), g.contiguous()
    b, ci, d, h, w = x.shape
    co = g.shape[1]
    if tuple(g.shape) != (b, co, 2 * d, 2 * h, 2 * w):
        raise _lib.DiffuVolumeError(f"k4 weight gradient: input {tuple(x.shape)} against gradient {tuple(g.shape)}")
    ws = _lib.workspace("dv_deconv3d_k4s2_wgrad_workspace_floats", x.device, b, ci, d, h, w, co)
    if ws is None:
        raise _lib.DiffuVolumeError(f"dv_deconv3d_k4s2_wgrad_f32 does not take the shape {tuple(x.shape)}")
    dw = torch.empty((ci, co, 4, 4, 4), dtype=torch.float32, device=x.device)
    _lib.launch("dv_deconv3d_k4s2_wgrad_f32", x.device, x.data_ptr(), g.data_ptr(), dw.data_ptr(), ws.data_ptr(), b, ci, d, h,
                w, co)
    return dw


class ConvTranspose3dK4Fn(torch.autograd.Function):
    """nn.ConvTranspose3d(k=4, stride=2, padding=1, bias=False); weight [Cin,Cout,4,4,4]."""

    @staticmethod
    def forward(ctx, x, weight):
        _lib.check_f32(x, "x")
        _lib.check_f32(weight, "weight")
        if weight.dim() != 5 or tuple(weight.shape[2:]) != (4, 4, 4):
            raise _lib.DiffuVolumeError(f"unsupported ConvTranspose3d kernel {tuple(weight.shape[2:])}")
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        return Deconv3dPlan(weight.detach().contiguous(), None, act=ACT_NONE)(x.detach())

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = deconv3d_k4_input_grad(g, w.detach())
        if ctx.needs_input_grad[1]:
            dw = deconv3d_k4_weight_grad(x, g)
        return dx, dw


def feature_gate_grads(cv: torch.Tensor, logit: torch.Tensor, g: torch.Tensor):
    """(dcv, dlogit) of ``sigmoid(logit).unsqueeze(2) * cv`` from the output gradient ``g``."""
    cv, logit, g = cv.contiguous(), logit.contiguous(), g.contiguous()
    b, c, d, h, w = cv.shape
    dcv, dlogit = torch.empty_like(cv), torch.empty_like(logit)
    ws = _lib.workspace("dv_feature_gate_bwd_workspace_floats", cv.device, b, c, d, h, w)
    _lib.launch("dv_feature_gate_bwd_f32", cv.device, cv.data_ptr(), logit.data_ptr(), g.data_ptr(), dcv.data_ptr(),
                dlogit.data_ptr(), _lib.ptr(ws), b, c, d, h, w)
    return dcv, dlogit


class FeatureGateFn(torch.autograd.Function):
    """FeatureAtt's gate ``sigmoid(logit)[:, :, None] * cv`` (out of place); the backward recomputes the sigmoid."""

    @staticmethod
    def forward(ctx, cv, logit):
        _lib.check_f32(cv, "cv")
        _lib.check_f32(logit, "logit")
        if cv.dim() != 5 or tuple(logit.shape) != (cv.shape[0], cv.shape[1], cv.shape[3], cv.shape[4]):
            raise _lib.DiffuVolumeError(f"gate logits {tuple(logit.shape)} do not match volume {tuple(cv.shape)}")
        cv, logit = cv.contiguous(), logit.contiguous()
        ctx.save_for_backward(cv, logit)
        return feature_gate(cv.detach(), logit.detach(), inplace=False)

    @staticmethod
    def backward(ctx, g):
        cv, logit = ctx.saved_tensors
        dcv, dlogit = feature_gate_grads(cv, logit, g)
        return (dcv if ctx.needs_input_grad[0] else None), (dlogit if ctx.needs_input_grad[1] else None)


def conv3d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1,
           precision: Optional[str] = None) -> torch.Tensor:
    """``precision``: "f32" | "f16" | "bf16"; None = the precision of the model call in progress (``precision_scope``),
    "f32" outside one.  "f16" / "bf16" move the 3x3x3 stride-1 layers with more than one output channel to the fp16 / bf16
    kernels."""
    k = weight.shape[2]
    precision = check_precision(ambient_precision() if precision is None else precision)
    if route() == "torch":
        if precision in REDUCED and takes_f16(k, stride, weight.shape[0]) and x.is_cuda:
            # the A/B and reference route of "f16" / "bf16": what a reference user gets from autocast (operands AND result
            # in the 16-bit type)
            with torch.autocast("cuda", dtype=REDUCED[precision]):
                y = F.conv3d(x, weight, bias, stride=stride, padding=1)
            return y.float()
        return F.conv3d(x, weight, bias, stride=stride, padding=(k - 1) // 2)
    return Conv3dFn.apply(x, weight, bias, stride, precision)


def conv_transpose3d(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    if route() == "torch":
        return F.conv_transpose3d(x, weight, None, stride=2, padding=1, output_padding=1)
    return ConvTranspose3dFn.apply(x, weight)


def conv_transpose3d_k4(x: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    if route() == "torch":
        return F.conv_transpose3d(x, weight, None, stride=2, padding=1)
    return ConvTranspose3dK4Fn.apply(x, weight)


def feature_gate_train(cv: torch.Tensor, logit: torch.Tensor) -> torch.Tensor:
    if route() == "torch":
        return torch.sigmoid(logit).unsqueeze(2) * cv
    return FeatureGateFn.apply(cv, logit)


def conv3d_module(m: torch.nn.Conv3d, x: torch.Tensor, precision: Optional[str] = None) -> torch.Tensor:
    """An nn.Conv3d of the aggregation stack (cubic kernel, padding (k-1)/2) on the differentiable HIP route."""
    return conv3d(x, m.weight, m.bias, stride=m.stride[0], precision=precision)


def conv_transpose3d_module(m: torch.nn.ConvTranspose3d, x: torch.Tensor) -> torch.Tensor:
    """An nn.ConvTranspose3d (stride 2, padding 1, bias-free): kernel 3 with output_padding 1, or kernel 4."""
    if tuple(m.kernel_size) == (4, 4, 4):
        if tuple(m.stride) != (2, 2, 2) or tuple(m.padding) != (1, 1, 1) or tuple(m.output_padding) != (0, 0, 0) \
                or m.bias is not None:
            raise _lib.DiffuVolumeError(f"ConvTranspose3d kernel 4 on the training route: stride 2, padding 1, no bias; got {m}")
        return conv_transpose3d_k4(x, m.weight)
    return conv_transpose3d(x, m.weight)
