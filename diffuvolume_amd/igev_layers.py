"""IGEV's 2-D layers (KITTI15/core/submodule.py:9-150, core/extractor.py:10-74), each written once as a function of
a *route*, and the walk over an nn.Sequential of them.  The routes:
  ``HIP``    inference on the in-tree kernels (`hip_conv2d` with eval BatchNorm folded, `instance_norm_act` in place): no
             MIOpen, so a rerun and a shard of a batch give the same bits as the batch.  Plans are cached per layer and
             rebuilt when a weight is loaded, moved or overwritten in place (key = data pointers + versions).
  ``TORCH``  the module's own PyTorch expression: what a module's ``forward`` takes for an input that asks for gradients.
  ``TRAIN``  the differentiable HIP route (train2d): BatchNorm2d is the module's own call (frozen by `freeze_bn()` an
             affine map whose weight and bias still train; in train mode batch statistics), activations are PyTorch.
A module's ``forward`` picks HIP or TORCH; the owners (IGEVFront2d, IGEVStereo_ddim.forward_train) pass TRAIN.  The
modules' own forwards are not used for training: they take the inference kernels whenever the input asks for no
gradient -- images never do --, which leaves these weights without one, and their autograd fallback is MIOpen, whose
backward-weights does not return the same bits twice."""
from __future__ import annotations

import weakref
from functools import partial
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, train2d, train3d
from .plans import settle_build
from .submodule import (ACT_LEAKY, ACT_NONE, ACT_RELU, Conv2dPlan, Conv3dPlan, Deconv2dK4S2Plan, Deconv3dPlan, _dev_f32,
                        weight_key)

ACT_RELU6 = -6                # the walkers' own code: `dv_dwconv3x3_f32` takes it as a capped ReLU inside the launch, the
                              # other kernels have no ReLU6 and every route spells it out
_PLAN_CACHE = weakref.WeakKeyDictionary()


def _wants_autograd(*xs) -> bool:
    return torch.is_grad_enabled() and any(x.requires_grad for x in xs)


def _train_mode(m: nn.Module) -> bool:
    """The training route of a volume-side module, decided per module like the update block's (update.py): the module is
    in train mode and autograd records.  Not ``x.requires_grad``: a frozen backbone still trains the volume weights."""
    return m.training and torch.is_grad_enabled()


def _bn_tuple(bn):
    return None if bn is None else (bn.weight, bn.bias, bn.running_mean, bn.running_var)


def _require_cuda(*named):
    for name, t in named:
        if not t.is_cuda:
            raise _lib.DiffuVolumeError(f"{name} is on {t.device}: training runs on the MI355X (no CPU fallback)")


def _refuse_autocast(what: str):
    if torch.is_autocast_enabled("cuda"):
        raise _lib.DiffuVolumeError(f"{what} trains in float32: fp16 / bf16 autocast is not supported in train mode "
                                    "(mixed-precision training is IGEVStereo_ddim.forward_train(..., amp=True))")


def freeze_bn(self):
    """The reference's ``freeze_bn`` (igev_stereo_ddim.py:198-201), a method of the modules that own 2-D BatchNorm."""
    for m in self.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.eval()


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
        settle_build(x.device)                 # the cache is shared by every stream and thread that calls this layer
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
        _lib.launch("dv_conv2d_fewin_f32", x.device, x.data_ptr(), self.w.data_ptr(), _lib.ptr(self.bias), _lib.ptr(self.scale),
                    _lib.ptr(self.shift), out.data_ptr(), b, c, h, w, self.cout, self.k, self.stride, self.act)
        return out


def depthwise_stride(conv: nn.Module) -> int:
    """The stride of a depthwise 3x3 convolution as MobileNetV2 builds it -- nn.Conv2d(C, C, 3, stride, 1, groups=C,
    bias=False) with stride 1 or 2 --; anything else raises."""
    st = conv.stride[0] if isinstance(conv, nn.Conv2d) and not isinstance(conv, nn.ConvTranspose2d) else 0
    if (st not in (1, 2) or conv.stride != (st, st) or conv.kernel_size != (3, 3) or conv.padding != (1, 1)
            or conv.dilation != (1, 1) or conv.groups != conv.in_channels or conv.out_channels != conv.in_channels
            or conv.bias is not None or conv.padding_mode != "zeros"):
        raise _lib.DiffuVolumeError(f"depthwise Conv2d on the HIP front: kernel 3, padding 1, stride 1 or 2, groups = "
                                    f"channels, no bias, got {conv}")
    return st


def hip_dwconv2d(conv: nn.Conv2d, x: torch.Tensor, bn: Optional[nn.BatchNorm2d] = None, act: int = ACT_NONE) -> torch.Tensor:
    """``act(bn(conv(x)))`` for a depthwise 3x3 nn.Conv2d (`depthwise_stride`) with eval-mode BatchNorm folded and
    ``act`` in ACT_NONE / ACT_RELU / ACT_RELU6 applied inside the one launch of `dv_dwconv3x3_f32`."""
    x = _dev_f32(x, "x")
    if bn is not None and bn.training:
        raise _lib.DiffuVolumeError("BatchNorm2d in training mode: the HIP front folds running statistics (model.eval())")
    key = (act, weight_key([conv.weight] + (list(_bn_tuple(bn)) if bn is not None else [])))
    hit = _PLAN_CACHE.get(conv)
    if hit is None or hit[0] != key:
        plan = _DepthwisePlan(conv.weight, bn, depthwise_stride(conv), act)
        settle_build(x.device)
        _PLAN_CACHE[conv] = hit = (key, plan)
    return hit[1](x)


class _DepthwisePlan:
    """A depthwise 3x3 nn.Conv2d [+ eval BatchNorm, folded in double] [+ ReLU | ReLU6] on `dv_dwconv3x3_f32`."""

    def __init__(self, w, bn, stride, act):
        if act not in (ACT_NONE, ACT_RELU, ACT_RELU6):
            raise _lib.DiffuVolumeError(f"depthwise Conv2d on the HIP front: no activation, ReLU or ReLU6, got {act}")
        self.c, self.stride = w.shape[0], stride
        self.w = _dev_f32(w.detach(), "weight").reshape(self.c, 9).contiguous()
        self.act, self.relu_max = (ACT_RELU, 6.0) if act == ACT_RELU6 else (act, 0.0)
        self.scale = self.shift = None
        if bn is not None:
            sc = (bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps))
            self.scale = sc.float().contiguous()
            self.shift = (bn.bias.detach().double() - bn.running_mean.detach().double() * sc).float().contiguous()

    def __call__(self, x):
        b, c, h, w = x.shape
        if c != self.c:
            raise RuntimeError(f"expected {self.c} channels, got {c}")
        out = torch.empty((b, c, (h - 1) // self.stride + 1, (w - 1) // self.stride + 1), dtype=torch.float32, device=x.device)
        _lib.launch("dv_dwconv3x3_f32", x.device, x.data_ptr(), self.w.data_ptr(), _lib.ptr(self.scale), _lib.ptr(self.shift),
                    out.data_ptr(), b, c, h, w, self.stride, self.act, self.relu_max)
        return out


def instance_norm_act(x: torch.Tensor, act: int = ACT_NONE, eps: float = 1e-5, inplace: bool = True) -> torch.Tensor:
    """nn.InstanceNorm2d (affine=False) + activation: `dv_instance_norm_act_f32`, one block per (b, c) plane."""
    x = _dev_f32(x, "x")
    b, c, h, w = x.shape
    out = x if inplace else torch.empty_like(x)
    _lib.launch("dv_instance_norm_act_f32", x.device, x.data_ptr(), out.data_ptr(), b * c, h * w, float(eps), act)
    return out


# ---- the routes: conv [+ BatchNorm2d] [+ act], conv + InstanceNorm2d [+ act], add-and-relu; ``act``: ACT_NONE, ACT_RELU,
# ---- ACT_LEAKY (slope 0.01) or ACT_RELU6 -----------------------------------------------------------------------------
class _HipRoute:
    name = "HIP"

    @staticmethod
    def conv(conv, x, bn=None, act=ACT_NONE, residual=None):
        x = hip_conv2d(conv, x, bn, ACT_RELU if act == ACT_RELU6 else act, residual)
        return x.clamp_(max=6.0) if act == ACT_RELU6 else x

    @staticmethod
    def dwconv(conv, x, bn=None, act=ACT_NONE):
        return hip_dwconv2d(conv, x, bn, act)

    @staticmethod
    def conv_in(conv, x, inorm, act=ACT_NONE, torch_norm=False):
        x = instance_norm_act(hip_conv2d(conv, x), ACT_RELU if act == ACT_RELU6 else act, inorm.eps)
        return x.clamp_(max=6.0) if act == ACT_RELU6 else x

    @staticmethod
    def add_relu(x, y):
        return torch.relu_(y.add_(x))


_TORCH_ACT = {ACT_NONE: lambda x: x, ACT_RELU: F.relu, ACT_RELU6: F.relu6, ACT_LEAKY: partial(F.leaky_relu, negative_slope=0.01)}


class _AutogradRoute:
    """Convolution, norm and activation one autograd node each; the two instances differ in the convolution and in who
    runs InstanceNorm.  ``torch_norm`` (TRAIN only has the choice): PyTorch's InstanceNorm2d instead of the HIP pass --
    the spx heads of the upsampler train on it, and the two do not give the same bits."""

    def __init__(self, name, raw_conv, raw_dwconv, hip_inorm):
        self.name, self.raw_conv, self.raw_dwconv, self.hip_inorm = name, raw_conv, raw_dwconv, hip_inorm

    def conv(self, conv, x, bn=None, act=ACT_NONE, residual=None):
        x = self.raw_conv(conv, x)
        x = x if bn is None else bn(x)
        return _TORCH_ACT[act](x if residual is None else residual + x)

    def dwconv(self, conv, x, bn=None, act=ACT_NONE):
        x = self.raw_dwconv(conv, x)
        return _TORCH_ACT[act](x if bn is None else bn(x))

    def conv_in(self, conv, x, inorm, act=ACT_NONE, torch_norm=False):
        x = self.raw_conv(conv, x)
        if torch_norm or not self.hip_inorm:
            return _TORCH_ACT[act](inorm(x))
        x = train2d.instance_norm_act(x, ACT_NONE if act == ACT_RELU6 else act, inorm.eps)   # ReLU6 after the launch
        return F.relu6(x) if act == ACT_RELU6 else x

    @staticmethod
    def add_relu(x, y):
        return F.relu(x + y)


def _train_conv(conv, x):
    return train2d.conv_transpose2d_module(conv, x) if isinstance(conv, nn.ConvTranspose2d) else train2d.conv2d_any(conv, x)


def _train_dwconv(conv, x):
    return train2d.dwconv2d(x, conv.weight, depthwise_stride(conv))


HIP = _HipRoute()
TORCH = _AutogradRoute("torch", lambda conv, x: conv(x), lambda conv, x: conv(x), hip_inorm=False)
TRAIN = _AutogradRoute("training", _train_conv, _train_dwconv, hip_inorm=True)


def _own_route(*xs):
    """What a module's own ``forward`` runs on: TORCH for an input that asks for gradients, else the inference kernels."""
    return TORCH if _wants_autograd(*xs) else HIP


# ---- the layers, once each: ``layer(route, module, x)`` ---------------------------------------------------------------
def basic_conv(route, m, x):
    """The 2-D BasicConv (core/submodule.py:27-35)."""
    if m.is_3d:
        raise _lib.DiffuVolumeError("3-D BasicConv runs through its HIP plan, not nn.Module.forward")
    return route.conv(m.conv, x, m.bn if m.use_bn else None, ACT_LEAKY if m.relu else ACT_NONE)


def basic_conv_in(route, m, x, torch_norm=False):
    """BasicConv_IN (core/submodule.py:99-107); ``torch_norm``: see _AutogradRoute."""
    act = ACT_LEAKY if m.relu else ACT_NONE
    if m.use_in:
        return route.conv_in(m.conv, x, m.IN, act, torch_norm=torch_norm)
    return route.conv(m.conv, x, None, act)


def conv2x(route, m, x, rem, torch_norm=False):
    """Conv2x / Conv2x_IN (core/submodule.py:62-76 / :133-150)."""
    layer = partial(basic_conv_in, torch_norm=torch_norm) if isinstance(m, Conv2x_IN) else basic_conv
    x = layer(route, m.conv1, x)
    if x.shape != rem.shape:
        x = F.interpolate(x, size=(rem.shape[-2], rem.shape[-1]), mode="nearest")
    x = torch.cat((x, rem), 1) if m.concat else x + rem
    return layer(route, m.conv2, x)


def residual_block(route, m, x):
    """ResidualBlock (core/extractor.py:46-56)."""
    y = route.conv(m.conv1, x, m.norm1, ACT_RELU)
    y = route.conv(m.conv2, y, m.norm2, ACT_RELU)
    if m.downsample is not None:
        x = route.conv(m.downsample[0], x, m.downsample[1], ACT_NONE)
    return route.add_relu(x, y)


def _parse(route, seq):
    """The members of an nn.Sequential (or a list of modules) of the front as a flat list of ``step(x)`` callables:
    [conv][BatchNorm2d | InstanceNorm2d][ReLU | ReLU6 | LeakyReLU(0.01)] groups, nested nn.Sequential, ResidualBlock,
    BasicConv_IN and the 2-D BasicConv.  The whole list is checked before anything is launched."""
    mods = list(seq) if isinstance(seq, (nn.Sequential, list, tuple)) else [seq]
    steps, i = [], 0
    while i < len(mods):
        m, i = mods[i], i + 1
        if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)):
            bn, inorm, act = None, None, ACT_NONE
            if i < len(mods) and isinstance(mods[i], nn.BatchNorm2d):
                bn, i = mods[i], i + 1
            elif i < len(mods) and isinstance(mods[i], nn.InstanceNorm2d):
                inorm, i = mods[i], i + 1
                if inorm.affine or inorm.track_running_stats:
                    raise _lib.DiffuVolumeError("InstanceNorm2d on the HIP front: affine=False, no running statistics")
            if i < len(mods) and isinstance(mods[i], (nn.ReLU, nn.ReLU6, nn.LeakyReLU)):       # (subclasses of the three too)
                a, i = mods[i], i + 1
                if isinstance(a, nn.LeakyReLU) and abs(a.negative_slope - 0.01) > 1e-12:
                    raise _lib.DiffuVolumeError("LeakyReLU on the HIP front: negative_slope 0.01")
                act = ACT_LEAKY if isinstance(a, nn.LeakyReLU) else (ACT_RELU6 if isinstance(a, nn.ReLU6) else ACT_RELU)
            steps.append(partial(route.conv, m, bn=bn, act=act) if inorm is None else
                         partial(route.conv_in, m, inorm=inorm, act=act))
        elif isinstance(m, nn.Sequential):
            steps += _parse(route, m)
        elif isinstance(m, (nn.Identity, nn.Dropout, nn.Dropout2d)):
            steps += [] if route is HIP else [m]                              # inference skips them
        else:
            layer = next((fn for cls, fn in _LAYERS.items() if isinstance(m, cls)), None)
            if layer is None:
                raise _lib.DiffuVolumeError(f"the 2-D front has no {route.name} route for {type(m).__name__}")
            steps.append(partial(layer, route, m))
    return steps


def walk(route, seq, x):
    for step in _parse(route, seq):
        x = step(x)
    return x


def hip_sequential(seq, x: torch.Tensor) -> torch.Tensor:
    """An nn.Sequential of the front (stems, spx heads, stub backbone stages, FeatureAtt's gate) with every
    [conv][BatchNorm2d | InstanceNorm2d][ReLU | ReLU6 | LeakyReLU(0.01)] run fused on the HIP kernels."""
    return walk(HIP, seq, x)


def train_sequential(seq, x: torch.Tensor) -> torch.Tensor:
    """`hip_sequential`'s walk on the training route.  A member without a training route raises."""
    return walk(TRAIN, seq, x)


# ---- the modules: the reference's constructors and parameter names; ``forward`` picks HIP or TORCH --------------------
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
        bn = _bn_tuple(self.bn if self.use_bn else None)
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
        return basic_conv(_own_route(x), self, x)


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
        return basic_conv_in(_own_route(x), self, x)


class _Conv2xBase(nn.Module):
    """core/submodule.py:36-76 / :110-150: stride-2 (de)convolution, resize to the skip tensor, concat (or add), 3x3."""

    def forward(self, x, rem):
        return conv2x(_own_route(x, rem), self, x, rem)


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
        return residual_block(_own_route(x), self, x)


def _stem(cin, cout):
    """`stem_2` / `stem_4` (igev_stereo_ddim.py:168-177)."""
    return nn.Sequential(BasicConv_IN(cin, cout, kernel_size=3, stride=2, padding=1),
                         nn.Conv2d(cout, cout, 3, 1, 1, bias=False), nn.InstanceNorm2d(cout), nn.ReLU())


_LAYERS = {ResidualBlock: residual_block, BasicConv_IN: basic_conv_in, BasicConv: basic_conv}     # members the walk knows
