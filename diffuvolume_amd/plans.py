"""The inference plans: a layer's weights repacked once for its HIP kernel, BatchNorm folded in, and a ``__call__`` that
picks the kernel for the shape it is handed and launches it on the current stream (inference only: the training routes are
train2d.py / train3d.py).  ``PlanCache`` keeps a module's plans until its weights change.

What the plans share is here once: ``_dev_f32`` (the tensor check), ``same_shape`` (an epilogue operand), ``cat_parts`` /
``cat_args`` (a virtual concatenation, checked, and its pointer / channel arrays) and ``pack`` (a weight image).  Every
launch goes through ``_lib.timed_launch`` (or ``_lib.launch`` where it carries no timer tag).
"""
from __future__ import annotations

import ctypes
import itertools
import os
from typing import Optional, Tuple

import torch

from . import _lib
from .profiling import S2PP_MULT_REDUCTION, WINO3_MULT_REDUCTION, WINO_MULT_REDUCTION

ACT_NONE, ACT_RELU, ACT_MISH, ACT_LEAKY, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3, 4, 5     # last two: 2-D convs only



_CONV_PRECISION = None


def set_default_conv_precision(precision=None) -> None:
    """Override DV_CONV_PRECISION for plans built from now on ('f32', 'f32_direct', 'f16x3' or None = environment)."""
    global _CONV_PRECISION
    if precision not in (None, "f32", "f32_direct", "f16x3"):
        raise ValueError("precision must be 'f32', 'f32_direct', 'f16x3' or None")
    _CONV_PRECISION = precision


_OVERFLOW_FLAGS = {}


def split_overflow_flag(device) -> torch.Tensor:
    """Device int32 the split-fp16 conv kernels raise when an activation leaves the fp16 range."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    if key not in _OVERFLOW_FLAGS:
        flag = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
        settle_build(flag.device)             # zeroed before a kernel on any other stream can raise it
        _OVERFLOW_FLAGS[key] = flag
    return _OVERFLOW_FLAGS[key]


def check_split_overflow(device) -> None:
    """Raise (after one device sync) if a split-fp16 convolution saw an out-of-range activation since the
    last check; the wrappers call it before they hand results back."""
    flag = split_overflow_flag(device)
    if int(flag.item()) != 0:
        flag.zero_()
        raise _lib.DiffuVolumeError("an activation exceeded the split-fp16 range (|x| >= 2.6e5 or NaN): "
                                    "rebuild the plans with precision='f32' (DV_CONV_PRECISION=f32)")


def default_conv_precision() -> str:
    """'f32' = fp32 MFMA everywhere, the 3x3x3 stride-1 layers in the Winograd F(2x2,3x3) form
    (csrc/conv3d_wino.hip; default); 'f32_direct' = fp32 MFMA with direct taps everywhere (csrc/conv3d.hip);
    'f16x3' = the split-fp16 kernel for the 3x3x3 stride-1 layers it covers (csrc/conv3d_f16x3.hip; inputs must
    stay below 2.6e5 in magnitude).  Set with DV_CONV_PRECISION, set_default_conv_precision() or per plan."""
    return _CONV_PRECISION or os.environ.get("DV_CONV_PRECISION", "f32")


def _dev_f32(t: torch.Tensor, name: str) -> torch.Tensor:
    _lib.check_f32(t, name)
    if torch.is_grad_enabled() and t.requires_grad:
        raise NotImplementedError("the HIP hot path is inference-only; call it under torch.no_grad()")
    return t.contiguous()


def same_shape(t: Optional[torch.Tensor], like, name: str) -> Optional[torch.Tensor]:
    """An optional epilogue operand: None, or ``t`` checked and contiguous with the shape of ``like`` (a tensor or a shape)."""
    if t is None:
        return None
    t = _dev_f32(t, name)
    if tuple(t.shape) != tuple(getattr(like, "shape", like)):
        raise RuntimeError(f"{name} shape mismatch")
    return t


def cat_parts(x, cin: int) -> list:
    """The sources of a virtual concatenation -- ``x`` itself or a list of 1..4 tensors whose channels sum to ``cin`` --
    checked and contiguous."""
    parts = [_dev_f32(t, "x") for t in (x if isinstance(x, (list, tuple)) else [x])]
    if not 1 <= len(parts) <= 4 or any(t.shape[0] != parts[0].shape[0] or t.shape[2:] != parts[0].shape[2:] for t in parts):
        raise RuntimeError("virtual concatenation: 1..4 tensors with equal batch and spatial size")
    got = sum(t.shape[1] for t in parts)
    if got != cin:
        raise RuntimeError(f"expected {cin} input channels, got {got}")
    return parts


def cat_args(parts) -> tuple:
    """(pointer array, channel-count array, n): how every ``*_cat_*`` entry takes a virtual concatenation."""
    n = len(parts)
    return (ctypes.c_void_p * n)(*[t.data_ptr() for t in parts]), (ctypes.c_int * n)(*[t.shape[1] for t in parts]), n


def pack(size_entry: str, pack_entry: str, w: torch.Tensor, *dims, dtype=torch.float32) -> torch.Tensor:
    """The weight image ``pack_entry`` makes of ``w``: as many floats (or bytes, kept as ``dtype``) as ``size_entry`` returns
    for ``dims``."""
    n = getattr(_lib.load(), size_entry)(*dims)
    out = torch.empty(n // dtype.itemsize if size_entry.endswith("_bytes") else n, dtype=dtype, device=w.device)
    _lib.launch(pack_entry, w.device, w.data_ptr(), out.data_ptr(), *dims)
    return out


class AttentionConcatVolume:
    """``F.softmax(att_weights, dim=2) * build_concat_volume(left, right)`` (acv_ddim.py:388-390) kept as its three
    FACTORS -- p = softmax(att) [B,D,h,w] and the two feature maps [B,C,h,w] -- instead of the [B,2C,D,h,w] tensor
    (3.0 GB at batch 8).  The first aggregation layer of every DDIM step reads the factors (``Rank1FilterPlan``), so on
    the model's own path the tensor is never written; ``tensor()`` materialises it (once) for any other consumer.
    The factors are private copies: nothing the caller does to its feature tensors afterwards can reach them."""

    def __init__(self, p_att: torch.Tensor, ref: torch.Tensor, tgt: torch.Tensor):
        self.p_att, self.ref, self.tgt = p_att, ref, tgt
        b, d, h, w = p_att.shape
        self.shape = torch.Size((b, 2 * ref.shape[1], d, h, w))
        self.device, self.dtype = p_att.device, p_att.dtype
        self._tensor: Optional[torch.Tensor] = None
        self._rank1_tables = None

    def dim(self) -> int:
        return 5

    def size(self, i: Optional[int] = None):
        return self.shape if i is None else self.shape[i]

    def numel(self) -> int:
        return self.shape.numel()

    def tensor(self) -> torch.Tensor:
        """The materialised [B,2C,D,h,w] volume (``dv_concat_attn_volume_f32`` run on p directly)."""
        if self._tensor is None:
            b, c2, d, h, w = self.shape
            out = torch.empty(tuple(self.shape), dtype=torch.float32, device=self.device)
            if out.numel() == 0:
                self._tensor = out
                return out
            _lib.timed_launch("concat_attn_volume", 2.0 * out.numel(),
                              4.0 * (2 * self.ref.numel() + self.p_att.numel() + out.numel()), "dv_concat_prob_volume_f32",
                              self.device, self.ref.data_ptr(), self.tgt.data_ptr(), self.p_att.data_ptr(), out.data_ptr(),
                              b, c2 // 2, h, w, d)
            self._tensor = out
        return self._tensor


def volume_factors(volume) -> Optional[AttentionConcatVolume]:
    """The factors a volume may be replaced by: the handle itself, or the ride-along of a tensor that
    ``build_concat_attention_volume`` returned and that has not been written to since (any in-place operation on the
    tensor bumps ``_version``; a clone / slice / arithmetic result is a new tensor without the attribute)."""
    if isinstance(volume, AttentionConcatVolume):
        return volume
    fac = getattr(volume, "_dv_factors", None)
    if fac is None or getattr(volume, "_dv_factors_version", None) != volume._version:
        return None
    return fac


class Conv3dPlan:
    """A Conv3d(bias=False)[+BatchNorm3d eval][+activation] layer prepared for the
    implicit-GEMM kernel: weights repacked once on the device, BN folded to a
    per-channel scale/bias applied in the epilogue (submodule.py:94-97).

    ``precision``: 'f32' (default; Winograd / polyphase fp32 MFMA), 'f32_direct' (fp32 MFMA, direct taps) or 'f16x3', the
    opt-in split-fp16 kernel of the 3x3x3 stride-1 layers.  'f16x3' is as accurate as the fp32 kernels at unit-amplitude
    activations (3.5e-7 against float64 on the 26-layer stack); its 22-bit hi + lo split holds for |x * in_scale| >= 0.5,
    and below that every activation carries an absolute error of up to 2^-23 (2^-23 * sum |w| per output) -- see
    csrc/conv3d_f16x3.hip."""

    # 3x3x3 stride-1 layers: the F(2x2x2,3x3x3) kernel (False: the in-plane F(2x2,3x3) kernel everywhere; tests / A-B runs)
    # from WINO3_MIN_CIN input channels on -- measured at batch 8 (tools/ab_wino3.py): 64 -> 64 -6.5 %, 128 -> 128 -7.5 %,
    # 32 -> 32 +1.5 % (eight chunks do not amortise a block's prologue and depth exchange)
    WINO3 = True
    WINO3_MIN_CIN = 64

    def __init__(self, weight: torch.Tensor, bn: Optional[Tuple[torch.Tensor, ...]] = None,
                 stride: int = 1, act: int = ACT_NONE, bias: Optional[torch.Tensor] = None,
                 eps: float = 1e-5, precision: Optional[str] = None):
        w = _dev_f32(weight.detach(), "weight")
        self.cout, self.cin, k = w.shape[0], w.shape[1], w.shape[2]
        if tuple(w.shape[2:]) != (k, k, k) or k not in (1, 3):
            raise _lib.DiffuVolumeError(f"unsupported Conv3d kernel {tuple(w.shape[2:])}")
        self.k, self.stride, self.act = k, stride, act
        precision = precision or default_conv_precision()
        if precision not in ("f32", "f32_direct", "f16x3"):
            raise ValueError("precision must be 'f32' (v_mfma_f32_16x16x4_f32; Winograd F(2x2,3x3) in-plane for the "
                             "3x3x3 stride-1 layers), 'f32_direct' (the same instruction, direct taps everywhere) "
                             "or 'f16x3' (split-fp16 MFMA)")
        # the split-fp16 kernel covers the 3x3x3 stride-1 layers (32 output channels per block; wider
        # layers are split over the grid); the single-channel head stays on its vector-ALU kernel
        self.split = precision == "f16x3" and k == 3 and stride == 1 and self.cout > 1
        self.wino = precision == "f32" and k == 3 and stride == 1 and self.cout > 1
        lib = _lib.load()
        # 3x3x3 stride 2, 64 output channels per block: the polyphase minimal-filtering form (csrc/conv3d_s2pp.hip);
        # a call with a filter prologue falls back to the direct kernel (both weight images are kept)
        self.s2pp = (precision == "f32" and k == 3 and stride == 2 and os.environ.get("DV_S2PP", "1") != "0"
                     and bool(lib.dv_conv3d_s2pp_supported(self.cin, self.cout, 4, 4, 4)))
        cc = (self.cin, self.cout)
        if self.s2pp:
            self.wpacked_pp = pack("dv_conv3d_s2pp_packed_floats", "dv_conv3d_s2pp_pack_weights_f32", w, *cc)
        if self.wino:
            self.wpacked = pack("dv_conv3d_wino_packed_floats", "dv_conv3d_wino_pack_weights_f32", w, *cc)
            # the F(2x2x2,3x3x3) image (csrc/conv3d_wino3.hip): every call without a filter prologue
            self.wpacked3 = pack("dv_conv3d_wino3_packed_floats", "dv_conv3d_wino3_pack_weights_f32", w, *cc)
        elif self.split:
            self.wpacked = pack("dv_conv3d_f16x3_packed_bytes", "dv_conv3d_f16x3_pack_weights", w, *cc, dtype=torch.float16)
        else:
            self.wpacked = pack("dv_conv3d_packed_floats", "dv_conv3d_pack_weights_f32", w, *cc, k)
        self.scale, self.shift = _fold_bn(bn, bias, self.cout, w.device, eps)

    def out_shape(self, shape):
        b, _, d, h, w = shape
        s = self.stride
        f = (lambda n: (n - 1) // s + 1)
        return (b, self.cout, f(d), f(h), f(w))

    def __call__(self, x: torch.Tensor, in_scale: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None
                 ) -> torch.Tensor:
        x = _dev_f32(x, "x")
        b, cin, d, h, w = x.shape
        if cin != self.cin:
            raise RuntimeError(f"expected {self.cin} input channels, got {cin}")
        if out is None:
            out = torch.empty(self.out_shape(x.shape), dtype=torch.float32, device=x.device)
        if in_scale is not None:
            in_scale = _dev_f32(in_scale, "in_scale")
            if in_scale.numel() != b * d * h * w:
                raise RuntimeError("in_scale must be [B,D,H,W]")
        residual = same_shape(residual, self.out_shape(x.shape), "residual")
        lib = _lib.load()
        flops = 2.0 * out.numel() * cin * self.k ** 3
        nb = 4.0 * (x.numel() + out.numel() + (0 if in_scale is None else in_scale.numel())
                    + (0 if residual is None else residual.numel()))
        tag = f"conv3d_k{self.k}s{self.stride}_co{self.cout}" + ("" if in_scale is None else "_filter")
        plain = in_scale is None and x.data_ptr() % 16 == 0        # what the kernels without a filter prologue take
        # the route: entry, weight image, whether the entry has the filter prologue's operand, matrix-pipe flops
        if self.split:
            name, wimg, filt, issued = "dv_conv3d_f16x3_f32", self.wpacked, True, 0.0
            tag = f"conv3d_f16x3_co{self.cout}" + ("" if in_scale is None else "_filter")
        elif self.wino and self.WINO3 and cin >= self.WINO3_MIN_CIN and plain and lib.dv_conv3d_wino3_supported(cin, self.cout, d, h, w):
            name, wimg, filt, issued = "dv_conv3d_wino3_f32", self.wpacked3, False, flops / WINO3_MULT_REDUCTION
        elif self.wino:
            name, wimg, filt, issued = "dv_conv3d_wino_f32", self.wpacked, True, flops / WINO_MULT_REDUCTION
        elif self.s2pp and plain and lib.dv_conv3d_s2pp_supported(cin, self.cout, d, h, w):
            name, wimg, filt, issued = "dv_conv3d_s2pp_f32", self.wpacked_pp, False, flops / S2PP_MULT_REDUCTION
        else:
            name, wimg, filt, issued = "dv_conv3d_f32", self.wpacked, True, (flops if self.cout > 1 else 0.0)
        _lib.timed_launch(tag, flops, nb, name, x.device, x.data_ptr(), wimg.data_ptr(), _lib.ptr(self.scale), _lib.ptr(self.shift),
                          *((_lib.ptr(in_scale),) if filt else ()), _lib.ptr(residual), out.data_ptr(),
                          *((split_overflow_flag(x.device).data_ptr(),) if self.split else ()), b, cin, d, h, w, self.cout,
                          *((self.k, self.stride) if name == "dv_conv3d_f32" else ()), self.act, issued=issued)
        return out


def settle_build(device=None) -> None:
    """Wait for the stream something was just BUILT on -- packed weights, folded BatchNorm, a table -- before it is kept
    where another stream can find it: the current stream of ``device`` (None: the current device).  The build's kernels
    are enqueued there and nothing else orders them before a consumer on another stream -- a second thread, a replica
    that finds the plans parked, the same caller on a later request.  Once per build, never per step.  A capturing
    stream cannot be waited for and is left alone: builds are never captured (igev_loop.py warms up eagerly)."""
    if not torch.cuda.is_available():
        return
    with torch.cuda.device(device):
        if not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream().synchronize()


def weight_key(tensors) -> tuple:
    """Identity of a weight set: (storage address, in-place version) of every tensor -- a weight replaced through
    ``param.data = ...`` changes the address, an in-place write (``copy_``, an optimizer step) the version."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


class PlanCache:
    """Mixed into every nn.Module that holds HIP plans (weights repacked for a kernel, BatchNorm folded in).  The module
    defines ``_build_plans(slot)``; ``plans(slot)`` builds a named slot once and keeps it until the weights change:

    - ``.to()`` / ``.cuda()``, ``load_state_dict`` (through this module or any parent or wrapper: ``nn.DataParallel(
      model).load_state_dict`` only reaches ``_load_from_state_dict``) and a real train/eval toggle drop the plans;
    - an in-place write or a ``.data`` swap fires no hook: ``refresh_plans()``, called at the public entry points (never
      inside a loop), compares the weight key recorded at build time with the current one and drops the plans of the
      whole subtree when they differ;
    - ``nn.DataParallel`` re-creates its replicas on EVERY forward (SceneFlow/test_sceneflow_ddim.py:54-61, KITTI12/
      test.py), so a replica parks the plans it builds on the module it was copied from, keyed by device and slot and
      valid for one weight key of that SOURCE (the replicas' own weights are re-broadcast from it each time).

    Streams: this level carries the guarantee that plans may cross streams.  When ``plans(slot)`` or ``prepare()`` returns,
    the stream the plans were built on has been waited for (``settle_build``, before they are stored or parked), so they
    may be used on any stream of their device -- by another thread, or by a replica that finds them parked.  What a
    plan builds later on first use and keeps (``_RefinePlan.plan``, the per-layer cache of igev_layers, ``ddim.loop_plan``)
    settles the same way.  A bare plan object built outside a PlanCache belongs to the stream that built it."""

    @property
    def _plans(self):
        """The default slot's plans, None until they are built."""
        return self.__dict__.get("_plan_slots", {}).get(None)

    def _weight_key(self) -> tuple:
        return weight_key(itertools.chain(self.parameters(), self.buffers()))

    def _drop_plans(self):
        for name in ("_plan_slots", "_plan_key", "_replica_plans"):
            self.__dict__.pop(name, None)

    def plans(self, slot=None):
        slots = self.__dict__.setdefault("_plan_slots", {})
        p = slots.get(slot)
        if p is None:
            src = self.__dict__.get("_plan_source")
            if src is not None:
                # a replica holds its weights as plain attributes (not parameters); nn.DataParallel runs each replica
                # under its own device, so that is the device its plans are built on
                where, src_key = (torch.cuda.current_device(), slot), src._weight_key()
                parked = src.__dict__.setdefault("_replica_plans", {})
                p = parked[where][1] if where in parked and parked[where][0] == src_key else None
            if p is None:
                p = self._build_plans(slot)
                self._settle_build()          # before the plans are stored or parked: from here on any stream may use them
                if src is not None:
                    parked[where] = (src_key, p)
            if "_plan_key" not in self.__dict__:
                self.__dict__["_plan_key"] = self._weight_key()
            slots[slot] = p
        return p

    def _settle_build(self):
        """``settle_build`` on the device of the weights (a replica's weights are plain attributes: the current device)."""
        devices = {t.device for t in itertools.chain(self.parameters(), self.buffers()) if t.is_cuda}
        for d in devices or {None}:
            settle_build(d)

    def drop_slot(self, slot):
        """Drop one slot's plans (a slot that keeps a narrower weight key of its own and found it stale)."""
        self.__dict__.get("_plan_slots", {}).pop(slot, None)

    def refresh_plans(self):
        """Drop every plan in this module's subtree if a weight was written in place or swapped since they were built."""
        key = self._weight_key()
        if self.__dict__.get("_plan_key") != key:
            for m in self.modules():
                if isinstance(m, PlanCache):
                    m._drop_plans()
            self.__dict__["_plan_key"] = key

    def prepare(self, check_weights: bool = False):
        """The default slot's plans; ``check_weights=True`` refreshes them first (what the public entry points do)."""
        if check_weights:
            self.refresh_plans()
        return self.plans()

    def _apply(self, fn, *args, **kwargs):
        self._drop_plans()
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._drop_plans()
        return super()._load_from_state_dict(*args, **kwargs)

    def train(self, mode: bool = True):
        if mode != self.training:          # the reference calls model.eval() on every batch: keep the plans then
            self._drop_plans()
        return super().train(mode)

    def _replicate_for_data_parallel(self):
        replica = super()._replicate_for_data_parallel()      # a shallow copy of __dict__: the cache must not be shared
        replica._drop_plans()
        replica.__dict__["_plan_source"] = self.__dict__.get("_plan_source") or self
        return replica


class PointwiseExpandPlan:
    """A 1x1 Conv2d(bias=False) from few input channels (<= 32) to many output channels, nothing fused: the per-pair
    table convolutions of ``Rank1FilterPlan`` (csrc/pointwise_expand.hip).  weight [Cout, Cin, 1, 1] or [Cout, Cin]."""

    MAX_CIN = 32

    def __init__(self, weight: torch.Tensor):
        w = _dev_f32(weight.detach(), "weight")
        w = w.reshape(w.shape[0], -1).contiguous()
        self.cout, self.cin = w.shape
        if self.cin > self.MAX_CIN:
            raise _lib.DiffuVolumeError(f"PointwiseExpandPlan: at most {self.MAX_CIN} input channels")
        self.wpacked = pack("dv_pointwise_expand_packed_floats", "dv_pointwise_expand_pack_weights_f32", w, self.cin, self.cout)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        x = _dev_f32(x, "x")
        b, cin, h, w = x.shape
        if cin != self.cin:
            raise RuntimeError(f"expected {self.cin} input channels, got {cin}")
        out = torch.empty((b, self.cout, h, w), dtype=torch.float32, device=x.device)
        _lib.timed_launch(f"pointwise_expand_co{self.cout}", 2.0 * out.numel() * cin, 4.0 * (x.numel() + out.numel()),
                          "dv_pointwise_expand_f32", x.device, x.data_ptr(), self.wpacked.data_ptr(), out.data_ptr(), b, cin,
                          h * w, self.cout, issued=2.0 * out.numel() * 32)
        return out


class Rank1FilterPlan:
    """The first layer of a DiffuVolume step, ``relu(bn(conv3d(volume * noise)))`` (acv_ddim.py:260 + dres0[0],
    :200-203), on the FACTORS of its input instead of the [B,64,48,h,w] volume: with volume = p * [L ; R(x-d)]
    (p = softmax(att), :388-390) and noise a per-voxel scalar the convolution is
    ``sum_tap (p*noise)(.) * (GL[tap] + GR[tap](x - d))``, GL / GR = 1x1 convolutions of L / R with the layer's weights,
    built once per stereo pair (csrc/rank1_filter.hip): 54 instead of 1728 multiply-adds per output, the same function
    up to fp32 re-association.  Used by ``ACVNet_DDIM`` whenever the volume it is handed carries its factors
    (``build_concat_attention_volume`` attaches them); any other volume takes the generic convolution."""

    MAX_D = 48

    def __init__(self, weight: torch.Tensor, bn, act: int = ACT_RELU, eps: float = 1e-5):
        w = _dev_f32(weight.detach(), "weight")
        self.cout, cin2, k = w.shape[0], w.shape[1], w.shape[2]
        if tuple(w.shape[2:]) != (3, 3, 3) or cin2 % 2:
            raise _lib.DiffuVolumeError("Rank1FilterPlan: a 3x3x3 convolution over [left | right] channel halves")
        self.c = cin2 // 2
        self.act = act
        # table weights: output channel = tap * Cout + co
        wl = w[:, :self.c].permute(2, 3, 4, 0, 1).reshape(27 * self.cout, self.c, 1, 1).contiguous()
        wr = w[:, self.c:].permute(2, 3, 4, 0, 1).reshape(27 * self.cout, self.c, 1, 1).contiguous()
        # few input channels -> 27 * Cout output channels, nothing fused: an HBM write stream with its own kernel
        # (csrc/pointwise_expand.hip; the generic 2-D convolution stays for more than 32 input channels)
        mk = PointwiseExpandPlan if self.c <= PointwiseExpandPlan.MAX_CIN else (lambda t: Conv2dPlan(t, None, act=ACT_NONE))
        self.table_l, self.table_r = mk(wl), mk(wr)
        self.scale, self.shift = _fold_bn(bn, None, self.cout, w.device, eps)

    def applies(self, volume) -> bool:
        fac = volume_factors(volume)
        return (fac is not None and len(volume.shape) == 5 and volume.shape[1] == 2 * self.c
                and volume.shape[2] <= self.MAX_D and fac.ref.shape[1] == self.c
                and tuple(fac.p_att.shape) == (volume.shape[0],) + tuple(volume.shape[2:]))

    def tables(self, volume):
        """(GL, GR) [B, 27*Cout, h, w] of a volume's feature maps, cached on its factor handle."""
        fac = volume_factors(volume)
        cached = fac._rank1_tables
        if cached is not None and cached[0] is self:
            return cached[1], cached[2]
        gl, gr = self.table_l(fac.ref), self.table_r(fac.tgt)
        fac._rank1_tables = (self, gl, gr)
        return gl, gr

    def __call__(self, volume, noise01: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``noise01`` None: the unfiltered volume (the origin network's first aggregation layer, acv.py)."""
        p_att = volume_factors(volume).p_att
        b, d, h, w = p_att.shape
        gl, gr = self.tables(volume)
        out = torch.empty((b, self.cout, d, h, w), dtype=torch.float32, device=p_att.device)
        if noise01 is None:
            s = p_att
        else:
            noise01 = _dev_f32(noise01, "noise01")
            if noise01.numel() != p_att.numel():
                raise RuntimeError("the filter must be [B,D,H,W]")
            s = torch.empty_like(p_att)
            _lib.launch("dv_mul_f32", s.device, p_att.data_ptr(), noise01.data_ptr(), s.data_ptr(), s.numel())
        # algorithmic flops / bytes of the layer it replaces; issued on the vector ALU, not the matrix pipe
        _lib.timed_launch(f"conv3d_k3s1_co{self.cout}_filter_rank1", 2.0 * out.numel() * 2 * self.c * 27,
                          4.0 * (volume.numel() + out.numel() + s.numel()), "dv_conv3d_rank1_filter_f32", s.device,
                          s.data_ptr(), gl.data_ptr(), gr.data_ptr(), _lib.ptr(self.scale), _lib.ptr(self.shift), out.data_ptr(),
                          b, d, h, w, self.cout, self.act,
                          valu=out.numel() * 27 * 4.0)       # per output and tap: two fma lanes (GL term, GR term)
        return out


class Deconv2dK4S2Plan:
    """ConvTranspose2d(kernel 4, stride 2, padding 1) [+ bias] [+ BatchNorm2d eval] [+ activation] -- IGEV's `spx_2_gru.conv1`
    and `spx_gru` (KITTI15/core/igev_stereo_ddim.py:110-112, core/submodule.py:27-28) -- on the 3x3 kernels: output pixel
    (2i+a, 2j+b) reads the 2x2 inputs {i-1+a, i+a} x {j-1+b, j+b}, so the four output parities are four 3x3 stride-1
    convolutions of the input (each with five structurally zero taps) whose results interleave (pixel shuffle)."""

    def __init__(self, weight: torch.Tensor, bn=None, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                 eps: float = 1e-5):
        wc = self.parity_weights(weight)
        self.cout = wc.shape[0] // 4
        rep = lambda t: None if t is None else t.detach().repeat_interleave(4)
        self.conv = Conv2dPlan(wc, None if bn is None else tuple(rep(t) for t in bn), act=act, eps=eps, bias=rep(bias))

    @staticmethod
    def parity_weights(weight: torch.Tensor) -> torch.Tensor:
        """[Cin, Cout, 4, 4] -> the [4*Cout, Cin, 3, 3] weights of the four parity convolutions (channel 4 co + 2 a + b
        is output parity (a, b) of channel co: F.pixel_shuffle's order)."""
        w = _dev_f32(weight.detach(), "weight")                  # [Cin, Cout, 4, 4]
        if w.dim() != 4 or tuple(w.shape[2:]) != (4, 4):
            raise _lib.DiffuVolumeError("Deconv2dK4S2Plan: kernel 4, stride 2, padding 1")
        cin, cout = w.shape[0], w.shape[1]
        wc = torch.zeros((cout, 2, 2, cin, 3, 3), dtype=torch.float32, device=w.device)
        tap = {0: {0: 1, -1: 3}, 1: {1: 0, 0: 2}}              # parity -> {input offset: kernel index}
        for a in (0, 1):
            for dy, ky in tap[a].items():
                for b in (0, 1):
                    for dx, kx in tap[b].items():
                        wc[:, a, b, :, dy + 1, dx + 1] = w[:, :, ky, kx].t()
        return wc.reshape(cout * 4, cin, 3, 3)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        return torch.nn.functional.pixel_shuffle(self.conv(x), 2)


class Conv2dPairPlan:
    """Two biased 3x3 convolutions of the same input in one Winograd launch (ConvGRU's `convz` / `convr`,
    KITTI15/core/update.py:33-35): out_g = act(conv_g(x) + bias_g + residual_g) [* mul_g].  Launches too small for the
    Winograd kernel go through the two single plans."""

    def __init__(self, conv1: Tuple[torch.Tensor, Optional[torch.Tensor]], conv2: Tuple[torch.Tensor, Optional[torch.Tensor]],
                 act: int = ACT_NONE):
        (w1, b1), (w2, b2) = conv1, conv2
        self.single = (Conv2dPlan(w1, None, act=act, bias=b1), Conv2dPlan(w2, None, act=act, bias=b2))
        p1, p2 = self.single
        self.act, self.cin, self.c1, self.c2 = act, p1.cin, p1.cout, p2.cout
        self.packed = None
        if p1.wino_packed is not None and p2.wino_packed is not None and p1.cin == p2.cin and self.c1 % 32 == 0:
            w = torch.cat([_dev_f32(w1.detach(), "weight"), _dev_f32(w2.detach(), "weight")], dim=0).contiguous()
            self.packed = pack("dv_conv2d_wino_packed_floats", "dv_conv2d_wino_pack_weights_f32", w, self.cin, self.c1 + self.c2)

            def both(a, b, fill):
                if a is None and b is None:
                    return None
                mk = lambda t, c: t if t is not None else torch.full((c,), fill, dtype=torch.float32, device=w.device)
                return torch.cat([mk(a, self.c1), mk(b, self.c2)]).contiguous()
            self.scale, self.shift = both(p1.scale, p2.scale, 1.0), both(p1.shift, p2.shift, 0.0)

    def __call__(self, x, residual=(None, None), mul=(None, None)):
        singles = lambda: (self.single[0](x, residual=residual[0], mul=mul[0]), self.single[1](x, residual=residual[1], mul=mul[1]))
        if self.packed is None or not 1 <= (len(x) if isinstance(x, (list, tuple)) else 1) <= 4:
            return singles()
        parts = cat_parts(x, self.cin)
        b, _, h, w = parts[0].shape
        cout = self.c1 + self.c2
        if (-(-h // 16)) * (-(-w // 16)) * (cout // 32) < Conv2dPlan.WINO_MIN_BLOCKS:      # of ONE batch item, see Conv2dPlan
            return singles()
        dev = parts[0].device
        outs = [torch.empty((b, c, h, w), dtype=torch.float32, device=dev) for c in (self.c1, self.c2)]
        res = [same_shape(residual[g], outs[g], "residual") for g in (0, 1)]
        mu = [same_shape(mul[g], outs[g], "mul") for g in (0, 1)]
        n_out = outs[0].numel() + outs[1].numel()
        extra = sum(t.numel() for t in res + mu if t is not None)
        args = (*cat_args(parts), self.packed.data_ptr(), _lib.ptr(self.scale), _lib.ptr(self.shift), _lib.ptr(res[0]),
                _lib.ptr(mu[0]), outs[0].data_ptr(), _lib.ptr(res[1]), _lib.ptr(mu[1]), outs[1].data_ptr())
        name, tag = "dv_conv2d_wino_cat_pair_f32", f"conv2d_k3d1_co{self.c1}+{self.c2}"
        ks = _lib.load().dv_conv2d_wino_auto_kslices(self.cin, h, w, cout, 1) if Conv2dPlan.KSPLIT else 1
        if ks > 1:            # a launch that leaves most of the chip empty: K-split, partial tiles in scratch, fixed-order sum
            scratch = torch.empty(ks * n_out, dtype=torch.float32, device=dev)
            name, tag, args = "dv_conv2d_wino_cat_pair_ksplit_f32", tag + "_ksplit", args + (scratch.data_ptr(), ks)
        flops = 2.0 * n_out * self.cin * 9
        _lib.timed_launch(tag, flops, 4.0 * (sum(t.numel() for t in parts) + n_out * (1 + 2 * ks if ks > 1 else 1) + extra),
                          name, dev, *args, b, h, w, self.c1, self.c2, self.act, issued=flops / WINO_MULT_REDUCTION)
        return outs[0], outs[1]


class Conv2dF16Plan:
    """The fp16-autocast form of a stride-1, dilation-1 Conv2d(k 3 or 1) + bias [+ residual] [+ activation] [+ ConvGRU
    gate arithmetic] (csrc/conv2d_f16.hip, v_mfma_f32_16x16x32_f16): what IGEV's update block computes under
    `autocast(enabled=args.mixed_precision)` (KITTI15/core/update.py:26-142, igev_stereo_ddim.py:242-246).  Input,
    weight and bias are rounded to fp16, products accumulate in fp32, the output and every epilogue op's result are
    rounded to fp16; tensors stay float32 holding fp16-exact values.

    Selected per plan by the update block (never through DV_CONV_PRECISION, which steers the 3-D convolutions).  With
    ``pair=(w2, b2)`` it is the two-gate launch of ConvGRU's convz | convr: ``__call__`` then returns two tensors and takes
    ``residual`` / ``mul`` as pairs, like Conv2dPairPlan.

    ``elem``: the 16-bit element type, "f16" (default) or "bf16" -- the same kernel body (csrc/conv2d_mp.h) instantiated on
    v_mfma_f32_16x16x32_bf16 with bfloat16 rounding (csrc/conv2d_bf16.hip, the entries of
    include/diffuvolume_hip_amp2d_bf16.h): the update block's train precision "bf16".  The packed image's size and the
    K-split choice are the fp16 entries': they do not depend on the element type."""

    KSPLIT = True

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: int = ACT_NONE,
                 pair: Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]] = None, elem: str = "f16"):
        if elem not in ("f16", "bf16"):
            raise ValueError(f"Conv2dF16Plan: elem must be 'f16' or 'bf16', got {elem!r}")
        self.elem = elem
        w = _dev_f32(weight.detach(), "weight")
        self.c1, self.cin, self.k = w.shape[0], w.shape[1], w.shape[2]
        if tuple(w.shape[2:]) != (self.k, self.k) or self.k not in (1, 3):
            raise _lib.DiffuVolumeError(f"unsupported Conv2d kernel {tuple(w.shape[2:])} for the {elem} path")
        self.act, self.c2 = act, 0
        biases = [bias]
        if pair is not None:
            w2 = _dev_f32(pair[0].detach(), "weight")
            if self.k != 3 or tuple(w2.shape[1:]) != tuple(w.shape[1:]):
                raise _lib.DiffuVolumeError("pair launch: two 3x3 convolutions of the same input")
            self.c2 = w2.shape[0]
            w = torch.cat([w, w2], dim=0).contiguous()
            biases.append(pair[1])
        cout = self.c1 + self.c2
        self.bias = None
        if any(t is not None for t in biases):
            sizes = [self.c1] + ([self.c2] if pair is not None else [])
            self.bias = torch.cat([_dev_f32(t.detach(), "bias") if t is not None else
                                   torch.zeros(n, dtype=torch.float32, device=w.device) for t, n in zip(biases, sizes)]).contiguous()
        self.wpacked = pack("dv_conv2d_f16_packed_bytes", f"dv_conv2d_{elem}_pack_weights", w, self.cin, cout, self.k,
                            dtype=torch.uint8)

    def __call__(self, x, residual=None, mul=None, blend=None):
        parts = cat_parts(x, self.cin)
        b, _, h, w = parts[0].shape
        is_pair = self.c2 > 0
        if not is_pair:
            residual, mul = (residual,), (mul,)
        elif blend is not None:
            raise RuntimeError("the pair launch has no GRU blend")
        outs = [torch.empty((b, c, h, w), dtype=torch.float32, device=parts[0].device)
                for c in ((self.c1, self.c2) if is_pair else (self.c1,))]
        res = [same_shape(residual[g], outs[g], "residual") for g in range(len(outs))]
        mu = [same_shape(mul[g], outs[g], "mul") for g in range(len(outs))]
        bz, bh = (None, None) if blend is None else (same_shape(blend[0], outs[0], "blend z"), same_shape(blend[1], outs[0], "blend h"))
        cout = self.c1 + self.c2
        n_out = b * cout * h * w
        flops = 2.0 * n_out * self.cin * self.k ** 2
        nb = 4.0 * (sum(t.numel() for t in parts) + n_out + sum(t.numel() for t in res + mu + [bz, bh] if t is not None))
        # the K-split factor looks at ONE batch item (a shard of a batch reproduces the batch's bits, see Conv2dPlan)
        ks = _lib.load().dv_conv2d_f16_auto_kslices(self.cin, h, w, cout, self.k) if self.KSPLIT else 1
        tag = f"conv2d_{self.elem}_k{self.k}_co{self.c1}" + (f"+{self.c2}" if is_pair else "") + ("_ksplit" if ks > 1 else "")
        args = (*cat_args(parts), self.wpacked.data_ptr(), _lib.ptr(self.bias), _lib.ptr(res[0]), _lib.ptr(mu[0]))
        if is_pair:
            name = f"dv_conv2d_{self.elem}_cat_pair"
            args += (outs[0].data_ptr(), _lib.ptr(res[1]), _lib.ptr(mu[1]), outs[1].data_ptr())
            tail = (b, h, w, self.c1, self.c2, self.act)
        else:
            name = f"dv_conv2d_{self.elem}_cat"
            args += (_lib.ptr(bz), _lib.ptr(bh), outs[0].data_ptr())
            tail = (b, h, w, self.c1, self.k, self.act)
        if ks > 1:
            scratch = torch.empty(ks * n_out, dtype=torch.float32, device=parts[0].device)
            name, args = name + "_ksplit", args + (scratch.data_ptr(), ks)
        _lib.timed_launch(tag, flops, nb, name, parts[0].device, *args, *tail)
        return (outs[0], outs[1]) if is_pair else outs[0]


class Conv2dPlan:
    """Conv2d(k 3 or 1, stride 1, padding = dilation) [+ bias] [+ BatchNorm2d eval] [+ residual] [+ activation]
    [+ ConvGRU gate arithmetic] on the 2-D implicit-GEMM kernel: `convbn` / `BasicBlock` of the KITTI12 refinement
    stack (KITTI12/models/submodule.py:21-24, :192-215) and the biased convolutions of IGEV's update block
    (KITTI15/core/update.py)."""

    def __init__(self, weight: torch.Tensor, bn: Optional[Tuple[torch.Tensor, ...]] = None, dilation: int = 1,
                 act: int = ACT_NONE, eps: float = 1e-5, bias: Optional[torch.Tensor] = None, stride: int = 1):
        w = _dev_f32(weight.detach(), "weight")
        self.cout, self.cin, k = w.shape[0], w.shape[1], w.shape[2]
        if tuple(w.shape[2:]) != (k, k) or k not in (1, 3):
            raise _lib.DiffuVolumeError(f"unsupported Conv2d kernel {tuple(w.shape[2:])}")
        if k == 3 and not 1 <= dilation <= 16:
            raise _lib.DiffuVolumeError("3x3 convolutions: dilation 1..16")
        if stride not in (1, 2) or (stride == 2 and k == 3 and dilation != 1):
            raise _lib.DiffuVolumeError("stride 1, or stride 2 with dilation 1")
        self.k, self.dilation, self.act, self.stride = k, (dilation if k == 3 else 1), act, stride
        self.wpacked = pack("dv_conv2d_packed_floats", "dv_conv2d_pack_weights_f32", w, self.cin, self.cout, k, self.dilation)
        # 3x3, stride 1: also the Winograd F(2x2,3x3) image (csrc/conv2d_wino.hip), used when the launch has enough
        # 16x16x32 blocks to fill the chip (small images stay on the direct kernel's small tiles).  Dilated layers
        # run it on their dilation^2 sub-sampled images (up to WINO_MAX_DILATION).
        self.wino_packed = None
        if k == 3 and self.dilation <= self.WINO_MAX_DILATION and stride == 1 and default_conv_precision() == "f32":
            self.wino_packed = pack("dv_conv2d_wino_packed_floats", "dv_conv2d_wino_pack_weights_f32", w, self.cin, self.cout)
        self.scale, self.shift = _fold_bn(bn, bias, self.cout, w.device, eps)

    # Which kernel runs (Winograd or direct, and the K-split factor of the direct one) decides the ORDER an output is summed
    # in, so it may only look at ONE batch item: a shard of a batch has to reproduce the batch's bits (round 5: config 5
    # is sharded over ranks; until then the thresholds counted the whole launch, 128 blocks = 32 per item at batch 4).
    WINO_MIN_BLOCKS = 32
    WINO_MAX_DILATION = 8       # measured at 1248x384 (tools/ab_wino2d_dil.py): d=2 -27 %, d=4 -19 %, d=8 -11..17 %, d=16 +41..57 % (the gathers spread over too many sectors)
    KSPLIT = True               # K-split the launches that are too small to fill the chip (A/B switch for tools/)

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, mul: Optional[torch.Tensor] = None,
                 blend: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, group: int = 1,
                 s2b_out: bool = False) -> torch.Tensor:
        """act(conv(x)*scale + shift + residual) [* mul] [-> h + z*(. - h) for blend = (z, h)].
        ``x`` may be a list of up to four tensors: the convolution then runs over their channel concatenation
        without materialising it (stride 1).  ``group``: how many consecutive batch entries of ``x`` make up ONE sample (the
        sub-images of a space-to-batch tensor): the per-sample block count that picks the kernel is taken over all of them.
        ``s2b_out``: store the result de-interleaved by 2, [4B,Cout,H/2,W/2] (`dv_conv2d_wino_s2b_f32`; Winograd layers
        without residual / mul / blend, even H and W) -- what `pwcnet_ddim.space_to_batch2` would make of it."""
        cat = isinstance(x, (list, tuple))
        parts = cat_parts(x, self.cin)
        if cat and self.stride != 1:
            raise RuntimeError("virtual concatenation is stride-1 only")
        if self.stride == 2 and (mul is not None or blend is not None):
            raise RuntimeError("gate operands are stride-1 only")
        x, cin, cout, k, d = parts[0], self.cin, self.cout, self.k, self.dilation
        b, _, h, w = x.shape
        out = torch.empty((b, cout, (h - 1) // self.stride + 1, (w - 1) // self.stride + 1), dtype=torch.float32, device=x.device)
        residual, mul = same_shape(residual, out, "residual"), same_shape(mul, out, "mul")
        bz, bh = (None, None) if blend is None else (same_shape(blend[0], out, "blend z"), same_shape(blend[1], out, "blend h"))
        extra = sum(t is not None for t in (residual, mul, bz, bh))
        if s2b_out:
            if self.wino_packed is None or d != 1 or self.stride != 1 or extra or h % 2 or w % 2:
                raise _lib.DiffuVolumeError("s2b_out: a 3x3 dilation-1 stride-1 Winograd layer without residual / mul / "
                                            "blend on even H and W")
            out = torch.empty((4 * b, cout, h // 2, w // 2), dtype=torch.float32, device=x.device)
        lib = _lib.load()
        gates = (_lib.ptr(residual), _lib.ptr(mul), _lib.ptr(bz), _lib.ptr(bh), out.data_ptr())
        epilogue = (_lib.ptr(self.scale), _lib.ptr(self.shift))
        tag, wimg, wino, ks = f"conv2d_k{k}d{d}_co{cout}", self.wpacked, False, 1
        # the route: entry, weight image, tag, the arguments before and after the K-split pair (scratch, ks)
        if self.stride == 2:
            name, tag = "dv_conv2d_s2_f32", f"conv2d_k{k}s2_co{cout}"
            args, tail = (x.data_ptr(), wimg.data_ptr(), *epilogue, _lib.ptr(residual), out.data_ptr()), (b, cin, h, w, cout, k, self.act)
        elif s2b_out:
            name, tag, wimg, wino = "dv_conv2d_wino_s2b_f32", tag + "_s2b", self.wino_packed, True
            args, tail = (*cat_args(parts), wimg.data_ptr(), *epilogue, out.data_ptr()), (b, h, w, cout, self.act)
        elif self.wino_packed is not None and d <= self.WINO_MAX_DILATION and \
                group * d * d * (-(-(-(-h // d)) // 16)) * (-(-(-(-w // d)) // 16)) * (-(-cout // 32)) >= self.WINO_MIN_BLOCKS:
            name, wimg, wino = "dv_conv2d_wino_dil_cat_f32", self.wino_packed, True
            ks = lib.dv_conv2d_wino_auto_kslices(cin, h, w, cout, d) if (self.KSPLIT and group == 1) else 1
            if ks > 1:        # (see Conv2dPairPlan)
                name, tag = "dv_conv2d_wino_cat_ksplit_f32", tag + "_wksplit"
            args = (*cat_args(parts), wimg.data_ptr(), *epilogue, *gates)
            tail = (b, h, w, cout, d, self.act)
        else:
            # launches too small to fill the chip (a single IGEV pair at 1/8 and 1/16 resolution): K-split over the input
            # channels, partial tiles in a scratch buffer, fused epilogue in the reduction kernel
            ks = lib.dv_conv2d_auto_kslices(1, cin, h, w, cout, k, d) if self.KSPLIT else 1     # (one batch item: see above)
            if ks > 1:
                name, tag = "dv_conv2d_cat_ksplit_f32", tag + "_ksplit"
            elif cat:
                name = "dv_conv2d_cat_f32"
            else:
                name = "dv_conv2d_gated_f32"
            args = ((x.data_ptr(),) if name == "dv_conv2d_gated_f32" else cat_args(parts)) + (wimg.data_ptr(), *epilogue, *gates)
            tail = ((b, cin) if name == "dv_conv2d_gated_f32" else (b,)) + (h, w, cout, k, d, self.act)
        if ks > 1:
            scratch = torch.empty(ks * out.numel(), dtype=torch.float32, device=x.device)
            args += (scratch.data_ptr(), ks)
        flops = 2.0 * out.numel() * cin * k ** 2
        nb = 4.0 * (sum(t.numel() for t in parts) + out.numel() * (1 + extra + (2 * ks if ks > 1 else 0)))
        _lib.timed_launch(tag, flops, nb, name, x.device, *args, *tail, issued=flops / WINO_MULT_REDUCTION if wino else flops)
        return out


class Deconv3dPlan:
    """ConvTranspose3d(stride 2, padding 1, bias=False) + BatchNorm3d (eval) + skip add + activation that
    doubles every dimension: kernel 3 with output_padding 1 (acv_ddim.py:74-80, :91-92) or kernel 4
    (IGEV hourglass, igev_stereo_ddim.py:44-51).

    ``redir=(weight [Cout,Cskip,1,1,1], bn)``: the hourglass's 1x1x1 skip convolution + BN
    (acv_ddim.py:81-86).  Then ``plan(x, skip=t)`` computes ``act(BN(deconv(x)) + BN_r(conv1x1(t)))`` in one
    launch (both BN scales folded into the weights, the 1x1x1 product accumulated as extra K-steps); shapes the
    fused kernel does not take fall back to the two-launch form."""

    def __init__(self, weight: torch.Tensor, bn: Optional[Tuple[torch.Tensor, ...]] = None,
                 act: int = ACT_NONE, eps: float = 1e-5, redir=None, redir_eps: float = 1e-5):
        w = _dev_f32(weight.detach(), "weight")
        self.cin, self.cout, k = w.shape[0], w.shape[1], w.shape[2]
        if tuple(w.shape[2:]) != (k, k, k) or k not in (3, 4):
            raise _lib.DiffuVolumeError("transposed convolutions: k3 s2 p1 op1 and k4 s2 p1 are implemented")
        self.k, self.act = k, act
        stem = "dv_deconv3d" if k == 3 else "dv_deconv3d_k4"
        self.scale, self.shift = _fold_bn(bn, None, self.cout, w.device, eps)
        self.redir_w = self.redir_plan = None
        if redir is not None:
            if k != 3:
                raise _lib.DiffuVolumeError("the fused skip convolution exists for the kernel-3 flavour")
            rw, rbn = redir
            rw = _dev_f32(rw.detach(), "redir weight")
            if rw.shape[0] != self.cout or tuple(rw.shape[2:]) != (1, 1, 1):
                raise _lib.DiffuVolumeError("redir must be a 1x1x1 convolution onto the deconvolution's channels")
            self.cskip = rw.shape[1]
            rscale, rshift = _fold_bn(rbn, None, self.cout, w.device, redir_eps)
            one = torch.ones(self.cout, device=w.device)
            zero = torch.zeros(self.cout, device=w.device)
            sd, sr = (one if self.scale is None else self.scale), (one if rscale is None else rscale)
            # fold both BN scales into the weights; the fused kernel then needs a single accumulator
            w = w * sd.view(1, -1, 1, 1, 1)
            self.redir_w = (rw.reshape(self.cout, self.cskip) * sr.view(-1, 1)).contiguous()
            self.shift = ((zero if self.shift is None else self.shift) + (zero if rshift is None else rshift)).contiguous()
            self.scale = None
            self.redir_plan = Conv3dPlan(self.redir_w.view(self.cout, self.cskip, 1, 1, 1), None, stride=1, act=ACT_NONE,
                                         precision="f32")       # two-launch fallback
        self.wpacked = pack(stem + "_packed_floats", stem + "_pack_weights_f32", w.contiguous(), self.cin, self.cout)

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None,
                 skip: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = _dev_f32(x, "x")
        b, cin, d, h, w = x.shape
        if cin != self.cin:
            raise RuntimeError(f"expected {self.cin} input channels, got {cin}")
        out = torch.empty((b, self.cout, 2 * d, 2 * h, 2 * w), dtype=torch.float32, device=x.device)
        if skip is not None:
            if self.redir_w is None or residual is not None:
                raise RuntimeError("skip= needs a plan built with redir=, and excludes residual=")
            skip = same_shape(skip, (b, self.cskip, 2 * d, 2 * h, 2 * w), "skip")
            if w % 2 == 0 and (self.cskip + 7) // 8 <= (cin + 7) // 8:
                flops = 2.0 * x.numel() * self.cout * 27 + 2.0 * out.numel() * self.cskip
                _lib.timed_launch("deconv3d_k3s2_redir", flops, 4.0 * (x.numel() + out.numel() + skip.numel()),
                                  "dv_deconv3d_k3s2_redir_f32", x.device, x.data_ptr(), self.wpacked.data_ptr(), _lib.ptr(self.shift),
                                  skip.data_ptr(), self.redir_w.data_ptr(), out.data_ptr(), b, cin, d, h, w, self.cout, self.cskip,
                                  self.act, issued=flops)
                return out
            residual = self.redir_plan(skip)
        residual = same_shape(residual, out, "residual")
        flops = 2.0 * x.numel() * self.cout * self.k ** 3
        _lib.timed_launch(f"deconv3d_k{self.k}s2", flops, 4.0 * (x.numel() + out.numel() * (1 if residual is None else 2)),
                          f"dv_deconv3d_k{self.k}s2_f32", x.device, x.data_ptr(), self.wpacked.data_ptr(), _lib.ptr(self.scale),
                          _lib.ptr(self.shift), _lib.ptr(residual), out.data_ptr(), b, cin, d, h, w, self.cout, self.act, issued=flops)
        return out


def _fold_bn(bn, bias, cout, device, eps):
    """Eval-mode BatchNorm -> per-channel (scale, shift); a conv bias folds into shift."""
    if bn is None and bias is None:
        return None, None
    if bn is None:
        return None, bias.detach().to(device=device, dtype=torch.float32).contiguous()
    gamma, beta, mean, var = (t.detach().to(device=device, dtype=torch.float32) for t in bn)
    scale = gamma / torch.sqrt(var + eps)
    shift = beta - mean * scale
    if bias is not None:
        shift = shift + bias.detach().to(device=device, dtype=torch.float32) * scale
    return scale.contiguous(), shift.contiguous()

