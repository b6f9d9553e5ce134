"""IGEV geometry-encoding-volume lookup with the DiffuVolume noise filter, behind the
reference's class API (KITTI15/core/geometry_ddim.py:6-80).

``Combined_Geo_Encoding_Volume(init_fmap1, init_fmap2, geo_volume, num_levels=2, radius=4)``
then ``corr_fn(disp, coords, noisy) -> [B, 162, h, w]`` once per GRU iteration.  The lookup,
the `geo_volume * noise` multiply and both level-1 poolings are one HIP kernel
(``dv_geo_filter_lookup_f32``); the all-pairs correlation of ``__init__`` (one GEMM per image
row, once per pair) and its pooled level are a second one (``dv_allpairs_corr_f32``).

Training.  When autograd is recording and ``init_fmap1``, ``init_fmap2`` or ``geo_volume`` requires grad, the volume is on
the TRAINING ROUTE: the correlation is ``AllPairsCorrFn`` (forward ``dv_allpairs_corr_f32``, backward
``dv_allpairs_corr_bwd_f32``; the pooled level is non-differentiable, its share is folded into corr0's gradient) and every
``corr_fn(disp, coords, noisy)`` is ``GeoLookupFn``: the inference launch forward, ``dv_geo_filter_lookup_bwd_f32``
backward -- the lookup is linear in the volume and in the correlation rows, so nothing but ``disp``, ``coords`` and
``noisy`` is saved.  Those three are not differentiable (the reference detaches them, KITTI15/core/igev_stereo_ddim.py:436
``torch.tensor(noisy)`` and :442 ``disp.detach()``): one that requires grad raises.  The T dense volume gradients of T
lookups are summed by autograd.  ``DV_TRAIN_LOOKUP=torch`` swaps both functions for torch expressions (A/B runs, tests).
"""
from __future__ import annotations

import functools

import torch
import torch.nn.functional as F

from . import _env, _lib
from .plans import _dev_f32, pack
from .submodule import _wants_grad

route = functools.partial(_env.route, "DV_TRAIN_LOOKUP")     # what the training route of the lookup and the correlation runs on


def _checked(t, name: str) -> torch.Tensor:
    """The hot path's device / dtype checks for a tensor that may require grad; contiguous, still attached."""
    _dev_f32(t.detach() if isinstance(t, torch.Tensor) else t, name)
    return t.contiguous()


class AllPairsCorrFn(torch.autograd.Function):
    """(corr0, corr1) of two feature maps on ``dv_allpairs_corr_f32``.  corr1 = avg_pool(corr0) is marked
    non-differentiable: its consumer, the lookup's backward, adds the pooled level's share to corr0's gradient itself."""

    @staticmethod
    def forward(ctx, fmap1, fmap2):
        corr0, corr1 = Combined_Geo_Encoding_Volume._corr_levels(fmap1, fmap2)
        ctx.save_for_backward(fmap1, fmap2)
        ctx.mark_non_differentiable(corr1)
        return corr0, corr1

    @staticmethod
    def backward(ctx, g0, _g1):
        f1, f2 = ctx.saved_tensors
        g0 = _dev_f32(g0, "corr0 gradient")
        B, C, H, W1 = f1.shape
        W2 = f2.shape[-1]
        d1 = torch.empty_like(f1) if ctx.needs_input_grad[0] else None
        d2 = torch.empty_like(f2) if ctx.needs_input_grad[1] else None
        if d1 is None and d2 is None:
            return None, None
        n = (d1 is not None) + (d2 is not None)
        _lib.timed_launch("allpairs_corr_bwd", 2.0 * n * B * H * W1 * W2 * C,
                          4.0 * (n * g0.numel() + (f2.numel() + f1.numel() if d1 is not None else 0)
                                 + (f1.numel() + f2.numel() if d2 is not None else 0)),
                          "dv_allpairs_corr_bwd_f32", g0.device, g0.data_ptr(), f1.data_ptr(), f2.data_ptr(), _lib.ptr(d1),
                          _lib.ptr(d2), B, C, H, W1, W2, issued=2.0 * n * B * H * W1 * W2 * C)
        return d1, d2


class GeoLookupFn(torch.autograd.Function):
    """One lookup of a training-route volume: the inference launch, and ``dv_geo_filter_lookup_bwd_f32`` for the
    gradients of the geometry volume and of corr0 (each only if asked for)."""

    @staticmethod
    def forward(ctx, volume, geo, corr0, disp, coords, noisy):
        ctx.save_for_backward(disp, coords, noisy)
        ctx.dims = (*geo.shape, corr0.shape[-1], volume.radius)
        return Combined_Geo_Encoding_Volume._lookup(geo, corr0, volume.corr1, disp, coords, noisy, volume.radius)

    @staticmethod
    def backward(ctx, g):
        disp, coords, noisy = ctx.saved_tensors
        b, c, d, h, w, w2, radius = ctx.dims
        g = _dev_f32(g, "lookup gradient")
        dgeo = torch.empty((b, c, d, h, w), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[1] else None
        dcorr0 = torch.empty((b, h, w, w2), dtype=torch.float32, device=g.device) if ctx.needs_input_grad[2] else None
        if dgeo is not None or dcorr0 is not None:
            nbytes = 4.0 * (g.numel() + (dgeo.numel() + noisy.numel() if dgeo is not None else 0)
                            + (dcorr0.numel() if dcorr0 is not None else 0))
            _lib.timed_launch("geo_filter_lookup_bwd", 0.0, nbytes, "dv_geo_filter_lookup_bwd_f32", g.device, g.data_ptr(),
                              disp.data_ptr(), coords.data_ptr(), noisy.data_ptr(), _lib.ptr(dgeo), _lib.ptr(dcorr0),
                              b, c, d, h, w, w2, radius)
        return None, dgeo, dcorr0, None, None, None


def _sample_rows(rows: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """rows [N,C,L] linearly sampled at the pixel positions x [N,T] -> [N,C,T]: the reference's bilinear_sampler over
    grid_sample(align_corners=True, zero padding) along one axis (KITTI15/core/utils/utils.py:59-77), normalise /
    unnormalise round trip included."""
    L = rows.shape[-1]
    ix = (((2 * x / (L - 1) - 1) + 1) / 2) * (L - 1)
    fl = torch.floor(ix)
    i0 = fl.long()
    padded = F.pad(rows, (1, 1))                                            # entries -1 and L are the zero padding
    shape = (-1, rows.shape[1], -1)
    v0 = torch.gather(padded, 2, (i0.clamp(-1, L) + 1).unsqueeze(1).expand(*shape))
    v1 = torch.gather(padded, 2, ((i0 + 1).clamp(-1, L) + 1).unsqueeze(1).expand(*shape))
    return v0 * ((fl + 1) - ix).unsqueeze(1) + v1 * (ix - fl).unsqueeze(1)


def torch_lookup(geo_volume, corr0, disp, coords, noisy, radius: int = 4, num_levels: int = 2) -> torch.Tensor:
    """The lookup as differentiable torch operations (geometry_ddim.py:33-69 on the pyramids of :19-30): the
    ``DV_TRAIN_LOOKUP=torch`` route.  corr0 [B,h,w,W2]."""
    b, c, d, h, w = geo_volume.shape
    n = b * h * w
    geo = geo_volume.permute(0, 3, 4, 1, 2).reshape(n, c, d)
    corr = corr0.reshape(n, 1, -1)
    noi = noisy.reshape(n, 1, d)                                           # the raw reshape of :37
    dx = torch.linspace(-radius, radius, 2 * radius + 1, dtype=disp.dtype, device=disp.device).view(1, -1)
    dflat, cflat = disp.reshape(n, 1), coords.reshape(n, 1)
    outs = []
    for i in range(num_levels):
        outs.append(_sample_rows(geo * noi, dflat / 2 ** i + dx).reshape(n, -1))
        outs.append(_sample_rows(corr, cflat / 2 ** i - dflat / 2 ** i + dx).reshape(n, -1))
        geo, corr, noi = (F.avg_pool1d(t, 2, 2) for t in (geo, corr, noi))
    return torch.cat(outs, dim=-1).view(b, h, w, -1).permute(0, 3, 1, 2).contiguous()


class GeoLookupRequest:
    """A lookup that has not run yet: what `Combined_Geo_Encoding_Volume.request` hands to this build's update block, whose
    motion encoder consumes the lookup through ONE 1x1 convolution (BasicMotionEncoder.convc1, KITTI15/core/update.py:79,:89)
    and can therefore ask for `conv1x1` -- lookup and convolution in one kernel, the [B,162,h,w] tensor never written.
    `materialize()` is the plain lookup (what the reference's `corr_fn(...)` returns)."""

    def __init__(self, volume, disp, coords, noisy):
        self.volume, self.disp, self.coords, self.noisy = volume, disp, coords, noisy

    def materialize(self) -> torch.Tensor:
        return self.volume(self.disp, self.coords, self.noisy)

    def conv1x1(self, wpacked: torch.Tensor, bias, act: int) -> torch.Tensor:
        return self.volume.lookup_conv1x1(self.disp, self.coords, self.noisy, wpacked, bias, act)


def pack_lookup_conv1x1(weight: torch.Tensor, channel: int = 8) -> torch.Tensor:
    """nn.Conv2d(2*(9*channel+9), 64, 1).weight -> the layout `dv_geo_filter_lookup_conv1x1_f32` reads."""
    w = _dev_f32(weight.detach().reshape(weight.shape[0], -1), "weight")
    if tuple(w.shape) != (64, 2 * (9 * channel + 9)):
        raise _lib.DiffuVolumeError(f"fused lookup + 1x1 convolution: weight [64, {2 * (9 * channel + 9)}], got {tuple(w.shape)}")
    return pack("dv_geo_lookup_conv1x1_packed_floats", "dv_geo_lookup_conv1x1_pack_weights_f32", w, channel)


class Combined_Geo_Encoding_Volume:
    def __init__(self, init_fmap1, init_fmap2, geo_volume, num_levels=2, radius=4):
        if num_levels != 2 or radius != 4:
            raise _lib.DiffuVolumeError("the HIP lookup implements num_levels=2, radius=4 (every IGEV config)")
        self.num_levels, self.radius = num_levels, radius
        self.training_route = _wants_grad(init_fmap1, init_fmap2, geo_volume)
        if self.training_route:
            self.geo_volume = _checked(geo_volume, "geo_volume")
            f1, f2 = _checked(init_fmap1, "init_fmap1"), _checked(init_fmap2, "init_fmap2")
            if f1.dim() != 4 or f2.shape[:3] != f1.shape[:3]:
                raise RuntimeError(f"feature maps must agree in batch, channels and height: {tuple(f1.shape)} vs {tuple(f2.shape)}")
            if route() == "torch":
                self.corr0 = torch.einsum("aijk,aijh->ajkh", f1, f2).contiguous()
                self.corr1 = F.avg_pool2d(self.corr0, [1, 2], stride=[1, 2])
            elif _wants_grad(f1, f2):
                self.corr0, self.corr1 = AllPairsCorrFn.apply(f1, f2)
            else:                                                            # frozen features: nothing to differentiate
                self.corr0, self.corr1 = self._corr_levels(f1, f2)
        else:
            self.geo_volume = _dev_f32(geo_volume, "geo_volume")             # [B,C,D,h,w], no permuted copy
            self.corr0, self.corr1 = self._corr_levels(_dev_f32(init_fmap1, "init_fmap1"), _dev_f32(init_fmap2, "init_fmap2"))
        self.channel = self.geo_volume.shape[1]

    def _differentiating(self, disp, coords, noisy) -> bool:
        """True when this call is recorded by autograd (a training-route volume with grad mode on).  The sample positions
        and the noise have no gradient here, as in the reference: asking for one is an error, never a silent None."""
        if not (self.training_route and torch.is_grad_enabled()):
            return False
        for t, name in ((disp, "disp"), (coords, "coords"), (noisy, "noisy")):
            if isinstance(t, torch.Tensor) and t.requires_grad:
                raise _lib.DiffuVolumeError(
                    f"{name} requires grad: the geometry lookup is differentiable in geo_volume and the feature maps only; "
                    "the reference detaches the rest (KITTI15/core/igev_stereo_ddim.py:436 `torch.tensor(noisy)`, :442 "
                    "`disp.detach()`) -- detach it before the lookup")
        return True

    def __call__(self, disp, coords, noisy):
        train = self._differentiating(disp, coords, noisy)
        disp = _dev_f32(disp, "disp")
        coords = _dev_f32(coords, "coords")
        noisy = _dev_f32(noisy, "noisy")
        b, c, d, h, w = self.geo_volume.shape
        if disp.numel() != b * h * w or coords.numel() != b * h * w or noisy.numel() != b * h * w * d:
            raise RuntimeError("disp/coords must be [B,1,h,w] and noisy [B,D,h,w] for this volume")
        if train and route() == "torch":
            return torch_lookup(self.geo_volume, self.corr0, disp, coords, noisy, self.radius, self.num_levels)
        if train:
            return GeoLookupFn.apply(self, self.geo_volume, self.corr0, disp, coords, noisy)
        return self._lookup(self.geo_volume, self.corr0, self.corr1, disp, coords, noisy, self.radius)

    @staticmethod
    def _lookup(geo, corr0, corr1, disp, coords, noisy, radius):
        """The inference launch: [B, 2*(9C+9), h, w]."""
        b, c, d, h, w = geo.shape
        nch = 2 * (c * (2 * radius + 1) + (2 * radius + 1))
        out = torch.empty((b, nch, h, w), dtype=torch.float32, device=disp.device)
        _lib.timed_launch("geo_filter_lookup", 0.0, 4.0 * (out.numel() + noisy.numel()), "dv_geo_filter_lookup_f32", disp.device,
                          geo.data_ptr(), corr0.data_ptr(), corr1.data_ptr(), disp.data_ptr(), coords.data_ptr(), noisy.data_ptr(),
                          out.data_ptr(), b, c, d, h, w, corr0.shape[-1], radius)
        return out

    def request(self, disp, coords, noisy) -> GeoLookupRequest:
        return GeoLookupRequest(self, disp, coords, noisy)

    def lookup_conv1x1(self, disp, coords, noisy, wpacked, bias, act):
        """act(conv1x1(lookup(disp, coords, noisy)) + bias) -> [B,64,h,w] in one launch (`pack_lookup_conv1x1` weights)."""
        if self.training_route and torch.is_grad_enabled():
            raise _lib.DiffuVolumeError("the fused lookup + 1x1 convolution is inference-only and this volume is on the "
                                        "training route: use request(...).materialize() (update.py does in train mode), "
                                        "or call it under torch.no_grad()")
        disp = _dev_f32(disp, "disp")
        coords = _dev_f32(coords, "coords")
        noisy = _dev_f32(noisy, "noisy")
        b, c, d, h, w = self.geo_volume.shape
        if disp.numel() != b * h * w or coords.numel() != b * h * w or noisy.numel() != b * h * w * d:
            raise RuntimeError("disp/coords must be [B,1,h,w] and noisy [B,D,h,w] for this volume")
        nch = 2 * (c * (2 * self.radius + 1) + (2 * self.radius + 1))
        out = torch.empty((b, 64, h, w), dtype=torch.float32, device=disp.device)
        fl = 2.0 * out.numel() * nch
        _lib.timed_launch("geo_filter_lookup_conv1x1", fl, 4.0 * (out.numel() + noisy.numel()), "dv_geo_filter_lookup_conv1x1_f32",
                          disp.device, self.geo_volume.data_ptr(), self.corr0.data_ptr(), self.corr1.data_ptr(), disp.data_ptr(),
                          coords.data_ptr(), noisy.data_ptr(), wpacked.data_ptr(), _lib.ptr(bias), out.data_ptr(), b, c, d, h, w,
                          self.corr0.shape[-1], self.radius, 64, act, issued=fl * 20.0 / 18.0)
        return out

    @staticmethod
    def _corr_levels(fmap1, fmap2):
        """corr0 [B,H,W1,W2] and its avg_pool2d([1,2]) level corr1 [B,H,W1,W2//2] in one launch."""
        B, C, H, W1 = fmap1.shape
        if fmap2.shape[:3] != fmap1.shape[:3]:
            raise RuntimeError(f"feature maps must agree in batch, channels and height: {tuple(fmap1.shape)} vs {tuple(fmap2.shape)}")
        W2 = fmap2.shape[-1]
        corr0 = torch.empty((B, H, W1, W2), dtype=torch.float32, device=fmap1.device)
        corr1 = torch.empty((B, H, W1, W2 // 2), dtype=torch.float32, device=fmap1.device)
        _lib.timed_launch("allpairs_corr", 2.0 * B * H * W1 * W2 * C, 4.0 * (fmap1.numel() + fmap2.numel() + corr0.numel() + corr1.numel()),
                          "dv_allpairs_corr_f32", fmap1.device, fmap1.data_ptr(), fmap2.data_ptr(), corr0.data_ptr(), corr1.data_ptr(),
                          B, C, H, W1, W2, issued=2.0 * B * H * W1 * W2 * C)
        return corr0, corr1

    @staticmethod
    def corr(fmap1, fmap2):
        """All-pairs correlation along the epipolar line (geometry_ddim.py:72-80): [B,H,W1,1,W2]."""
        fmap1, fmap2 = _dev_f32(fmap1, "fmap1"), _dev_f32(fmap2, "fmap2")
        corr0, _ = Combined_Geo_Encoding_Volume._corr_levels(fmap1, fmap2)
        B, H, W1, W2 = corr0.shape
        return corr0.reshape(B, H, W1, 1, W2)
