"""The host side of the DDIM sampler, written once for the ACV, PCW and IGEV flavours.

Every DDIM step of all three runs through ``dv_noise_prepare_f32/f64``, ``dv_ddim_step`` and ``dv_encode_two_hot_f32``
with one coefficient struct, ``DvDdimCoef``.  This module owns what drives them: the twelve float64 schedule buffers of
the reference modules, the float64 tables derived from ``alphas_cumprod``, the time list, the coefficient builder, the
launchers, the loop plan (per-step constants kept on the device) and the argument checks in front of the loop.  The
flavours differ in four thresholds and in which of ``unc`` / ``coords0`` the state update reads.
"""
from __future__ import annotations

import ctypes
import math
from typing import Callable, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from .plans import settle_build

NoiseFn = Callable[[str, Tuple[int, ...], torch.dtype], torch.Tensor]

# buffer names and order of the reference modules (acv_ddim.py:147-172): the order of their state_dict keys
SCHEDULE_BUFFERS = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod",
                    "log_one_minus_alphas_cumprod", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
                    "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2")


def cosine_beta_schedule(timesteps: int, s: float = 0.008) -> torch.Tensor:
    """acv_ddim.py:113-119 (float64)."""
    x = torch.linspace(0, timesteps, timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / timesteps) + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


def register_schedule(module: torch.nn.Module, num_timesteps: int) -> None:
    """The float64 schedule buffers of a reference ``*_ddim`` module, under its names and in its order."""
    betas = cosine_beta_schedule(num_timesteps)
    alphas = 1.0 - betas
    ac = torch.cumprod(alphas, dim=0)
    ac_prev = F.pad(ac[:-1], (1, 0), value=1.0)
    post_var = betas * (1.0 - ac_prev) / (1.0 - ac)
    values = (betas, ac, ac_prev, torch.sqrt(ac), torch.sqrt(1.0 - ac), torch.log(1.0 - ac), torch.sqrt(1.0 / ac),
              torch.sqrt(1.0 / ac - 1), post_var, torch.log(post_var.clamp(min=1e-20)),
              betas * torch.sqrt(ac_prev) / (1.0 - ac), (1.0 - ac_prev) * torch.sqrt(alphas) / (1.0 - ac))
    for name, val in zip(SCHEDULE_BUFFERS, values):
        module.register_buffer(name, val)


class Tables:
    """What the sampler reads of the schedule, in float64 on the host, and the loop-plan cache (`loop_plan`).

    ACV and PCW build it from the module's ``alphas_cumprod`` buffer, which a checkpoint may have overwritten; the IGEV
    loop, which holds no module, builds it from ``cosine_beta_schedule(1000)``."""

    def __init__(self, alphas_cumprod: torch.Tensor):
        ac = alphas_cumprod.detach().double().cpu()
        self.alphas_cumprod = ac
        self.sqrt_ac, self.sqrt_1mac = torch.sqrt(ac), torch.sqrt(1.0 - ac)
        self.sqrt_recip, self.sqrt_recipm1 = torch.sqrt(1.0 / ac), torch.sqrt(1.0 / ac - 1)
        self.loop_key = self.loop_steps = None

    def q_fill(self, time: int, asd: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
        """q_sample(asd, time) with the draw ``q``, in float64 (float64 schedule buffers in the reference).  The bits of
        ``x_next`` depend on this order of operations."""
        return self.sqrt_ac[time].item() * asd.double() + self.sqrt_1mac[time].item() * q.double()


def time_pairs(num_timesteps: int, sampling_timesteps: int) -> List[Tuple[int, int]]:
    """acv_ddim.py:306-308: [(T-1, ...), ..., (..., -1)]."""
    times = torch.linspace(-1, num_timesteps - 1, steps=sampling_timesteps + 1)
    times = list(reversed(times.int().tolist()))
    return list(zip(times[:-1], times[1:]))


def step_coef(tables: Tables, time: int, time_next: int, cof: float, *, eta: float, dif_thr: float, unc_thr: float,
              clamp_max: float, ens_dif_thr: float) -> _lib.DvDdimCoef:
    """The struct ``dv_ddim_step`` takes by value (acv_ddim.py:348-352 in float64).  ACV and PCW: their renewal
    thresholds, ``clamp_max = maxdisp - 1``, no output rule (0.0).  IGEV: dif < 5, no uncertainty test (inf),
    clamp(pred, 0, 48 - 1), output rule dif < 3."""
    k = _lib.DvDdimCoef()
    k.sqrt_recip_alpha, k.sqrt_recipm1_alpha = float(tables.sqrt_recip[time]), float(tables.sqrt_recipm1[time])
    k.dif_thr, k.unc_thr, k.cof, k.last = dif_thr, unc_thr, cof, int(time_next < 0)
    k.clamp_max, k.ens_dif_thr = clamp_max, ens_dif_thr
    if time_next >= 0:
        alpha, alpha_next = tables.alphas_cumprod[time], tables.alphas_cumprod[time_next]
        sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
        k.sigma, k.c = float(sigma), float((1 - alpha_next - sigma ** 2).sqrt())
        k.sqrt_alpha_next = float(alpha_next.sqrt())
    return k


def noise_prepare(time_embedding, x_t: torch.Tensor, t: Optional[torch.Tensor], shift: Optional[torch.Tensor] = None):
    """time shift + clamp + [0,1] (head.py:74-77, acv_ddim.py:256-258) -> (n01 in the state's dtype, n01 fp32).
    ``shift`` [B,C]: the time MLP's output when it was precomputed for this step (`loop_plan`)."""
    if x_t.dtype not in (torch.float32, torch.float64):
        raise TypeError("the DDIM state is float32 (first step) or float64")
    b, c, h, w = x_t.shape
    if shift is None:
        shift = time_embedding.shift(t).float().contiguous()
    x_t = x_t.contiguous()
    n01 = torch.empty_like(x_t)
    if x_t.dtype == torch.float32:
        _lib.launch("dv_noise_prepare_f32", x_t.device, x_t.data_ptr(), shift.data_ptr(), n01.data_ptr(), b, c, h * w)
        return n01, n01
    n01f = torch.empty(x_t.shape, dtype=torch.float32, device=x_t.device)
    _lib.launch("dv_noise_prepare_f64", x_t.device, x_t.data_ptr(), shift.data_ptr(), n01.data_ptr(), n01f.data_ptr(), b, c, h * w)
    return n01, n01f


def train_filter(sqrt_alphas_cumprod: torch.Tensor, sqrt_one_minus_alphas_cumprod: torch.Tensor, time_embedding, scale: float,
                 num_timesteps: int, x_start: torch.Tensor) -> torch.Tensor:
    """The volume filter of a training step of ACV and PCW (acv_ddim.py:441-451, pwcnet_ddim.py:661-669): draws
    ``t = torch.randint(0, T, (1,))`` and then q_sample's ``torch.randn_like`` (in that order), q_sample with the model's
    schedule buffers, the time embedding, clamp, [0,1] -> [B,1,D,h,w] float32.  No gradient reaches ``time_embedding``
    (the reference's ``torch.tensor(noisy)``)."""
    t = torch.randint(0, num_timesteps, (1,), device=x_start.device).long()
    noise = torch.randn_like(x_start)
    with torch.no_grad():
        noisy = (sqrt_alphas_cumprod.gather(-1, t).reshape(-1, 1, 1, 1) * x_start
                 + sqrt_one_minus_alphas_cumprod.gather(-1, t).reshape(-1, 1, 1, 1) * noise)
        noisy = time_embedding(noisy, t)
        noisy = torch.clamp(noisy, min=-1 * scale, max=scale)
        noisy = ((noisy / scale) + 1) / 2.
        return noisy.unsqueeze(1).to(torch.float32)


def ddim_update(disp, used, n01, eps, fill, mask, ens, coef: _lib.DvDdimCoef, *, unc=None, coords0=None,
                want_pred_noise=False):
    """``dv_ddim_step``: two-hot x_start of ``disp``, renewal mask, ensemble and the next state -> (x_start fp32,
    x_next fp64 | None on the last step, pred_noise fp64 | None).  ``unc``: the uncertainty ACV and PCW test;
    ``coords0``: the x coordinates IGEV's disparity is measured from."""
    b, c, h, w = n01.shape
    dev = disp.device
    x_start = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
    x_next = None if coef.last else torch.empty((b, c, h, w), dtype=torch.float64, device=dev)
    pred_noise = torch.empty((b, c, h, w), dtype=torch.float64, device=dev) if want_pred_noise else None
    f32 = n01.dtype == torch.float32
    eps32 = eps if (eps is not None and eps.dtype == torch.float32) else None
    eps64 = eps if (eps is not None and eps.dtype == torch.float64) else None
    _lib.launch("dv_ddim_step", dev, disp.data_ptr(), _lib.ptr(unc), used.data_ptr(), _lib.ptr(coords0),
                n01.data_ptr() if f32 else 0, 0 if f32 else n01.data_ptr(), _lib.ptr(eps32), _lib.ptr(eps64), _lib.ptr(fill),
                mask.data_ptr(), x_start.data_ptr(), _lib.ptr(pred_noise), _lib.ptr(x_next), _lib.ptr(ens), b, c, h, w,
                ctypes.byref(coef))
    return x_start, x_next, pred_noise


def encode_two_hot(disp: torch.Tensor, bins: int) -> torch.Tensor:
    """Quarter-resolution disparity [B,1,h,w] (float32, contiguous, on the device) -> two-hot [B,bins,h,w] in [-1,1]
    (acv_ddim.py:403-419)."""
    b, h, w = disp.shape[0], disp.shape[-2], disp.shape[-1]
    x = torch.empty((b, bins, h, w), dtype=torch.float32, device=disp.device)
    _lib.launch("dv_encode_two_hot_f32", disp.device, disp.data_ptr(), x.data_ptr(), b, bins, h * w)
    return x


class _LoopStep:
    """Everything one DDIM step needs that depends only on its timestep: the coefficient struct handed to
    ``dv_ddim_step`` by value and the time-MLP shift (device resident; one row per batch entry on demand)."""

    def __init__(self, time: int, time_next: int, coef: _lib.DvDdimCoef, shift: torch.Tensor):
        self.time, self.time_next, self.coef, self.shift = time, time_next, coef, shift
        self._rows = {}

    def shift_rows(self, b: int) -> torch.Tensor:
        if b not in self._rows:
            rows = self.shift.reshape(1, -1).expand(b, -1).contiguous()
            settle_build(rows.device)          # kept for every later caller, whatever its stream
            self._rows[b] = rows
        return self._rows[b]


def loop_plan(model, tables: Tables, device) -> List[_LoopStep]:
    """Per-step constants of ``model.ddim_sample`` (ACVNet_DDIM / PWCNet_ddim): the coefficients of acv_ddim.py:306-308,
    :348-352 and the time MLP of head.py:74-75, which sees nothing but ``t``.  Computed once per (weights, step list) and
    kept on the device, so the loop itself launches no time-MLP kernels and copies no scalars."""
    key = (model.sampling_timesteps, model.ensemble_cof, model.dif_threshold, model.unc_threshold,
           model.ddim_sampling_eta, model.num_timesteps)
    if tables.loop_key != key:
        steps = []
        for i, (time, time_next) in enumerate(time_pairs(model.num_timesteps, model.sampling_timesteps)):
            t = torch.full((1,), time, device=device, dtype=torch.long)
            shift = model.time_embedding.shift(t).float().reshape(-1).contiguous()
            steps.append(_LoopStep(time, time_next, model._step_coef(time, time_next, model.ensemble_cof[i + 1]), shift))
        settle_build(device)                   # the shifts are kept for every later caller, whatever its stream
        tables.loop_steps, tables.loop_key = steps, key
    return tables.loop_steps


def check_loop_args(volume, used: torch.Tensor, x_T: torch.Tensor, maxdisp: int, what: str = "volume") -> torch.Tensor:
    """Shapes the kernels index by: used / disp / ens are [B,4h,4w] for a [B,C,maxdisp/4,h,w] volume (the reference
    fails with a broadcast error at ``disp - used``, acv_ddim.py:322).  Returns ``used`` as [B,4h,4w]."""
    b, _, d, h, w = volume.shape
    if d != maxdisp // 4:
        raise RuntimeError(f"the {what} must have {maxdisp // 4} disparity bins, got {d}")
    if used.numel() != b * 16 * h * w or tuple(used.shape[-2:]) != (4 * h, 4 * w):
        raise RuntimeError(f"The size of tensor a {(b, 4 * h, 4 * w)} must match the size of tensor b "
                           f"{tuple(used.shape)}: `used` must be the full-resolution disparity of the volume")
    if tuple(x_T.shape) != (b, d, h, w):
        raise RuntimeError(f"x_T must be {(b, d, h, w)}, got {tuple(x_T.shape)}")
    return used.reshape(b, 4 * h, 4 * w)


def make_draw(noise: Optional[NoiseFn], generator: Optional[torch.Generator], device):
    """``draw(kind, shape, dtype)``: a random draw of the loop, from ``noise(kind, shape, dtype)`` when the caller injects
    them (parity tests), else from the device generator: 'fill' (ACV's rand_like, acv_ddim.py:360) uniform, every other
    kind ('x_T', 'eps', 'q') normal."""
    def draw(kind, shape, dtype):
        if noise is not None:
            return noise(kind, shape, dtype).to(device=device, dtype=dtype).contiguous()
        fn = torch.rand if kind == "fill" else torch.randn
        return fn(shape, device=device, dtype=dtype, generator=generator)
    return draw
