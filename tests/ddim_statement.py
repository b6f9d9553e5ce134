"""One DDIM state update of the reference, written once in plain torch with the reference's dtypes, and the bars the
kernels of csrc/ddim.hip are held to against it (tests/test_ddim_statement_host.py, tests/test_gpu_ddim_kernels.py).

The lines restated: SceneFlow/models/acv_ddim.py:272-294 and :318-362 (ACV, PCW), KITTI15/core/igev_stereo_ddim.py:265-272
and :316-327 (IGEV).  The coefficients have the shapes the reference gives them -- ``extract()`` returns [B,1,1,1] float64
tensors, ``alpha_next.sqrt()``, ``c`` and ``sigma`` are 0-dim float64 tensors -- and torch's own promotion produces the
dtypes: ``x_start * alpha_next.sqrt()`` stays float32, ``sigma * eps`` follows ``eps``, everything else is float64.  No
cast is written that the reference does not have.  It runs on whatever device its inputs are on.
"""
import torch

U64 = 2.0 ** -52    # float64 ulp of 1
U32 = 2.0 ** -23    # float32 ulp of 1


def down4(t):
    """``F.interpolate(t[:, None], size=(H/4, W/4), mode="bilinear")`` of a [B,H,W] tensor: with align_corners=False and an
    exact factor of 4 every weight is 0.5 and the taps are the central 2x2 of each 4x4 cell.  Spelled out in the order of
    ATen's GPU kernel, h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d): ATen's CPU kernel sums in another order."""
    a, b, c, d = t[:, 1::4, 1::4], t[:, 1::4, 2::4], t[:, 2::4, 1::4], t[:, 2::4, 2::4]
    return 0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d)


def two_hot(dq, nbins):
    """acv_ddim.py:277-290 in ``dq``'s dtype and on its device: [B,1,h,w] in [0, nbins) -> [B,nbins,h,w] in [0,1].  The
    operations of ``oracle.acv_oracle.encode_two_hot``, which is float32 on the CPU only."""
    b, _, h, w = dq.shape
    real = torch.floor(dq).long()
    coff = real - dq + 1
    vol = torch.zeros(b, nbins, h, w, dtype=dq.dtype, device=dq.device)
    vol = vol.view(b, nbins, -1).scatter_(1, real.view(b, 1, -1), coff.view(b, 1, -1)).reshape(b, nbins, h, w)
    vol = vol.view(b, nbins, -1).scatter_(1, torch.clamp(real + 1, 0, nbins - 1).view(b, 1, -1),
                                          (1 - coff).view(b, 1, -1)).reshape(b, nbins, h, w)
    last = torch.zeros(b, nbins, h, w, dtype=dq.dtype, device=dq.device)
    last[:, -1] = 1
    return torch.where(real == nbins - 1, last, vol)


def quarter_position(disp, coords0, clamp_max, nbins):
    """The position the two-hot encodes, [B,1,h,w]: acv_ddim.py:272-274; with ``coords0`` igev_stereo_ddim.py:268-273."""
    dq = down4(torch.clamp(disp, 0, clamp_max)).unsqueeze(1) / 4
    if coords0 is not None:
        dq = torch.clamp(coords0.unsqueeze(1) + dq, 0, nbins - 1)
    return dq


def output_rule(disp, used, k):
    """The disparity a step hands to the ensemble: IGEV's ``where(dif < 3, disp, used)`` (igev_stereo_ddim.py:324-326) when
    ``ens_dif_thr`` > 0, else ``disp`` itself (acv_ddim.py:318)."""
    return torch.where(torch.abs(disp - used) < k.ens_dif_thr, disp, used) if k.ens_dif_thr > 0 else disp


def ddim_step_statement(disp, unc, used, coords0, n01, eps, fill, mask0, ens0, k, nbins, all_float64=False):
    """What ``dv_ddim_step`` computes, from what it takes: disp, used [B,4h,4w] float32, unc the same or None, coords0
    [B,h,w] or None, n01 [B,nbins,h,w] float32 / float64 / None, eps the same, fill float64, mask0 [B,h,w], ens0 [B,4h,4w] or
    None, ``k`` a DvDdimCoef -> (x_start, pred_eps | None, mask, x_next | None, ens | None).

    ``all_float64``: pred_eps and x_next with every operand in float64, i.e. without the float32 rounding points of
    ``x_start * sqrt_alpha_next`` and ``sigma * eps``; x_start itself is the float32 tensor the reference scatters into.
    Only the self-check of the bars uses it."""
    b = disp.shape[0]
    dev = disp.device
    x_start = two_hot(quarter_position(disp, coords0, k.clamp_max, nbins), nbins)
    x_start = torch.clamp(x_start * 2 - 1., min=-1, max=1)
    # renewal mask (acv_ddim.py:322-338; igev_stereo_ddim.py:316-322 has no uncertainty test)
    dif = torch.abs(disp - used)
    keep = torch.where(dif < k.dif_thr, 1, 0)
    if unc is not None:
        keep = torch.where(unc < k.unc_thr, 1, 0) * keep
    mask = torch.clamp(mask0 + down4(keep.to(disp.dtype)), 0, 1)
    # ensemble term (acv_ddim.py:318, :366-368), after IGEV's output rule (igev_stereo_ddim.py:324-326)
    ens = None
    if ens0 is not None:
        ens = ens0 + output_rule(disp, used, k) * k.cof
    pred_eps = x_next = None
    if all_float64:
        x_start, n01, eps = (None if t is None else t.double() for t in (x_start, n01, eps))
    if n01 is not None:
        sr = torch.full((b, 1, 1, 1), k.sqrt_recip_alpha, dtype=torch.float64, device=dev)
        srm1 = torch.full((b, 1, 1, 1), k.sqrt_recipm1_alpha, dtype=torch.float64, device=dev)
        pred_eps = (sr * n01 - x_start) / srm1                                         # acv_ddim.py:249-252
    if not k.last:
        san = torch.tensor(k.sqrt_alpha_next, dtype=torch.float64, device=dev)
        c = torch.tensor(k.c, dtype=torch.float64, device=dev)
        sigma = torch.tensor(k.sigma, dtype=torch.float64, device=dev)
        img = x_start * san + c * pred_eps + sigma * eps                               # acv_ddim.py:356
        x_next = torch.where(mask.unsqueeze(1) == 0, fill, img)                        # acv_ddim.py:362
    return x_start, pred_eps, mask, x_next, ens


def noise_prepare_statement(x, shift):
    """head.py:74-77, acv_ddim.py:256-258 with scale 1: x [B,C,h,w] float32 / float64, shift [B,C] float32, in x's dtype."""
    return ((x + shift[:, :, None, None]).clamp(-1, 1) + 1) / 2


# The bars.  The library is built with -ffp-contract=on, so a float64 `a * b + c` may be one rounding in the kernel where
# torch has two: x_next and pred_eps are held to float64 ulps of their largest intermediate, not to bit-equality.

def pred_eps_bar(k, n01):
    """(sqrt_recip * n01 - x_start) / sqrt_recipm1: three roundings in the statement, two in a fused kernel, each half an ulp
    of an intermediate no larger than (sqrt_recip * |n01| + 1) / sqrt_recipm1."""
    return 4 * U64 * (k.sqrt_recip_alpha * n01.double().abs() + 1) / k.sqrt_recipm1_alpha


def x_next_bar(k, x_start, pred_eps, n01, eps):
    """x_start * sqrt_alpha_next + c * pred_eps + sigma * eps: float64 ulps of the three terms, and pred_eps' own bar
    scaled by |c|."""
    terms = ((x_start.double() * k.sqrt_alpha_next).abs() + (k.c * pred_eps.double()).abs()
             + (k.sigma * eps.double()).abs())
    return 4 * U64 * terms + abs(k.c) * pred_eps_bar(k, n01)


def ens_bar(k, out, ens):
    """ens0 + out * cof in float32: a fused multiply-add skips the product's rounding."""
    return U32 * ((out.double() * k.cof).abs() + ens.double().abs())


# The edge map: inputs of one state update in which every quarter-resolution pixel is one case of the kernel's branches.

def _exact_minus(v, thr):
    """``v`` (moved to a multiple of 2^-10 where it has to be) and ``u`` with v - u == thr exactly in float32."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    if float(f32(v) - (f32(v) - f32(thr))) != thr:
        v = round(v * 1024) / 1024
    u = f32(v) - f32(thr)
    assert float(f32(v) - u) == thr and float(f32(v)) == v
    return v, float(u)


def edge_inputs(b, nbins, h, w, igev, seed=0):
    """disp, used, unc | None [B,4h,4w], coords0 | None, mask0 [B,h,w] and, per quarter-resolution pixel, the case it holds
    (``labels``: disparity class, renewal pattern, mask0, coords0).  Only the central 2x2 of each 4x4 cell carries the
    case; the twelve outer pixels hold unrelated finite values, out of range included.

    Disparity classes: four equal values 4k and nextafter(4k, 0) for k in {0, 1, nbins-2, nbins-1} (an integer dq and the
    float32 just below it), below 0, above clamp_max, four distinct values, and four distinct values with one clamped at
    either end.  Renewal patterns: 0..4 pixels kept; |disp - used| == dif_thr exactly (not kept, strict <); for ACV
    unc == unc_thr exactly (not kept), for IGEV |disp - used| == 3 exactly (kept by dif < 5, handed on as `used`)."""
    g = torch.Generator().manual_seed(1000 + seed)
    clamp_max = float(nbins - 1 if igev else 4 * nbins - 1)
    dif_thr, unc_thr, ens_thr = (5.0, float("inf"), 3.0) if igev else (1.0, 3.0, 0.0)
    H, W = 4 * h, 4 * w
    rnd = lambda *s: torch.rand(*s, generator=g)
    disp = (rnd(b, H, W) * 1.4 - 0.2) * clamp_max
    used = disp + torch.randn(b, H, W, generator=g) * 2
    unc = rnd(b, H, W) * 5
    mask0 = torch.zeros(b, h, w)
    coords0 = torch.zeros(b, h, w)
    below = lambda k: float(torch.nextafter(torch.tensor(4.0 * k), torch.tensor(0.0)))
    ks = sorted({0, 1, nbins - 2, nbins - 1})
    classes = [(f"int{k}", lambda k=k: [4.0 * k] * 4) for k in ks] + [(f"below{k}", lambda k=k: [below(k)] * 4) for k in ks]
    mix = lambda n: (rnd(n) * clamp_max).tolist()
    classes += [("neg", lambda: [-3.5] * 4), ("over", lambda: [clamp_max + 2.25] * 4), ("mix", lambda: mix(4)),
                ("mix_hi", lambda: mix(3) + [clamp_max + 5.0]), ("mix_lo", lambda: [-1.25] + mix(3))]
    labels = []
    for j in range(b * h * w):
        i = j + 1
        bi, y, x = j // (h * w), (j // w) % h, j % w
        name, make = classes[i % len(classes)]
        c = make()
        r, p0 = i % 7, (i // 7) % 4
        u, q = [0.0] * 4, [0.5] * 4
        for p in range(4):
            kept = ((p - p0) % 4 < r) if r < 5 else p != p0
            if kept:
                u[p] = c[p] + (0.25 if p % 2 else -0.25)
            elif r < 5 and p % 2 and not igev:
                u[p], q[p] = c[p] + 0.25, 4.0                                   # fails the uncertainty test alone
            elif r < 5:
                u[p] = c[p] + dif_thr + 1.5
            elif r == 5:
                c[p], u[p] = _exact_minus(c[p], dif_thr)
            elif igev:
                c[p], u[p] = _exact_minus(c[p], ens_thr)
            else:
                u[p], q[p] = c[p] + 0.25, unc_thr
        for p in range(4):
            yy, xx = 4 * y + 1 + p // 2, 4 * x + 1 + p % 2
            disp[bi, yy, xx], used[bi, yy, xx], unc[bi, yy, xx] = c[p], u[p], q[p]
        mask0[bi, y, x] = (0.0, 0.5, 1.0)[i % 3]
        coords0[bi, y, x] = (0.0, nbins // 2, nbins - 1.0, nbins + 3.0)[i % 4]
        labels.append((name, r, i % 3, i % 4))
    return {"disp": disp, "used": used, "unc": None if igev else unc, "coords0": coords0 if igev else None, "mask0": mask0,
            "labels": labels, "thresholds": (dif_thr, unc_thr, clamp_max, ens_thr)}
