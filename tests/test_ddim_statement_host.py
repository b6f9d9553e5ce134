"""tests/ddim_statement.py, the CPU statement of one DDIM state update that tests/test_gpu_ddim_kernels.py holds the kernels
of csrc/ddim.hip to: tied to the oracle the goldens pin, its bars shown to be able to fail, its edge map shown to hold the
cases it claims.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import ddim_statement as S
from diffuvolume_amd import _lib, ddim
from oracle import acv_oracle as O

G = lambda seed: torch.Generator().manual_seed(seed)
FORMS = {"acv": dict(eta=1.0, dif_thr=1.0, unc_thr=3.0, ens_dif_thr=0.0),
         "igev": dict(eta=1.0, dif_thr=5.0, unc_thr=float("inf"), ens_dif_thr=3.0)}


def coef(form, nbins, pair, cof=0.3, steps=5):
    time, time_next = ddim.time_pairs(1000, steps)[pair]
    clamp_max = float(nbins - 1 if form == "igev" else 4 * nbins - 1)
    return ddim.step_coef(ddim.Tables(torch.cumprod(1 - ddim.cosine_beta_schedule(1000), 0)), time, time_next, cof,
                          clamp_max=clamp_max, **FORMS[form])


def away_from_integers(form, b, nbins, h, w, seed):
    """The kind of inputs of the arena row `_ddim_step`, with a 2x2 average that averages: the position the two-hot encodes
    stays 1e-3 away from every integer, so that floor() comes out the same whichever way the average is rounded."""
    g = G(seed)
    top = (nbins - 1) / 4 if form == "igev" else nbins - 1
    dq = torch.rand(b, h, w, generator=g) * top
    dq = dq.floor() + (dq - dq.floor()).clamp(2e-3, 1 - 2e-3)
    dq[0, 0, 0], dq[0, 0, 1] = 0.25, top + 0.5
    disp = F.interpolate(dq[:, None] * 4, size=(4 * h, 4 * w), mode="nearest")[:, 0].contiguous()
    disp = disp + (torch.rand(b, 4 * h, 4 * w, generator=g) - 0.5) * 4e-3
    used = disp + torch.randn(b, 4 * h, 4 * w, generator=g) * (4.0 if form == "igev" else 1.2)
    unc = None if form == "igev" else torch.rand(b, 4 * h, 4 * w, generator=g) * 5
    coords0 = None
    if form == "igev":          # integer x coordinates; the last columns push the position up to and past nbins - 1
        coords0 = (torch.arange(w) * (nbins + 2) // w).float().expand(b, h, w).contiguous()
    mask0 = (torch.rand(b, h, w, generator=g) > 0.6).float() * 0.5
    return disp, unc, used, coords0, mask0


@pytest.mark.parametrize("form", ["acv", "igev"])
def test_statement_against_the_oracle(form):
    """x_start within 4e-6 of the oracle's expression (acv_oracle.ACVOracle.model_predictions, igev_oracle.IGEVLoopOracle.
    model_predictions) at the arena row's size: the oracle's position comes from ATen's CPU interpolate, which sums the 2x2
    in another order and lands up to one float32 ulp from the statement's, and the two-hot weight 2 * frac - 1 doubles that.
    Below 12 an ulp is 9.5e-7: 1.9e-6 measured here.  (At 48 bins, positions above 32, the same single ulp is 3.8e-6 and
    x_start differs by 7.6e-6.)  mask, the output rule and pred_eps given x_start: equal."""
    b, nbins, h, w = 2, 12, 4, 6
    k = coef(form, nbins, 4, cof=1.0)                            # the last step: neither eps nor fill
    disp, unc, used, coords0, mask0 = away_from_integers(form, b, nbins, h, w, 31)
    n01 = torch.rand(b, nbins, h, w, generator=G(32))
    x_start, pred_eps, mask, _, ens = S.ddim_step_statement(disp, unc, used, coords0, n01, None, None, mask0,
                                                            torch.zeros_like(disp), k, nbins)
    dn = F.interpolate(torch.clamp(disp[:, None], 0, k.clamp_max), size=(h, w), mode="bilinear") / 4
    if form == "igev":
        dn = torch.clamp(coords0[:, None] + dn, 0, nbins - 1)
    inner = dn < nbins - 1
    assert float((dn - dn.round()).abs()[inner].min()) > 5e-4 and bool((~inner).any()) and bool(inner.any())
    ref = torch.clamp(O.encode_two_hot(dn, nbins) * 2 - 1.0, -1, 1)
    assert x_start.dtype == torch.float32 and pred_eps.dtype == torch.float64
    err = float((x_start - ref).abs().max())
    print(f"    x_start: max abs err {err:.2e} (bar 4e-6)")
    assert err <= 4e-6
    dif = torch.abs(disp - used)
    keep = (dif < k.dif_thr) if form == "igev" else ((dif < k.dif_thr) & (unc < k.unc_thr))
    ref_mask = torch.clamp(mask0 + F.interpolate(keep.float()[:, None], size=(h, w), mode="bilinear")[:, 0], 0, 1)
    assert torch.equal(mask, ref_mask) and 0 < float(mask.mean()) < 1
    out = torch.where(dif < 3, disp, used) if form == "igev" else disp
    assert torch.equal(ens, out) and torch.equal(S.output_rule(disp, used, k), out)
    bs = (b, 1, 1, 1)
    t = torch.full((b,), ddim.time_pairs(1000, 5)[4][0], dtype=torch.long)
    sr, srm1 = torch.sqrt(1 / O.cosine_alphas_cumprod(1000)), torch.sqrt(1 / O.cosine_alphas_cumprod(1000) - 1)
    assert torch.equal(pred_eps, (sr.gather(-1, t).reshape(bs) * n01 - x_start) / srm1.gather(-1, t).reshape(bs))


def test_two_hot_is_the_oracles():
    """The statement's two-hot, which also runs on the device and in float64, has the oracle's float32 bits: integers, their
    float32 neighbours and the forced last bin."""
    for nbins in (2, 12, 48):
        ints = torch.arange(nbins, dtype=torch.float32)
        dq = torch.cat([ints, torch.nextafter(ints, ints + 1), torch.nextafter(ints[1:], ints[1:] - 1),
                        torch.tensor([nbins - 0.5]), torch.rand(40, generator=G(nbins)) * nbins]).view(1, 1, 1, -1)
        assert torch.equal(S.two_hot(dq, nbins), O.encode_two_hot(dq, nbins))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_the_x_next_bar_can_fail(dtype):
    """With the real coefficients of a 5-step loop, the same update without the reference's float32 rounding points
    (x_start * sqrt_alpha_next, sigma * eps_f32) misses the bar x_next is held to by a factor of 1000
    and more: the bar tells a kept rounding point from a lost one."""
    b, nbins, h, w = 2, 48, 6, 9
    worst = 0.0
    for pair in (0, 2):
        k = coef("acv", nbins, pair)
        disp, unc, used, coords0, mask0 = away_from_integers("acv", b, nbins, h, w, 33 + pair)
        g = G(35)
        n01 = torch.rand(b, nbins, h, w, generator=g, dtype=dtype)
        eps = torch.randn(b, nbins, h, w, generator=g, dtype=dtype)
        fill = torch.rand(b, nbins, h, w, generator=g, dtype=torch.float64)
        mask0 = mask0 + 0.5                                     # no pixel takes `fill`
        xs, pn, _, xn, _ = S.ddim_step_statement(disp, unc, used, coords0, n01, eps, fill, mask0, None, k, nbins)
        xs64, _, _, xn64, _ = S.ddim_step_statement(disp, unc, used, coords0, n01, eps, fill, mask0, None, k, nbins,
                                                 all_float64=True)
        assert xn.dtype == xn64.dtype == torch.float64 and torch.equal(xs64, xs.double())
        ratio = float(((xn - xn64).abs() / S.x_next_bar(k, xs, pn, n01, eps)).max())
        print(f"    pair {pair}, {dtype}: all-float64 differs by {float((xn - xn64).abs().max()):.1e}, {ratio:.0f} bars")
        assert ratio >= 1000
        worst = max(worst, ratio)
    assert worst >= 1000


@pytest.mark.parametrize("igev", [False, True])
@pytest.mark.parametrize("shape", [(2, 12, 5, 7), (2, 48, 9, 15)])
def test_edge_map_holds_its_cases(shape, igev):
    b, nbins, h, w = shape
    e = S.edge_inputs(b, nbins, h, w, igev)
    names = {l[0] for l in e["labels"]}
    assert {"neg", "over", "mix", "mix_hi", "mix_lo"} <= names
    assert {f"{p}{k}" for p in ("int", "below") for k in (0, 1, nbins - 2, nbins - 1)} <= names
    assert {l[1] for l in e["labels"]} == set(range(7)) and {l[2] for l in e["labels"]} == {0, 1, 2}
    assert {l[3] for l in e["labels"]} == {0, 1, 2, 3}
    dif_thr, unc_thr, clamp_max, ens_thr = e["thresholds"]
    k = coef("igev" if igev else "acv", nbins, 4)
    assert (k.dif_thr, k.unc_thr, k.clamp_max, k.ens_dif_thr) == (dif_thr, unc_thr, clamp_max, ens_thr)
    disp, used, unc = e["disp"], e["used"], e["unc"]
    centre = torch.zeros(b, 4 * h, 4 * w, dtype=torch.bool)
    for dy in (1, 2):
        for dx in (1, 2):
            centre[:, dy::4, dx::4] = True
    dif = (disp - used).abs()
    assert bool(((dif == dif_thr) & centre).any())                                      # exactly on the threshold
    assert bool(((dif == ens_thr) & centre).any() if igev else ((unc == unc_thr) & centre).any())
    assert bool(((disp < 0) & centre).any()) and bool(((disp > clamp_max) & centre).any())
    assert bool(torch.isfinite(disp).all()) and bool(((disp < 0) & ~centre).any()) and bool(((disp > clamp_max) & ~centre).any())
    dq = S.quarter_position(disp, e["coords0"], clamp_max, nbins)
    real = dq.floor()
    assert bool((dq == real).any()) and bool((real == nbins - 1).any()) and bool((dq == 0).any())
    assert bool((real - torch.nextafter(dq, dq + 1).floor() != 0).any())                # the float32 just below an integer
    if igev:
        assert bool((dq == nbins - 1).any()) and bool(((e["coords0"] > 0) & (dq < nbins - 1)).any())
    n01 = torch.rand(b, nbins, h, w, generator=G(5))
    _, _, mask, _, _ = S.ddim_step_statement(disp, unc, used, e["coords0"], n01, None, None, e["mask0"], None, k, nbins)
    kept4 = (mask - e["mask0"]) * 4
    assert set(mask.unique().tolist()) == {0.0, 0.25, 0.5, 0.75, 1.0}
    # every renewal pattern keeps what it says; on a threshold exactly is not kept (IGEV's dif == 3 is: 3 < 5)
    for (name, r, m, c), got, m0 in zip(e["labels"], kept4.reshape(-1).tolist(), e["mask0"].reshape(-1).tolist()):
        want = r if r < 5 else (4 if (igev and r == 6) else 3)
        assert got == min(want, 4 * (1 - m0)), (name, r, m, got)
