"""The shared DDIM host code (diffuvolume_amd/ddim.py): time list, coefficient struct, schedule buffers, and the checks
that come before anything touches the library or the device.  No GPU."""
import ctypes
import types

import pytest
import torch

from conftest import load_golden
from diffuvolume_amd import _lib, ddim, synth

STEP_COUNTS = (2, 3, 5, 20)
# (eta, dif_thr, unc_thr, clamp_max, ens_dif_thr): ACVNet_DDIM, PWCNet_ddim (maxdisp 192), IGEVDiffusionLoop
THRESHOLDS = {"acv": (1.0, 1.0, 3.0, 191.0, 0.0), "pcw": (1.0, 1.0, 1.0, 191.0, 0.0),
              "igev": (1.0, 5.0, float("inf"), 47.0, 3.0)}


@pytest.fixture(scope="module")
def schedule():
    return load_golden("encoder_schedule")


def test_time_pairs(schedule):
    for s in STEP_COUNTS:
        pairs = ddim.time_pairs(1000, s)
        assert len(pairs) == s and pairs[-1][1] == -1
        assert [p[0] for p in pairs] + [pairs[-1][1]] == schedule[f"times_{s}"].tolist()
    assert ddim.time_pairs(1000, 20)[0] == (999, 949)
    assert ddim.time_pairs(1000, 5) == [(999, 799), (799, 599), (599, 399), (399, 199), (199, -1)]
    assert ddim.time_pairs(1000, 3) == [(999, 665), (665, 332), (332, -1)]


def _f32(x):
    return ctypes.c_float(x).value


@pytest.mark.parametrize("flavour", sorted(THRESHOLDS))
def test_step_coef_fields(schedule, flavour):
    """Every field against the reference's own float64 statements (SceneFlow acv_ddim.py:156-157, :348-352) on the
    reference's ``alphas_cumprod``; the struct's float fields hold the float32 of what was passed."""
    ac = schedule["alphas_cumprod"]
    assert ac.dtype == torch.float64
    tables = ddim.Tables(ac)
    eta, dif_thr, unc_thr, clamp_max, ens_dif_thr = THRESHOLDS[flavour]
    for s in STEP_COUNTS:
        for i, (time, time_next) in enumerate(ddim.time_pairs(1000, s)):
            cof = 0.1 * (i + 1)
            k = ddim.step_coef(tables, time, time_next, cof, eta=eta, dif_thr=dif_thr, unc_thr=unc_thr,
                               clamp_max=clamp_max, ens_dif_thr=ens_dif_thr)
            assert k.sqrt_recip_alpha == float(torch.sqrt(1. / ac)[time])
            assert k.sqrt_recipm1_alpha == float(torch.sqrt(1. / ac - 1)[time])
            assert (k.dif_thr, k.unc_thr, k.cof) == (_f32(dif_thr), _f32(unc_thr), _f32(cof))
            assert (k.clamp_max, k.ens_dif_thr) == (_f32(clamp_max), _f32(ens_dif_thr))
            assert k.last == int(time_next < 0) and (k.last == 1) == (i == s - 1)
            if time_next < 0:
                assert (k.sigma, k.c, k.sqrt_alpha_next) == (0.0, 0.0, 0.0)
                continue
            alpha = ac[time]
            alpha_next = ac[time_next]
            sigma = eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            assert (k.sigma, k.c, k.sqrt_alpha_next) == (float(sigma), float(c), float(alpha_next.sqrt()))


def _igev_args():
    return types.SimpleNamespace(**synth.IGEV_TRAIN_ARGS)


def _igev_feature():
    from diffuvolume_amd.igev_stereo_ddim import Feature
    return Feature(synth.StubMobileNetV2())


def test_schedule_buffers(schedule):
    from diffuvolume_amd import ACVNet, ACVNet_DDIM, PWCNet, PWCNet_ddim
    from diffuvolume_amd.igev_stereo import IGEVStereo
    from diffuvolume_amd.igev_stereo_ddim import IGEVStereo_ddim
    assert len(ddim.SCHEDULE_BUFFERS) == 12
    assert ddim.SCHEDULE_BUFFERS[0] == "betas" and ddim.SCHEDULE_BUFFERS[-1] == "posterior_mean_coef2"
    for m in (ACVNet_DDIM(192), PWCNet_ddim(192, True), IGEVStereo_ddim(_igev_args(), feature=_igev_feature())):
        sd = m.state_dict()
        assert tuple(k for k in sd if "." not in k and k in ddim.SCHEDULE_BUFFERS) == ddim.SCHEDULE_BUFFERS
        for name in ddim.SCHEDULE_BUFFERS:
            assert sd[name].dtype == torch.float64 and sd[name].shape == (1000,), name
        torch.testing.assert_close(sd["alphas_cumprod"], schedule["alphas_cumprod"], rtol=1e-13, atol=0)
    for m in (ACVNet(192), PWCNet(192), IGEVStereo(_igev_args(), feature=_igev_feature())):
        assert not set(ddim.SCHEDULE_BUFFERS) & set(m.state_dict())


@pytest.mark.parametrize("dtype", [torch.float16, torch.int64])
def test_noise_prepare_refuses_other_dtypes(monkeypatch, dtype):
    """The float32 / float64 check of every flavour's ``_filter`` comes before the time MLP, the library and the device."""
    def untouched(*a, **k):
        raise AssertionError("the dtype check must come first")
    monkeypatch.setattr(_lib, "load", untouched)
    head = types.SimpleNamespace(shift=untouched)
    x = torch.zeros((1, 48, 2, 3), dtype=dtype)
    with pytest.raises(TypeError, match="float32 .* or float64"):
        ddim.noise_prepare(head, x, torch.zeros(1, dtype=torch.long))
    with pytest.raises(TypeError, match="float32 .* or float64"):
        ddim.noise_prepare(head, x, None, shift=torch.zeros(1, 48))


def test_check_loop_args_messages():
    b, h, w = 2, 3, 5
    volume = torch.zeros(b, 4, 48, h, w)
    used = torch.zeros(b, 4 * h, 4 * w)
    x_T = torch.zeros(b, 48, h, w)
    assert ddim.check_loop_args(volume, used.unsqueeze(1), x_T, 192).shape == (b, 4 * h, 4 * w)
    with pytest.raises(RuntimeError) as e:
        ddim.check_loop_args(volume, used[:, :-4], x_T, 192)
    assert str(e.value) == ("The size of tensor a (2, 12, 20) must match the size of tensor b (2, 8, 20): "
                            "`used` must be the full-resolution disparity of the volume")
    with pytest.raises(RuntimeError) as e:
        ddim.check_loop_args(volume, used, x_T[:, :24], 192)
    assert str(e.value) == "x_T must be (2, 48, 3, 5), got (2, 24, 3, 5)"
    with pytest.raises(RuntimeError) as e:
        ddim.check_loop_args(volume[:, :, :24], used, x_T, 192)
    assert str(e.value) == "the volume must have 48 disparity bins, got 24"
    with pytest.raises(RuntimeError) as e:
        ddim.check_loop_args(volume[:, :, :24], used, x_T, 192, what="fused volume")
    assert str(e.value) == "the fused volume must have 48 disparity bins, got 24"
