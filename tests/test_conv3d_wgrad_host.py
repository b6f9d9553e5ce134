"""Host-side checks of the training additions (no GPU): the weight-gradient entry points are exported and bound, bad
arguments are refused before anything touches the device, csrc/conv3d_wgrad.hip compiles for gfx950 onto the exact-fp32
matrix instruction without spills or scratch, and diffuvolume_amd.loss restates SceneFlow/models/loss.py."""
import re
import subprocess

import pytest
import torch

from diffuvolume_amd import _build


@pytest.fixture(scope="module")
def lib():
    _build.build()
    from diffuvolume_amd import _lib
    return _lib.load()


def test_wgrad_entry_points_are_bound(lib):
    from diffuvolume_amd import _lib
    for name in ("dv_conv3d_wgrad_workspace_floats", "dv_conv3d_wgrad_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_wgrad_argument_validation_without_gpu(lib):
    ws = lib.dv_conv3d_wgrad_workspace_floats
    assert ws(1, 32, 8, 8, 8, 32, 5, 1) == 0
    assert ws(1, 32, 8, 8, 8, 32, 3, 3) == 0
    assert ws(1, 32, 8, 8, 8, 32, 1, 2) == 0
    assert ws(0, 32, 8, 8, 8, 32, 3, 1) == 0
    n = ws(2, 128, 12, 16, 32, 128, 3, 1)
    assert n > 0 and n % (128 * 128 * 27) == 0 and n * 4 <= 48 << 20          # whole splits, bounded workspace
    assert ws(1, 32, 2, 4, 16, 32, 3, 1) == 32 * 32 * 27                      # one 2 x 4 x 16 brick: one split
    fake = 256                                                                # never dereferenced: rejected first
    assert lib.dv_conv3d_wgrad_f32(fake, fake, fake, fake, 1, 32, 8, 8, 8, 32, 5, 1, None) == -3
    assert lib.dv_conv3d_wgrad_f32(fake, fake, fake, fake, 1, 32, 8, 8, 8, 32, 3, 3, None) == -3
    assert lib.dv_conv3d_wgrad_f32(fake, fake, fake, None, 1, 32, 8, 8, 8, 32, 3, 1, None) == -1
    assert lib.dv_conv3d_wgrad_f32(None, fake, fake, fake, 1, 32, 8, 8, 8, 32, 3, 1, None) == -1
    assert lib.dv_conv3d_wgrad_f32(fake, fake, fake, fake, 1, 0, 8, 8, 8, 32, 3, 1, None) == -2


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv3d_wgrad.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / "conv3d_wgrad.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return out.read_text()


def test_wgrad_kernels_on_fp32_mfma_without_spills(isa):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*s_endpgm", isa, re.M | re.S)}
    main = {n: b for n, b in bodies.items() if "conv3d_wgrad_kernel" in n}
    assert len(main) == 3, sorted(main)                       # k3 s1, k3 s2, k1
    for name, body in main.items():
        assert "v_mfma_f32_16x16x4_f32" in body, name
    assert ";;#ASMSTART" not in isa                           # no inline asm: the hazard lint has nothing to check
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert spills and all(v == 0 for v in spills)
    assert private and all(v == 0 for v in private)


def _smooth_l1(a, b):
    d = (a - b).abs()
    return torch.where(d < 1, 0.5 * d * d, d - 0.5).mean()


def test_losses_match_the_reference_formulas():
    from diffuvolume_amd import loss as L
    import diffuvolume_amd as dv
    g = torch.Generator().manual_seed(5)
    gt = torch.rand(2, 8, 12, generator=g, dtype=torch.float64) * 240 - 20
    mask = (gt < 192) & (gt > 0)
    ests = [gt + torch.randn(2, 8, 12, generator=g, dtype=torch.float64) * s for s in (0.3, 1.0, 2.0, 5.0)]
    terms = [_smooth_l1(e[mask], gt[mask]) for e in ests]
    torch.testing.assert_close(L.model_loss_train(ests, gt, mask),
                               0.5 * terms[0] + 0.5 * terms[1] + 0.7 * terms[2] + 1.0 * terms[3], rtol=1e-14, atol=0)
    torch.testing.assert_close(L.model_loss_train_freeze_attn(ests, gt, mask),
                               0.5 * terms[0] + 0.7 * terms[1] + 1.0 * terms[2], rtol=1e-14, atol=0)
    torch.testing.assert_close(L.model_loss_train_attn_only(ests, gt, mask), terms[0], rtol=1e-14, atol=0)
    torch.testing.assert_close(L.model_loss_test(ests, gt, mask), (ests[0][mask] - gt[mask]).abs().mean(),
                               rtol=1e-14, atol=0)
    assert dv.model_loss_train is L.model_loss_train


def test_train_route_switch_is_registered(monkeypatch):
    from diffuvolume_amd import _env, train3d
    assert "DV_TRAIN_CONV3D" in _env.KNOBS
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    assert train3d.route() == "hip"
    monkeypatch.setenv("DV_TRAIN_CONV3D", "torch")
    assert train3d.route() == "torch"
    monkeypatch.setenv("DV_TRAIN_CONV3D", "miopen")
    with pytest.raises(ValueError):
        train3d.route()


def test_hip_route_refuses_cpu_tensors(monkeypatch):
    from diffuvolume_amd import DiffuVolumeError, train3d
    monkeypatch.delenv("DV_TRAIN_CONV3D", raising=False)
    x = torch.zeros(1, 8, 4, 4, 4, requires_grad=True)
    with pytest.raises(DiffuVolumeError):
        train3d.conv3d(x, torch.zeros(8, 8, 3, 3, 3))
    with pytest.raises(DiffuVolumeError):
        train3d.conv_transpose3d(x, torch.zeros(8, 4, 3, 3, 3))
