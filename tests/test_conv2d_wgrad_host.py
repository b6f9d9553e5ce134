"""Host-side checks of the PWCNet_ddim training additions (no GPU): the 2-D weight-gradient entry points are exported
and bound, bad arguments are refused before anything touches the device, csrc/conv2d_wgrad.hip compiles for gfx950 onto
the exact-fp32 matrix instruction without spills or scratch, model_loss_kitti12 restates KITTI12/models/loss.py, and the
training route refuses CPU tensors and unknown switch values."""
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


def test_wgrad2d_entry_points_are_bound(lib):
    from diffuvolume_amd import _lib
    for name in ("dv_conv2d_wgrad_workspace_floats", "dv_conv2d_wgrad_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_wgrad2d_argument_validation_without_gpu(lib):
    ws = lib.dv_conv2d_wgrad_workspace_floats
    assert ws(1, 32, 16, 32, 32, 5, 1) == 0                                    # k = 5
    assert ws(1, 32, 16, 32, 32, 3, 0) == 0                                    # dilation 0
    assert ws(1, 32, 16, 32, 32, 3, 17) == 0                                   # dilation 17
    assert ws(1, 0, 16, 32, 32, 3, 1) == 0                                     # Cin 0
    assert ws(0, 32, 16, 32, 32, 3, 1) == 0
    n = ws(4, 128, 256, 512, 128, 3, 1)
    assert n > 0 and n % (128 * 128 * 9) == 0 and n * 4 <= 48 << 20           # whole splits, bounded workspace
    n = ws(4, 146, 256, 512, 128, 3, 1)
    assert n > 0 and n % (146 * 128 * 9) == 0 and n * 4 <= 48 << 20
    assert ws(1, 32, 4, 32, 32, 3, 1) == 32 * 32 * 9                          # one 4 x 32 brick: one split
    assert ws(1, 32, 2, 32, 32, 3, 16) == 32 * 32 * 9                         # one 2 x 32 brick (large dilations)
    assert ws(1, 32, 4, 32, 1, 1, 1) == 32                                    # 1x1
    fake = 256                                                                # never dereferenced: rejected first
    assert lib.dv_conv2d_wgrad_f32(fake, fake, fake, fake, 1, 32, 16, 32, 32, 5, 1, None) == -3
    assert lib.dv_conv2d_wgrad_f32(fake, fake, fake, fake, 1, 32, 16, 32, 32, 3, 0, None) == -3
    assert lib.dv_conv2d_wgrad_f32(fake, fake, fake, fake, 1, 32, 16, 32, 32, 3, 17, None) == -3
    assert lib.dv_conv2d_wgrad_f32(fake, fake, fake, None, 1, 32, 16, 32, 32, 3, 1, None) == -1
    assert lib.dv_conv2d_wgrad_f32(None, fake, fake, fake, 1, 32, 16, 32, 32, 3, 1, None) == -1
    assert lib.dv_conv2d_wgrad_f32(fake, fake, fake, fake, 1, 0, 16, 32, 32, 3, 1, None) == -2


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv2d_wgrad.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / "conv2d_wgrad.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return out.read_text()


def test_wgrad2d_kernels_on_fp32_mfma_without_spills(isa):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*s_endpgm", isa, re.M | re.S)}
    main = {n: b for n, b in bodies.items() if "conv2d_wgrad_kernel" in n}
    assert len(main) == 3, sorted(main)                       # k3 d<=4, k3 d<=16, k1
    for name, body in main.items():
        assert "v_mfma_f32_16x16x4_f32" in body, name
    assert ";;#ASMSTART" not in isa
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert spills and all(v == 0 for v in spills)
    assert private and all(v == 0 for v in private)


def test_kitti12_loss_matches_the_reference_formula():
    import diffuvolume_amd as dv
    from diffuvolume_amd import loss as L
    g = torch.Generator().manual_seed(7)
    gt = torch.rand(2, 8, 12, generator=g, dtype=torch.float64) * 240 - 20
    mask = (gt < 192) & (gt > 0)
    ests = [gt + torch.randn(2, 8, 12, generator=g, dtype=torch.float64) * s for s in (0.3, 0.6, 1.0, 2.0, 3.0, 5.0)]

    def smooth_l1(a, b):
        d = (a - b).abs()
        return torch.where(d < 1, 0.5 * d * d, d - 0.5).mean()

    want = sum(w * smooth_l1(e[mask], gt[mask]) for e, w in zip(ests, [0.5, 0.5, 0.5, 0.7, 1.0, 1.3]))
    torch.testing.assert_close(L.model_loss_kitti12(ests, gt, mask), want, rtol=1e-14, atol=0)
    assert dv.model_loss_kitti12 is L.model_loss_kitti12
    assert dv.model_loss_train is L.model_loss_train                         # the SceneFlow names are unchanged


def test_train2d_route_switch_is_registered(monkeypatch):
    from diffuvolume_amd import _env, train2d
    assert "DV_TRAIN_CONV2D" in _env.KNOBS
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    assert train2d.route() == "hip"
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    assert train2d.route() == "torch"
    monkeypatch.setenv("DV_TRAIN_CONV2D", "bogus")
    with pytest.raises(ValueError):
        train2d.route()
    with pytest.raises(ValueError):
        train2d.conv2d(torch.zeros(1, 4, 8, 8), torch.zeros(4, 4, 3, 3))


def test_train2d_refuses_cpu_tensors(monkeypatch):
    from diffuvolume_amd import DiffuVolumeError, train2d
    monkeypatch.delenv("DV_TRAIN_CONV2D", raising=False)
    x = torch.zeros(1, 8, 8, 8, requires_grad=True)
    with pytest.raises(DiffuVolumeError):
        train2d.conv2d(x, torch.zeros(8, 8, 3, 3), dilation=2)


def test_train_forward_refuses_cpu_tensors():
    from diffuvolume_amd import PWCNet_ddim
    model = PWCNet_ddim(192).train()
    left = torch.zeros(1, 3, 64, 128)
    with pytest.raises(NotImplementedError, match="MI355X only"):
        model(left, left, None, torch.zeros(1, 1, 16, 32), None)
