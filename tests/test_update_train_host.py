"""Host side of the update block's training route, without a GPU: the new entry points are bound and refuse bad arguments
before anything touches the device, csrc/conv2d_wgrad_cat.hip compiles for gfx950 onto the exact-fp32 MFMA without
scratch, train-mode calls on CPU tensors raise, and the committed fixture is inside its own gate."""
import ctypes
import re
import subprocess
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _build, _lib
from diffuvolume_amd.synth import UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_entry_points_are_bound(lib):
    for name in ("dv_conv2d_wgrad_cat_workspace_floats", "dv_conv2d_wgrad_cat_f32", "dv_conv2d_1in_wgrad_f32", "dv_gru_reset_mul_f32", "dv_gru_blend_f32",
                 "dv_gru_gates_bwd_blend_f32", "dv_gru_gates_bwd_reset_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)


def test_workspace_query(lib):
    ws = lib.dv_conv2d_wgrad_cat_workspace_floats
    assert ws(ints(128, 128, 128), 3, 2, 20, 28, 128, 3) % (128 * 384 * 9) == 0
    assert ws(ints(128, 128, 128), 3, 2, 20, 28, 128, 3) > 0
    assert ws(ints(162), 1, 2, 20, 28, 64, 1) > 0
    assert ws(ints(5, 3), 2, 1, 1, 1, 1, 3) == 1 * 8 * 9                          # one split at least
    assert ws(ints(128), 1, 2, 20, 28, 128, 5) == 0                                # k outside {1, 3}
    assert ws(ints(128), 1, 2, 20, 28, 128, 2) == 0
    assert ws(ints(128), 0, 2, 20, 28, 128, 3) == 0                                # n_inputs outside 1..4
    assert ws(ints(1, 1, 1, 1, 1), 5, 2, 20, 28, 128, 3) == 0
    assert ws(ints(128, 0), 2, 2, 20, 28, 128, 3) == 0                             # an empty source
    assert ws(None, 1, 2, 20, 28, 128, 3) == 0
    assert ws(ints(128), 1, 0, 20, 28, 128, 3) == 0 and ws(ints(128), 1, 2, 20, 28, 0, 3) == 0
    # the bench shapes (batch 4 at 80x184 / 40x92 / 20x46, refinenet3's 128 -> 128 at 256x512) stay within 48 MB
    for chans, cout, k, h, w in (((128, 128, 128), 128, 3, 80, 184), ((128, 128, 128), 128, 3, 40, 92),
                                 ((128, 128), 128, 3, 20, 46), ((162,), 64, 1, 80, 184), ((128,), 256, 3, 80, 184),
                                 ((64, 64), 127, 3, 80, 184), ((128,), 128, 3, 256, 512), ((128,), 128, 1, 256, 512)):
        n = ws(ints(*chans), len(chans), 4, h, w, cout, k)
        assert 0 < n * 4 <= 48 << 20, (chans, cout, k, h, w)


def test_argument_validation_without_gpu(lib):
    fake = ctypes.c_void_p(4096)
    ptrs = (ctypes.c_void_p * 4)(4096, 4096, 4096, 4096)
    f = lib.dv_conv2d_wgrad_cat_f32
    assert f(ptrs, ints(8, 8), 2, fake, fake, fake, 1, 8, 8, 16, 5, None) == -3      # k
    assert f(ptrs, ints(8, 8), 2, fake, fake, fake, 1, 8, 8, 16, 2, None) == -3
    assert f(None, ints(8, 8), 2, fake, fake, fake, 1, 8, 8, 16, 3, None) == -1
    assert f(ptrs, None, 2, fake, fake, fake, 1, 8, 8, 16, 3, None) == -1
    assert f(ptrs, ints(8, 8), 2, None, fake, fake, 1, 8, 8, 16, 3, None) == -1
    assert f(ptrs, ints(8, 8), 2, fake, None, fake, 1, 8, 8, 16, 3, None) == -1
    assert f(ptrs, ints(8, 8), 2, fake, fake, None, 1, 8, 8, 16, 3, None) == -1
    assert f((ctypes.c_void_p * 2)(4096, None), ints(8, 8), 2, fake, fake, fake, 1, 8, 8, 16, 3, None) == -1
    assert f(ptrs, ints(8, 8), 0, fake, fake, fake, 1, 8, 8, 16, 3, None) == -2      # n_inputs
    assert f(ptrs, ints(8, 8, 8, 8, 8), 5, fake, fake, fake, 1, 8, 8, 16, 3, None) == -2
    assert f(ptrs, ints(8, 0), 2, fake, fake, fake, 1, 8, 8, 16, 3, None) == -2      # channel sum with an empty source
    assert f(ptrs, ints(8, 8), 2, fake, fake, fake, 0, 8, 8, 16, 3, None) == -2
    w1 = lib.dv_conv2d_1in_wgrad_f32
    assert w1(fake, fake, fake, 1, 8, 8, 64, 5, None) == -3 and w1(fake, fake, fake, 1, 8, 8, 64, 3, None) == -3 and w1(fake, fake, None, 1, 8, 8, 64, 7, None) == -1
    assert w1(None, fake, fake, 1, 8, 8, 64, 7, None) == -1 and w1(fake, fake, fake, 1, 0, 8, 64, 7, None) == -2
    assert lib.dv_gru_reset_mul_f32(None, fake, fake, 16, None) == -1 and lib.dv_gru_reset_mul_f32(fake, fake, None, 16, None) == -1
    assert lib.dv_gru_reset_mul_f32(fake, fake, fake, 0, None) == -2
    assert lib.dv_gru_blend_f32(None, fake, fake, fake, 16, None) == -1 and lib.dv_gru_blend_f32(fake, None, fake, fake, 16, None) == -1
    assert lib.dv_gru_blend_f32(fake, fake, fake, fake, 0, None) == -2
    assert lib.dv_gru_gates_bwd_blend_f32(fake, fake, fake, fake, fake, fake, None, 16, None) == -1
    assert lib.dv_gru_gates_bwd_reset_f32(fake, fake, fake, None, fake, 16, None) == -1
    assert lib.dv_gru_gates_bwd_reset_f32(fake, fake, fake, fake, fake, 0, None) == -2


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv2d_wgrad_cat.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / "conv2d_wgrad_cat.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return out.read_text()


def test_kernels_on_fp32_mfma_without_scratch(isa):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*s_endpgm", isa, re.M | re.S)}
    main = {n: b for n, b in bodies.items() if "conv2d_wgrad_cat_kernel" in n}
    assert len(main) == 2, sorted(main)                                # k = 1 and k = 3
    for name, body in main.items():
        assert "v_mfma_f32_16x16x4_f32" in body, name
        assert "atomic" not in body, name
    assert ";;#ASMSTART" not in isa
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert spills and all(v == 0 for v in spills)
    assert private and all(v == 0 for v in private)


def block():
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    return BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)


def test_train_mode_on_cpu_tensors_raises():
    from diffuvolume_amd.synth import update_train_inputs
    m = block().train()
    x = update_train_inputs(1, 1, 8, 8, 1)
    with pytest.raises(DiffuVolumeError):
        m(list(x["net"]), x["inp"], x["corr"][0], x["disp"])
    with pytest.raises(DiffuVolumeError):
        m.gru16(x["net"][2], *x["inp"][2], x["net"][2])


def test_route_switch_is_the_existing_one(monkeypatch):
    from diffuvolume_amd import train2d
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    assert train2d.route() == "torch"
    monkeypatch.setenv("DV_TRAIN_CONV2D", "cudnn")
    with pytest.raises(ValueError):
        train2d.route()


def test_torch_route_of_a_conv_gru_is_the_reference_expression(monkeypatch):
    """DV_TRAIN_CONV2D=torch needs no device: ConvGRU's training call is then update.py:33-40 in torch ops."""
    from diffuvolume_amd import train2d
    monkeypatch.setenv("DV_TRAIN_CONV2D", "torch")
    gru = block().gru16.double()
    g = torch.Generator().manual_seed(3)
    h, cz, cr, cq, x = (torch.randn(1, 128, 5, 7, generator=g, dtype=torch.float64) for _ in range(5))
    out = train2d.conv_gru(None, gru, torch.tanh(h), cz, cr, cq, x)
    hx = torch.cat([torch.tanh(h), x], dim=1)
    z, r = torch.sigmoid(gru.convz(hx) + cz), torch.sigmoid(gru.convr(hx) + cr)
    q = torch.tanh(gru.convq(torch.cat([r * torch.tanh(h), x], dim=1)) + cq)
    assert torch.equal(out, (1 - z) * torch.tanh(h) + z * q)


def test_fixture_is_inside_its_gate():
    with np.load(GOLDEN / "update_train_loop.npz") as z:
        gold = {k: z[k] for k in z.files}
    assert float(gold["gate"]) == 1e-4 and sorted(str(c) for c in gold["cases"]) == ["even", "ragged"]
    assert tuple(gold["even_shape"]) == (2, 16, 32, 6) and tuple(gold["ragged_shape"]) == (2, 20, 28, 4)
    names = {n for n, _ in block().named_parameters()}
    for case in ("even", "ragged"):
        assert set(str(n) for n in gold[f"{case}_grad_names"]) == names          # every parameter has a gradient
        assert len(gold[f"{case}_leaf_names"]) == 12
        assert np.all(gold[f"{case}_ref_err"] <= 1e-4) and np.all(gold[f"{case}_ref_err"] > 0)
        for what in ("grad", "leaf"):                  # (ref_err above is over the full tensors; the norms agree likewise)
            a, b = gold[f"{case}_{what}_norm_f32"].astype(np.float64), gold[f"{case}_{what}_norm_f64"]
            assert np.all(b > 0) and np.all(np.abs(a - b) <= 1e-4 * b)
            assert gold[f"{case}_{what}_val_f32"].shape == gold[f"{case}_{what}_val_f64"].shape == (len(a), 32)
