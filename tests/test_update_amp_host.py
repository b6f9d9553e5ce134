"""Host-side checks of mixed-precision training of IGEV's update block (no GPU): the three new entries are declared in
the header, bound and exported, bad arguments are refused before anything touches the device, and the public switches
(``set_train_precision``, ``forward_train(amp=...)``) exist with float32 as the default."""
import inspect
import types

import pytest

from diffuvolume_amd import _build

NEW = ("dv_conv2d_wgrad_cat_f16", "dv_gru_reset_mul_f16", "dv_gru_blend_f16")


@pytest.fixture(scope="module")
def lib():
    _build.build()
    from diffuvolume_amd import _lib
    return _lib.load()


def test_header_declares_and_library_exports_the_entries(lib):
    from diffuvolume_amd import _lib
    header = (_build.PKG.parent / "include" / "diffuvolume_hip.h").read_text()
    for name in (*NEW, "dv_conv2d_wgrad_cat_f16_workspace_floats"):
        assert f" {name}(" in header, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert "update.py:26-142" in header[header.index("dv_conv2d_wgrad_cat_f16"):][:1200]
    assert (_build.CSRC / "conv2d_wgrad_cat_f16.hip").exists()


def test_argument_validation_without_gpu(lib):
    import ctypes
    ws = lib.dv_conv2d_wgrad_cat_f16_workspace_floats
    one, four, five = (ctypes.c_int * 1)(64), (ctypes.c_int * 4)(128, 128, 128, 128), (ctypes.c_int * 5)(8, 8, 8, 8, 8)
    assert ws(one, 1, 1, 4, 32, 64, 3) == 64 * 64 * 9                          # one 4 x 32 brick: one split
    assert ws(one, 1, 1, 4, 32, 64, 5) == 0                                    # k = 5
    assert ws(five, 5, 1, 4, 32, 64, 3) == 0                                   # five sources
    assert ws(one, 1, 0, 4, 32, 64, 3) == 0
    n = ws(four, 4, 4, 80, 184, 128, 3)
    assert n > 0 and n % (128 * 512 * 9) == 0 and n * 4 <= 48 << 20           # whole splits, bounded workspace
    fake = 256                                                                 # never dereferenced: rejected first
    ptrs = (ctypes.c_void_p * 1)(fake)
    assert lib.dv_conv2d_wgrad_cat_f16(ptrs, one, 1, fake, fake, fake, 1, 4, 32, 64, 5, None) == -3
    assert lib.dv_conv2d_wgrad_cat_f16(ptrs, one, 1, fake, fake, None, 1, 4, 32, 64, 3, None) == -1
    assert lib.dv_conv2d_wgrad_cat_f16(ptrs, one, 5, fake, fake, fake, 1, 4, 32, 64, 3, None) == -2
    assert lib.dv_gru_reset_mul_f16(fake, fake, None, 16, None) == -1
    assert lib.dv_gru_blend_f16(fake, fake, fake, fake, 0, None) == -2


def test_train_precision_switch_and_its_default():
    from diffuvolume_amd.synth import UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    block = BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)
    parts = (block, block.encoder, block.gru04, block.gru08, block.gru16, block.disp_head)
    assert all(m.train_precision == "f32" for m in parts)
    for bad in ("bf16", "fp16", None, 16):
        with pytest.raises(ValueError):
            block.set_train_precision(bad)
    assert all(m.train_precision == "f32" for m in parts)
    block.set_train_precision("f16")
    assert all(m.train_precision == "f16" for m in parts)
    block.set_train_precision("f32")
    assert all(m.train_precision == "f32" for m in parts)


def test_forward_train_has_the_amp_keyword():
    from diffuvolume_amd.igev_stereo_ddim import IGEVStereo_ddim
    p = inspect.signature(IGEVStereo_ddim.forward_train).parameters["amp"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
