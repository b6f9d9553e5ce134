"""`mixed_precision=True` on CPU: IGEVStereo_ddim(args) and IGEVStereo(args) built from an `args` namespace of the
reference's scripts (train_stereo.py turns the flag on) construct and load a reference-shaped state_dict strictly; the
C header declares the fp16 update-block entry points."""
import types
from pathlib import Path

import torch

from diffuvolume_amd.synth import StubMobileNetV2, synth_state_dict

ROOT = Path(__file__).resolve().parents[1]
ARGS = dict(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2, corr_radius=4,
            slow_fast_gru=False, max_disp=192, mixed_precision=True)


def test_models_accept_mixed_precision_and_load_strictly():
    from diffuvolume_amd.igev_stereo import IGEVStereo
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    for cls in (IGEVStereo_ddim, IGEVStereo):
        m = cls(types.SimpleNamespace(**ARGS), feature=Feature(StubMobileNetV2()))
        sd = m.state_dict()
        m.load_state_dict(synth_state_dict(sd, seed=5), strict=True)
        assert m.args.mixed_precision is True
        assert "update_block.gru04.convz.weight" in sd and sd["update_block.gru04.convz.weight"].dtype == torch.float32


def test_loop_reads_the_flag_per_forward():
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    m = IGEVStereo_ddim(types.SimpleNamespace(**ARGS), feature=Feature(StubMobileNetV2()))
    assert m._loop().mixed_precision is True
    m.args.mixed_precision = False
    assert m._loop().mixed_precision is False


def test_fp16_rounding_of_the_loop_inputs():
    from diffuvolume_amd.igev_stereo_ddim import round_gru_inputs_f16
    net = [torch.randn(1, 4, 3, 5) for _ in range(3)]
    inp = [[torch.randn(1, 4, 3, 5) for _ in range(3)] for _ in range(3)]
    rn, ri = round_gru_inputs_f16(net, inp)
    for a, b in zip(rn + sum(ri, []), net + sum(inp, [])):
        assert a.dtype == torch.float32 and torch.equal(a, b.half().float())
    rn2, _ = round_gru_inputs_f16(rn, ri)
    assert all(torch.equal(a, b) for a, b in zip(rn, rn2))


def test_header_declares_the_fp16_entry_points():
    text = (ROOT / "include" / "diffuvolume_hip.h").read_text()
    for name in ("dv_conv2d_f16_packed_bytes", "dv_conv2d_f16_pack_weights", "dv_conv2d_f16_auto_kslices",
                 "dv_conv2d_f16_cat", "dv_conv2d_f16_cat_ksplit", "dv_conv2d_f16_cat_pair",
                 "dv_conv2d_f16_cat_pair_ksplit", "dv_conv2d_1in_f16"):
        assert f" {name}(" in text, name
