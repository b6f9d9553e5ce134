"""Host-side checks of the cost-volume training route: the fixture tests/golden/igev_volume_train.npz (gate, shapes,
seeds), the shared synth helpers, the refusal of CPU tensors, the C ABI of the new kernels."""
import re
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _lib, synth, train3d
from diffuvolume_amd.igev_stereo_ddim import IGEVCostVolume

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("dv_deconv3d_k4s2_dgrad_packed_floats", "dv_deconv3d_k4s2_dgrad_pack_weights_f32",
               "dv_deconv3d_k4s2_dgrad_f32", "dv_deconv3d_k4s2_wgrad_workspace_floats", "dv_deconv3d_k4s2_wgrad_f32",
               "dv_feature_gate_bwd_workspace_floats", "dv_feature_gate_bwd_f32")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_volume_train.npz") as z:
        return {k: z[k] for k in z.files}


def test_fixture_gate_and_shapes(gold):
    assert float(gold["gate"]) == 1e-4 and float(gold["logit_gain"]) == 1.0
    assert [str(c) for c in gold["cases"]] == ["even", "tall"]
    template = IGEVCostVolume(64).state_dict()
    params = [n for n, _ in IGEVCostVolume(64).named_parameters()]
    for case, shape in (("even", (2, 16, 32, 64)), ("tall", (2, 8, 24, 192))):
        g = lambda k: gold[f"{case}_{k}"]
        b, h, w, max_disp = shape
        assert tuple(int(v) for v in g("shape")) == shape
        assert tuple(g("geo_shape")) == (b, 8, max_disp // 4, h, w) and tuple(g("init_shape")) == (b, 1, h, w)
        assert np.all(g("ref_err") > 0) and np.all(g("ref_err") < float(gold["gate"]))
        names, none = [str(n) for n in g("grad_names")], [str(n) for n in g("none_names")]
        assert sorted(names + none) == sorted(params)
        assert sorted(none) == ["cost_agg.conv1_up.bn.bias", "cost_agg.conv1_up.bn.weight"]     # bn=False: never called
        assert [str(n) for n in g("leaf_names")] == list(synth.IGEV_VOLUME_LEAVES)
        for tag in ("f32", "f64"):
            dt = np.float32 if tag == "f32" else np.float64
            assert g(f"grad_val_{tag}").shape == (len(names), 32) and g(f"grad_val_{tag}").dtype == dt
            assert g(f"leaf_val_{tag}").shape == (6, 32) and g(f"grad_norm_{tag}").shape == (len(names),)
            assert g(f"geo_{tag}").shape == (256,) and g(f"init_{tag}").shape == (256,)
            assert np.isfinite(g(f"loss_{tag}")) and np.all(g(f"grad_norm_{tag}") > 0)
            nbn = sum(template[str(k)].numel() for k in g("bn_names"))
            assert g(f"bn_{tag}").shape == (nbn,)
        assert [str(k) for k in g("bn_names")] == [k for k in template if k.endswith(("running_mean", "running_var"))]
    assert not any(k.endswith("weight") and gold[k].ndim > 2 for k in gold)                     # seeds, never weights


def test_synth_helpers_reproduce_the_stored_seeds(gold):
    assert int(gold["weight_seed"]) == synth.IGEV_VOLUME_TRAIN_WEIGHT_SEED == 91
    for case, c in synth.IGEV_VOLUME_TRAIN_CASES.items():
        assert int(gold[f"{case}_seed"]) == c["seed"]
        assert tuple(int(v) for v in gold[f"{case}_shape"]) == (c["b"], c["h"], c["w"], c["max_disp"])
    c = synth.IGEV_VOLUME_TRAIN_CASES["tall"]
    a, b = synth.igev_volume_train_inputs(**c), synth.igev_volume_train_inputs(dtype=torch.float64, **c)
    d = c["max_disp"] // 4
    assert a["gt"].shape == (2, 1, 8, 24) and float(a["gt"].min()) >= 0 and float(a["gt"].max()) <= d - 1
    assert a["cot"].shape == (2, 8, d, 8, 24)
    assert [tuple(f.shape) for f in a["features"]] == [(2, 96, 8, 24), (2, 64, 4, 12), (2, 192, 2, 6), (2, 160, 1, 3)]
    leaves = synth.igev_volume_train_leaves(a)
    assert list(leaves) == list(synth.IGEV_VOLUME_LEAVES) and all(t.requires_grad and t.is_leaf for t in leaves.values())
    for u, v in zip(leaves.values(), synth.igev_volume_train_leaves(b).values()):
        assert v.dtype == torch.float64 and torch.equal(u.detach().double(), v.detach())       # one draw, two precisions
    frozen = synth.igev_volume_train_inputs(requires_grad=False, **c)
    assert not any(t.requires_grad for t in synth.igev_volume_train_leaves(frozen).values())
    geo, init = torch.zeros_like(a["cot"]) + 2.0, a["gt"] + 0.5
    want = 0.125 + 2.0 * float(a["cot"].mean())                                                # smooth_l1(0.5) = 0.125
    assert abs(float(synth.igev_volume_train_loss(geo, init, a)) - want) < 1e-6


def test_cpu_tensors_raise_in_train_mode():
    c = synth.IGEV_VOLUME_TRAIN_CASES["even"]
    x = synth.igev_volume_train_inputs(**c)
    m = IGEVCostVolume(c["max_disp"]).train()
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        m(x["match_left"], x["match_right"], x["features"])
    with pytest.raises(DiffuVolumeError):
        m.cost_agg(torch.zeros(1, 8, 16, 16, 32), x["features"])
    with pytest.raises(DiffuVolumeError):
        train3d.conv_transpose3d_k4(torch.zeros(1, 16, 2, 2, 2), torch.zeros(16, 8, 4, 4, 4))
    with pytest.raises(DiffuVolumeError):
        train3d.feature_gate_train(torch.zeros(1, 8, 2, 2, 2), torch.zeros(1, 8, 2, 2))


def test_new_symbols_in_header_and_binding_table():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "diffuvolume_hip.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    text = (ROOT / "include" / "diffuvolume_hip.h").read_text()
    assert "igev_stereo_ddim.py:44-51" in text and "submodule.py:234-239" in text              # the reference lines served


def test_full_model_still_refuses_train_mode():
    from diffuvolume_amd.igev_stereo_ddim import Feature, IGEVStereo_ddim
    args = dict(hidden_dims=[128, 128, 128], n_gru_layers=3, n_downsample=2, corr_levels=2, corr_radius=4,
                slow_fast_gru=False, max_disp=192, mixed_precision=False)
    m = IGEVStereo_ddim(types.SimpleNamespace(**args), feature=Feature(synth.StubMobileNetV2())).train()
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 64, 128), torch.zeros(1, 3, 64, 128), torch.zeros(1, 1, 64, 128), torch.zeros(1, 1, 16, 32))
