"""Host-side checks of the upsampling head's training route: the fixture tests/golden/igev_upsample_train.npz (gate,
shapes, seeds), the shared synth helpers, the refusal of CPU tensors, the C ABI of the new kernels."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _lib, synth, train2d
from diffuvolume_amd.igev_stereo_ddim import IGEVUpsampler, context_upsample

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("dv_context_upsample_bwd_f32", "dv_deconv2d_k4s2_wgrad_workspace_floats", "dv_deconv2d_k4s2_wgrad_f32")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_upsample_train.npz") as z:
        return {k: z[k] for k in z.files}


def test_fixture_gate_and_shapes(gold):
    assert float(gold["gate"]) == 1e-4 and float(gold["logit_gain"]) == 1.0
    assert [str(c) for c in gold["cases"]] == ["even", "odd"]
    template = IGEVUpsampler().state_dict()
    params = [n for n, _ in IGEVUpsampler().named_parameters()]
    for case, shape in (("even", (2, 8, 16, 3)), ("odd", (1, 5, 7, 2))):
        g = lambda k: gold[f"{case}_{k}"]
        b, h, w, iters = shape
        assert tuple(int(v) for v in g("shape")) == shape
        assert tuple(g("up_shape")) == (b, 1, 4 * h, 4 * w)
        assert np.all(g("ref_err") > 0) and np.all(g("ref_err") < float(gold["gate"]))
        names = [str(n) for n in g("grad_names")]
        assert sorted(names) == sorted(params)                                  # every parameter gets a gradient
        leaves = [str(n) for n in g("leaf_names")]
        assert leaves == [f"{n}_{i}" for i in range(iters) for n in ("mask_feat_4", "disp")] + ["stem_2x", "feat0", "init_disp"]
        for tag in ("f32", "f64"):
            dt = np.float32 if tag == "f32" else np.float64
            assert g(f"grad_val_{tag}").shape == (len(names), 32) and g(f"grad_val_{tag}").dtype == dt
            assert g(f"leaf_val_{tag}").shape == (len(leaves), 32) and g(f"grad_norm_{tag}").shape == (len(names),)
            assert g(f"init_{tag}").shape == (256,) and g(f"up_{tag}").shape == (iters, 256)
            assert np.isfinite(g(f"loss_{tag}")) and np.all(g(f"grad_norm_{tag}") > 0) and np.all(g(f"leaf_norm_{tag}") > 0)
            nbn = sum(template[str(k)].numel() for k in g("bn_names"))
            assert g(f"bn_{tag}").shape == (nbn,)
        assert [str(k) for k in g("bn_names")] == [k for k in template if k.endswith(("running_mean", "running_var"))]
    assert not any(k.endswith("weight") and gold[k].ndim > 2 for k in gold)     # seeds, never weights


def test_synth_helpers_reproduce_the_stored_seeds(gold):
    assert int(gold["weight_seed"]) == synth.IGEV_UPSAMPLE_TRAIN_WEIGHT_SEED == 93
    for case, c in synth.IGEV_UPSAMPLE_TRAIN_CASES.items():
        assert int(gold[f"{case}_seed"]) == c["seed"]
        assert tuple(int(v) for v in gold[f"{case}_shape"]) == (c["b"], c["h"], c["w"], c["iters"])
    c = synth.IGEV_UPSAMPLE_TRAIN_CASES["odd"]
    a, b = synth.igev_upsample_train_inputs(**c), synth.igev_upsample_train_inputs(dtype=torch.float64, **c)
    assert [tuple(t.shape) for t in a["mask_feat_4"]] == [(1, 32, 5, 7)] * 2 and all(float(t.detach().min()) >= 0 for t in a["mask_feat_4"])
    assert [tuple(t.shape) for t in a["disp"]] == [(1, 1, 5, 7)] * 2
    assert a["stem_2x"].shape == (1, 32, 10, 14) and a["feat0"].shape == (1, 96, 5, 7) and a["init_disp"].shape == (1, 1, 5, 7)
    assert a["gt"].shape == (1, 1, 20, 28) and not a["gt"].requires_grad and float(a["gt"].min()) >= 1
    leaves = synth.igev_upsample_train_leaves(a)
    assert len(leaves) == 7 and all(t.requires_grad and t.is_leaf for t in leaves.values())
    for u, v in zip(leaves.values(), synth.igev_upsample_train_leaves(b).values()):
        assert v.dtype == torch.float64 and torch.equal(u.detach().double(), v.detach())       # one draw, two precisions
    frozen = synth.igev_upsample_train_inputs(requires_grad=False, **c)
    assert not any(t.requires_grad for t in synth.igev_upsample_train_leaves(frozen).values())
    sd1 = synth.igev_upsample_state_dict(IGEVUpsampler().state_dict(), 93, 1.0)
    sd2 = synth.igev_upsample_state_dict(IGEVUpsampler().state_dict(), 93, 0.5)
    for k in sd1:
        assert torch.equal(sd2[k], sd1[k] * 0.5 if k in synth.IGEV_UPSAMPLE_LOGIT_HEADS else sd1[k]), k
    IGEVUpsampler().load_state_dict(sd1, strict=True)

    class Stub:                                       # the loss on known outputs: |1| + (0.9 * |2| + 1.0 * |3|)
        def __init__(self):
            self.n = 0

        def __call__(self, disp, mask, stem):
            self.n += 1
            return a["gt"] + (self.n + 1.0)

        def init_forward(self, feat0, stem, init):
            return a["gt"] - 1.0
    loss, init_up, ups = synth.igev_upsample_train_step(Stub(), a)
    assert len(ups) == 2 and abs(float(loss) - (1.0 + 0.9 * 2.0 + 3.0)) < 1e-5


def test_cpu_tensors_raise():
    c = synth.IGEV_UPSAMPLE_TRAIN_CASES["odd"]
    x = synth.igev_upsample_train_inputs(**c)
    m = IGEVUpsampler().train()
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        m(x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        m.init_forward(x["feat0"], x["stem_2x"], x["init_disp"])
    with pytest.raises(DiffuVolumeError):
        m.spx_2_gru.conv1.train_forward(x["mask_feat_4"][0])
    with pytest.raises(DiffuVolumeError):
        train2d.conv_transpose2d_k4(torch.zeros(1, 8, 2, 2), torch.zeros(8, 3, 4, 4, requires_grad=True))
    with pytest.raises(DiffuVolumeError):
        context_upsample(x["disp"][0], torch.zeros(1, 9, 20, 28))
    with pytest.raises(DiffuVolumeError):                                      # eval mode: the inference route, no CPU path either
        with torch.no_grad():
            m.eval()(x["disp"][0], x["mask_feat_4"][0], x["stem_2x"])


def test_unsupported_transposed_geometry_raises():
    for m in (torch.nn.ConvTranspose2d(8, 3, 4, 2, 0), torch.nn.ConvTranspose2d(8, 3, 3, 2, 1),
              torch.nn.ConvTranspose2d(8, 3, 4, 1, 1), torch.nn.ConvTranspose2d(8, 4, 4, 2, 1, groups=2),
              torch.nn.ConvTranspose2d(8, 3, 4, 2, 1, output_padding=1), torch.nn.Conv2d(8, 3, 3, 1, 1)):
        with pytest.raises(DiffuVolumeError):
            train2d.conv_transpose2d_module(m, torch.zeros(1, 8, 2, 2))
    with pytest.raises(DiffuVolumeError):
        train2d.conv_transpose2d_k4(torch.zeros(1, 8, 2, 2), torch.zeros(8, 3, 3, 3))


def test_new_symbols_in_header_and_binding_table():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "diffuvolume_hip.h").read_text(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    text = (ROOT / "include" / "diffuvolume_hip.h").read_text()
    assert "igev_stereo_ddim.py:203-211" in text and "igev_stereo_ddim.py:110-112" in text      # the reference lines served


def test_kernel_argument_validation_without_gpu():
    lib = _lib.load()
    assert lib.dv_deconv2d_k4s2_wgrad_workspace_floats(1, 8, 1, 3, 3) == 8 * 3 * 16          # one brick: one split
    assert lib.dv_deconv2d_k4s2_wgrad_workspace_floats(0, 8, 1, 3, 3) == 0
    assert lib.dv_deconv2d_k4s2_wgrad_workspace_floats(4, 64, 160, 368, 9) % (64 * 9 * 16) == 0
    assert lib.dv_deconv2d_k4s2_wgrad_f32(None, None, None, None, 1, 8, 1, 3, 3, None) == -1
    assert lib.dv_context_upsample_bwd_f32(None, None, None, None, None, None, 1, 2, 2, 4.0, 1, None) == -1
