"""Host-side checks of the geometry lookup's training route: the C ABI of the new kernels, the switch, the fixture
tests/golden/igev_lookup_train.npz (gate, shapes, seeds) and the pin of the oracle's gradient to the reference: the
fixture's float64 numbers (from the imported reference class, tools/make_golden_igev_lookup_train.py) are reproduced by
float64 autograd of oracle.igev_oracle.geo_filter_lookup on the same seeded inputs.

Bound of that pin: both sides are float64 expressions of the same sums and both round the cotangent / numel to float32
once at their closing `.float()`, so they differ by float64 summation order only: 1e-12 relative L2 (measured 2e-16)."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from diffuvolume_amd import DiffuVolumeError, _env, _lib, synth
from diffuvolume_amd.geometry_ddim import Combined_Geo_Encoding_Volume
from oracle.igev_oracle import geo_filter_lookup

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("dv_geo_filter_lookup_bwd_f32", "dv_allpairs_corr_bwd_f32")


@pytest.fixture(scope="module")
def gold():
    with np.load(GOLDEN / "igev_lookup_train.npz") as z:
        return {k: z[k] for k in z.files}


def test_new_symbols_in_header_and_binding_table():
    text = (ROOT / "include" / "diffuvolume_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES, name
    for cite in ("geometry_ddim.py:33-69", "geometry_ddim.py:72-80", "igev_stereo_ddim.py:441-443"):
        assert cite in text, cite


def test_switch_is_registered(monkeypatch):
    from diffuvolume_amd import geometry_ddim
    assert _env.KNOBS["DV_TRAIN_LOOKUP"][0] == "hip"
    assert "DV_TRAIN_LOOKUP" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_LOOKUP", raising=False)
    assert geometry_ddim.route() == "hip"
    monkeypatch.setenv("DV_TRAIN_LOOKUP", "torch")
    assert geometry_ddim.route() == "torch" and _env.overrides()["DV_TRAIN_LOOKUP"] == "torch"
    monkeypatch.setenv("DV_TRAIN_LOOKUP", "triton")
    with pytest.raises(ValueError):
        geometry_ddim.route()


def test_kernel_argument_validation_without_gpu():
    """Null pointers and radius != 4 are rejected before any device call (the pointers are never dereferenced)."""
    lib = _lib.load()
    one = 16                                          # any non-null address: validation must return before using it
    dims = (1, 8, 48, 2, 5, 5)
    assert lib.dv_geo_filter_lookup_bwd_f32(None, one, one, one, one, one, *dims, 4, None) == -1
    assert lib.dv_geo_filter_lookup_bwd_f32(one, None, one, one, one, one, *dims, 4, None) == -1
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, None, one, one, one, *dims, 4, None) == -1
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, one, None, one, one, *dims, 4, None) == -1
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, one, one, None, None, *dims, 4, None) == -1
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, one, one, one, None, *dims, 3, None) == -3
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, one, one, None, one, *dims, 5, None) == -3
    assert lib.dv_geo_filter_lookup_bwd_f32(one, one, one, one, one, one, 1, 8, 3, 2, 5, 5, 4, None) == -2
    assert lib.dv_allpairs_corr_bwd_f32(None, one, one, one, one, 1, 8, 2, 3, 3, None) == -1
    assert lib.dv_allpairs_corr_bwd_f32(one, one, one, None, None, 1, 8, 2, 3, 3, None) == -1
    assert lib.dv_allpairs_corr_bwd_f32(one, one, one, one, one, 1, 257, 2, 3, 3, None) == -3
    assert lib.dv_allpairs_corr_bwd_f32(one, one, one, one, one, 1, 8, 0, 3, 3, None) == -2


def test_cpu_tensors_raise():
    x = synth.igev_lookup_train_inputs(**synth.IGEV_LOOKUP_TRAIN_CASES["odd"])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        Combined_Geo_Encoding_Volume(x["fmap1"], x["fmap2"], x["geo"])
    with pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        Combined_Geo_Encoding_Volume(x["fmap1"].detach(), x["fmap2"].detach(), x["geo"])
    with torch.no_grad(), pytest.raises(DiffuVolumeError, match="no CPU fallback"):
        Combined_Geo_Encoding_Volume(x["fmap1"], x["fmap2"], x["geo"])


def test_fixture_gate_shapes_and_seeds(gold):
    assert float(gold["gate"]) == 1e-4
    assert [str(c) for c in gold["cases"]] == ["even", "odd"] == list(synth.IGEV_LOOKUP_TRAIN_CASES)
    assert [str(k) for k in gold["kinds"]] == ["df1", "df2", "dgeo"]
    assert tuple(str(k) for k in gold["leaves"]) == synth.IGEV_LOOKUP_LEAVES == ("fmap1", "fmap2", "geo")
    for case, shape in (("even", (2, 8, 48, 8, 24, 3)), ("odd", (1, 8, 48, 5, 7, 2))):
        g = lambda k: gold[f"{case}_{k}"]
        c = synth.IGEV_LOOKUP_TRAIN_CASES[case]
        assert tuple(int(v) for v in g("shape")) == shape == tuple(c[k] for k in ("b", "c", "d", "h", "w", "iters"))
        assert int(g("seed")) == c["seed"]
        assert g("ref_err").shape == (3,) and np.all(g("ref_err") > 0) and np.all(g("ref_err") < float(gold["gate"]))
        assert g("grad_idx").shape == (3, 512)
        for tag, dt in (("f32", np.float32), ("f64", np.float64)):
            assert g(f"grad_val_{tag}").shape == (3, 512) and g(f"grad_val_{tag}").dtype == dt
            assert g(f"grad_norm_{tag}").shape == (3,) and np.all(g(f"grad_norm_{tag}") > 0) and np.isfinite(g(f"loss_{tag}"))
    assert all(v.size <= 3 * 512 for v in gold.values())                     # seeds, norms and samples, never whole tensors
    assert (GOLDEN / "igev_lookup_train.npz").stat().st_size < 100 * 1024


def test_synth_helpers():
    c = synth.IGEV_LOOKUP_TRAIN_CASES["odd"]
    a, b = synth.igev_lookup_train_inputs(**c), synth.igev_lookup_train_inputs(dtype=torch.float64, **c)
    assert a["geo"].shape == (1, 8, 48, 5, 7) and a["fmap1"].shape == a["fmap2"].shape == (1, 96, 5, 7)
    assert len(a["disp"]) == len(a["noisy"]) == len(a["cot"]) == 2
    assert a["disp"][0].shape == a["coords"].shape == (1, 1, 5, 7) and a["noisy"][0].shape == (1, 48, 5, 7)
    assert a["cot"][0].shape == (1, 162, 5, 7) and torch.equal(a["coords"][0, 0, 0], torch.arange(7.0))
    assert not any(t.requires_grad for k in ("disp", "noisy", "cot") for t in a[k]) and not a["coords"].requires_grad
    assert min(float(t.min()) for t in a["disp"]) < 0 and max(float(t.max()) for t in a["disp"]) > 47     # both borders
    assert not torch.equal(a["disp"][0], a["disp"][1]) and not torch.equal(a["noisy"][0], a["noisy"][1])
    leaves = synth.igev_lookup_train_leaves(a)
    assert tuple(leaves) == synth.IGEV_LOOKUP_LEAVES and all(t.requires_grad and t.is_leaf for t in leaves.values())
    for u, v in zip(leaves.values(), synth.igev_lookup_train_leaves(b).values()):
        assert v.dtype == torch.float64 and torch.equal(u.detach().double(), v.detach())       # one draw, two precisions
    frozen = synth.igev_lookup_train_inputs(requires_grad=False, **c)
    assert not any(t.requires_grad for t in synth.igev_lookup_train_leaves(frozen).values())

    class Stub:                                       # the loss on known outputs: mean(cot0 * 1) + mean(cot1 * 2)
        def __init__(self, f1, f2, geo):
            self.n = 0

        def __call__(self, disp, coords, noisy):
            self.n += 1
            return torch.full((1, 162, 5, 7), float(self.n))
    loss, outs = synth.igev_lookup_train_step(Stub, a)
    assert len(outs) == 2 and abs(float(loss) - float(a["cot"][0].mean() + 2 * a["cot"][1].mean())) < 1e-6


class OracleVolume:
    """oracle.igev_oracle.geo_filter_lookup behind the class API that synth.igev_lookup_train_step drives."""

    def __init__(self, fmap1, fmap2, geo):
        self.args = (geo, fmap1, fmap2)

    def __call__(self, disp, coords, noisy):
        return geo_filter_lookup(*self.args, disp, coords, noisy)


@pytest.mark.parametrize("case", ["even", "odd"])
def test_oracle_float64_autograd_reproduces_the_fixture(gold, case):
    x = synth.igev_lookup_train_inputs(dtype=torch.float64, **synth.IGEV_LOOKUP_TRAIN_CASES[case])
    loss, _ = synth.igev_lookup_train_step(OracleVolume, x)
    loss.backward()
    assert abs(float(loss.detach()) - float(gold[f"{case}_loss_f64"])) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    for i, (name, t) in enumerate(synth.igev_lookup_train_leaves(x).items()):
        got = t.grad.reshape(-1)[torch.from_numpy(gold[f"{case}_grad_idx"][i])].numpy()
        want = gold[f"{case}_grad_val_f64"][i]
        e = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        n = abs(float(t.grad.norm()) - float(gold[f"{case}_grad_norm_f64"][i])) / float(gold[f"{case}_grad_norm_f64"][i])
        print(f"PIN {case} {name}: samples {e:.2e}  norm {n:.2e}")
        assert e <= 1e-12 and n <= 1e-12, (name, e, n)
