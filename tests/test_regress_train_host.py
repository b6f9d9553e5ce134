"""The second table of the C ABI (include/diffuvolume_hip_train.h <-> _lib.TRAIN_SIGNATURES) and the switch of the
differentiable regression tail, as far as they can be checked without a GPU.

tests/test_abi.py ties _lib.SIGNATURES to diffuvolume_hip.h, and tests/test_abi_arena_complete.py forces a decision about
the pointer and bounds contract of every name in SIGNATURES.  This file does both for the second table: every name is
either an entry that only returns a size, or names the GPU test that holds its offset-view and bounds contract."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "diffuvolume_hip_train.h"

SIZE = "only returns a size: launches nothing"


def CONTRACT(test):
    return f"offset views, sentinel-guarded outputs and refusals are held by: {test}"


DECISIONS = {
    "dv_upsample_softmax_regress_bwd_workspace_floats": SIZE,
    "dv_upsample_softmax_regress_bwd_f32": CONTRACT("test_gpu_regress_train.py::test_abi_offset_views_bounds_and_refusals"),
}


def declarations():
    """name -> number of C parameters, from the header with its comments removed."""
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(dv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(params.split(","))
    return out


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_header_declares_exactly_the_second_table():
    from diffuvolume_amd import _lib
    decl = declarations()
    assert sorted(decl) == sorted(_lib.TRAIN_SIGNATURES) and decl
    for name, (_, args) in _lib.TRAIN_SIGNATURES.items():
        assert len(args) == decl[name], name


def test_library_exports_the_second_table(built):
    from diffuvolume_amd import _lib
    raw = ctypes.CDLL(str(built))
    for name in _lib.TRAIN_SIGNATURES:
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
    lib = _lib.load()                                             # load() types both tables
    fn = lib.dv_upsample_softmax_regress_bwd_workspace_floats
    assert fn.restype is ctypes.c_size_t and len(fn.argtypes) == 4
    assert fn(2, 48, 3, 5) == 0                                   # the fused path takes no workspace
    assert fn(2, 5, 3, 4) == 2 * 5 * 16 * 3 * 4                   # [B,D,4h,4w]
    assert fn(0, 48, 3, 5) == 0 and fn(2, 5, 3, -1) == 0
    # refused before anything touches the device
    bwd = lib.dv_upsample_softmax_regress_bwd_f32
    assert bwd(None, None, None, None, None, 1, 48, 1, 1, 0, None) == -1


def test_the_two_tables_are_disjoint():
    from diffuvolume_amd import _lib
    assert not set(_lib.TRAIN_SIGNATURES) & set(_lib.SIGNATURES)
    main = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "diffuvolume_hip.h").read_text(), flags=re.S)
    for name in _lib.TRAIN_SIGNATURES:
        assert not re.search(rf"\b{name}\s*\(", main), name


def test_every_training_entry_has_a_decision_and_the_named_tests_exist():
    from diffuvolume_amd import _lib
    assert set(DECISIONS) == set(_lib.TRAIN_SIGNATURES), set(DECISIONS) ^ set(_lib.TRAIN_SIGNATURES)
    here = Path(__file__).resolve().parent
    for name, why in DECISIONS.items():
        assert isinstance(why, str) and len(why) > 20
        if why == SIZE:
            assert _lib.TRAIN_SIGNATURES[name][0] is ctypes.c_size_t, name
            continue
        fname, test = why.split("held by: ")[1].split("::")
        text = (here / fname).read_text()
        assert f"def {test}(" in text and name in text, (name, why)


def test_switch_is_listed_and_documented(monkeypatch):
    from diffuvolume_amd import _env, train_tail
    assert _env.KNOBS["DV_TRAIN_TAIL"][0] == "hip"
    assert "DV_TRAIN_TAIL" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_TAIL", raising=False)
    assert train_tail.route() == "hip"
    monkeypatch.setenv("DV_TRAIN_TAIL", "torch")
    assert train_tail.route() == "torch"                           # read on every call
    monkeypatch.setenv("DV_TRAIN_TAIL", "cpu")
    with pytest.raises(ValueError):
        train_tail.route()


def test_cpu_tensors_raise():
    import torch
    import diffuvolume_amd as dv
    cost = torch.zeros(1, 48, 2, 2, requires_grad=True)
    with pytest.raises(dv.DiffuVolumeError):
        dv.upsample_softmax_regress_train(cost)
    with pytest.raises(dv.DiffuVolumeError):
        dv.upsample_softmax_regress_train(cost.unsqueeze(1), align_corners=True)
