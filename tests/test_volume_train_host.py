"""The third table of the C ABI (include/diffuvolume_hip_volume_train.h <-> _lib.VOLUME_TRAIN_SIGNATURES) and the switch of
the differentiable cost-volume builders, as far as they can be checked without a GPU.

The table carries, beside each signature, the decision about the entry's pointer and bounds contract: `_lib.SIZE_ONLY`, or
`_lib.held_by(<file>::<test>)` naming the GPU test that holds it.  This file owns no list of names: a later training
entry is a row of that table and a declaration in that header, and everything below then applies to it."""
import ctypes
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
HEADER = INCLUDE / "diffuvolume_hip_volume_train.h"


def declarations(header):
    """name -> number of C parameters, from a header with its comments removed."""
    text = re.sub(r"/\*.*?\*/", "", header.read_text(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\b(dv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        out[name] = 0 if params in ("", "void") else len(params.split(","))
    return out


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_header_declares_exactly_the_third_table():
    from diffuvolume_amd import _lib
    decl = declarations(HEADER)
    assert sorted(decl) == sorted(_lib.VOLUME_TRAIN_SIGNATURES) and decl
    for name, (_, args, _) in _lib.VOLUME_TRAIN_SIGNATURES.items():
        assert len(args) == decl[name], name
    assert {"dv_gwc_volume_bwd_f32", "dv_concat_volume_bwd_f32"} <= set(decl)


def test_library_exports_the_third_table(built):
    from diffuvolume_amd import _lib
    raw = ctypes.CDLL(str(built))
    for name in _lib.VOLUME_TRAIN_SIGNATURES:
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
    lib = _lib.load()                                             # load() types all three tables
    for name, (res, args, _) in _lib.VOLUME_TRAIN_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == len(args), name
    ws = lib.dv_concat_volume_bwd_workspace_floats
    assert ws(4, 32, 64, 128, 48) == 4 * (4 * 48 * 64 * 128)      # four chunks of 8 channels, [B,D,H,W] each
    assert ws(4, 8, 64, 128, 48) == 0                             # one chunk: ds is written directly
    assert ws(2, 12, 3, 11, 5) == 0                               # W % 4 != 0: the generic kernels take no workspace
    assert ws(0, 32, 64, 128, 48) == 0 and ws(4, 32, 64, -1, 48) == 0
    # refused before anything touches the device
    assert lib.dv_gwc_volume_bwd_f32(None, None, None, None, None, 1, 8, 1, 4, 1, 2, None) == -1
    assert lib.dv_concat_volume_bwd_f32(None, None, None, None, None, None, None, None, 1, 8, 1, 4, 1, 0, None) == -1
    assert b"NULL" in lib.dv_error_string(-1)


def test_the_three_tables_and_headers_are_disjoint():
    from diffuvolume_amd import _lib
    third = set(_lib.VOLUME_TRAIN_SIGNATURES)
    assert not third & set(_lib.SIGNATURES) and not third & set(_lib.TRAIN_SIGNATURES)
    for other in ("diffuvolume_hip.h", "diffuvolume_hip_train.h"):
        assert not third & set(declarations(INCLUDE / other)), other
    assert not set(declarations(HEADER)) & (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES))


def test_every_entry_names_its_decision_and_the_named_tests_exist():
    from diffuvolume_amd import _lib
    here = Path(__file__).resolve().parent
    held = 0
    for name, (res, _, why) in _lib.VOLUME_TRAIN_SIGNATURES.items():
        assert isinstance(why, str) and len(why) > 20, name
        if why == _lib.SIZE_ONLY:
            assert res is ctypes.c_size_t, name
            continue
        assert why == _lib.held_by(why.split("held by: ")[1]), name
        fname, test = why.split("held by: ")[1].split("::")
        text = (here / fname).read_text()
        assert f"def {test}(" in text and name in text, (name, why)
        assert "pytest.mark.gpu" in text, fname
        held += 1
    assert held >= 2


def test_switch_is_listed_and_documented(monkeypatch):
    from diffuvolume_amd import _env, train_volume
    assert _env.KNOBS["DV_TRAIN_VOLUME"][0] == "hip"
    assert "DV_TRAIN_VOLUME" in (ROOT / "INTEGRATION.md").read_text()
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    assert train_volume.route() == "hip"
    monkeypatch.setenv("DV_TRAIN_VOLUME", "torch")
    assert train_volume.route() == "torch"                         # read on every call
    monkeypatch.setenv("DV_TRAIN_VOLUME", "cpu")
    with pytest.raises(ValueError):
        train_volume.route()


def test_cpu_tensors_raise_in_the_train_functions(monkeypatch):
    import torch
    import diffuvolume_amd as dv
    ref = torch.zeros(1, 8, 2, 4, requires_grad=True)
    tgt = torch.zeros(1, 8, 2, 4)
    for route in ("hip", "torch"):
        monkeypatch.setenv("DV_TRAIN_VOLUME", route)
        with pytest.raises(dv.DiffuVolumeError):
            dv.build_gwc_volume_train(ref, tgt, 2, 4)
        with pytest.raises(dv.DiffuVolumeError):
            dv.build_concat_volume_train(ref, tgt, 2)
        with pytest.raises(dv.DiffuVolumeError):
            dv.build_concat_volume_train(ref, tgt, 2, scale=torch.ones(1, 2, 2, 4))


def test_the_builders_keep_the_statement_for_cpu_tensors(monkeypatch):
    """CPU tensors that require a gradient do not reach the train functions: the PyTorch statement, as before."""
    import torch
    import diffuvolume_amd as dv
    from diffuvolume_amd.submodule import _concat_volume_autograd, _gwc_volume_autograd
    monkeypatch.delenv("DV_TRAIN_VOLUME", raising=False)
    gen = torch.Generator().manual_seed(5)
    ref = torch.randn(2, 8, 3, 6, generator=gen).requires_grad_(True)
    tgt = torch.randn(2, 8, 3, 6, generator=gen).requires_grad_(True)
    vol = dv.build_gwc_volume(ref, tgt, 4, 2)
    assert vol.requires_grad and torch.equal(vol, _gwc_volume_autograd(ref, tgt, 4, 2))
    assert "VolumeFn" not in vol.grad_fn.name()
    vol.sum().backward()
    assert ref.grad is not None and tgt.grad is not None
    for zl in (False, True):
        cv = dv.build_concat_volume(ref, tgt, 4, zero_left=zl)
        assert cv.requires_grad and torch.equal(cv, _concat_volume_autograd(ref, tgt, 4, zl))
        assert "VolumeFn" not in cv.grad_fn.name()
