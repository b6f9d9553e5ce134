"""The fifth table of the C ABI (include/diffuvolume_hip_amp3d_bf16.h <-> _lib.AMP3D_BF16_SIGNATURES), train precision
"bf16" of ACVNet_DDIM / PWCNet_ddim and the machine code of the four mixed-precision kernel files (one body in
csrc/conv3d_mp.h / csrc/conv3d_wgrad_mp.h, instantiated for fp16 and for bf16), as far as they can be checked without a
GPU.  The method is tests/test_amp3d_host.py's, which pins the fourth table and stays as it is."""
import ctypes
import re
import subprocess
import threading
from pathlib import Path

import pytest
import torch

from test_volume_train_host import declarations

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
HEADER = INCLUDE / "diffuvolume_hip_amp3d_bf16.h"
ENTRIES = {"dv_conv3d_k3s1_bf16_f32", "dv_conv3d_wgrad_bf16_workspace_floats", "dv_conv3d_wgrad_bf16_f32"}
FILES = {"conv3d_f16": "f16", "conv3d_wgrad_f16": "f16", "conv3d_bf16": "bf16", "conv3d_wgrad_bf16": "bf16"}


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_header_declares_exactly_the_fifth_table():
    from diffuvolume_amd import _lib
    decl = declarations(HEADER)
    assert set(decl) == set(_lib.AMP3D_BF16_SIGNATURES) == ENTRIES
    text = HEADER.read_text()
    for name, (res, args, _) in _lib.AMP3D_BF16_SIGNATURES.items():
        assert len(args) == decl[name], name
        twin = _lib.AMP3D_SIGNATURES[name.replace("_bf16", "_f16")]          # the signatures of the fp16 twins
        assert (res, args) == twin[:2], name
        if res is ctypes.c_int:                                   # a launching entry: stream last, int return code
            assert args[-1] is _lib.P and re.search(rf"\bint\s+{name}\s*\([^)]*dv_stream_t\s+stream\s*\)", text), name
    assert "may be flushed to zero" in text and "v_cvt_pk_bf16_f32" in text


def test_the_fifth_table_is_disjoint_from_the_other_four():
    from diffuvolume_amd import _lib
    fifth = set(_lib.AMP3D_BF16_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VOLUME_TRAIN_SIGNATURES)
              | set(_lib.AMP3D_SIGNATURES))
    assert not fifth & others
    for other in ("diffuvolume_hip.h", "diffuvolume_hip_train.h", "diffuvolume_hip_volume_train.h",
                  "diffuvolume_hip_amp3d.h"):
        assert not fifth & set(declarations(INCLUDE / other)), other
    assert not set(declarations(HEADER)) & others


def test_every_entry_names_its_decision_and_the_named_tests_exist():
    from diffuvolume_amd import _lib
    here = Path(__file__).resolve().parent
    held = 0
    for name, (res, _, why) in _lib.AMP3D_BF16_SIGNATURES.items():
        assert isinstance(why, str) and len(why) > 20, name
        if why == _lib.SIZE_ONLY:
            assert res is ctypes.c_size_t, name
            continue
        assert why == _lib.held_by(why.split("held by: ")[1]), name
        fname, test = why.split("held by: ")[1].split("::")
        text = (here / fname).read_text()
        assert f"def {test}(" in text and name in text, (name, why)
        assert "pytest.mark.gpu" in text and "import arena" in text and "import streams" in text, fname
        held += 1
    assert held == 2


def test_no_hook_no_packer_no_switch():
    from diffuvolume_amd import _env, _lib
    for name in _lib.AMP3D_BF16_SIGNATURES:
        assert "_set_" not in name and "_pack_weights" not in name and "packed" not in name, name
    assert not [k for k in _env.KNOBS if "BF16" in k]
    csrc = ROOT / "diffuvolume_amd" / "csrc"
    for f in ("conv3d_bf16.hip", "conv3d_wgrad_bf16.hip", "conv3d_mp.h", "conv3d_wgrad_mp.h", "mp_elem.h"):
        assert "getenv" not in (csrc / f).read_text(), f


def test_library_exports_and_load_types_the_fifth_table(built):
    from diffuvolume_amd import _lib
    raw = ctypes.CDLL(str(built))
    for name in _lib.AMP3D_BF16_SIGNATURES:
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
    lib = _lib.load()
    for name, (res, args, _) in _lib.AMP3D_BF16_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == len(args), name
    # refused before anything touches the device
    assert lib.dv_conv3d_k3s1_bf16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, 3, 0, None) == -1
    assert lib.dv_conv3d_k3s1_bf16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, 1, 0, None) == -3
    assert lib.dv_conv3d_wgrad_bf16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, None) == -1


def test_the_size_entry_shares_the_fp16_plan(built):
    from diffuvolume_amd import _lib
    lib = _lib.load()
    for args in [(1, 8, 2, 2, 32, 8), (1, 8, 2, 2, 64, 8), (3, 128, 4, 6, 33, 128), (4, 64, 48, 64, 128, 32),
                 (0, 8, 2, 2, 8, 8), (1, 1024, 2, 2, 8, 1024), (1, 8, 1 << 10, 1 << 10, 1 << 10, 8)]:
        assert lib.dv_conv3d_wgrad_bf16_workspace_floats(*args) == lib.dv_conv3d_wgrad_f16_workspace_floats(*args), args
    assert lib.dv_conv3d_wgrad_bf16_workspace_floats(1, 8, 2, 2, 64, 8) == 2 * 8 * 8 * 27


# ------------------------------------------------------------------ the train-precision switch
@pytest.mark.parametrize("cls", ["ACVNet_DDIM", "PWCNet_ddim"])
def test_set_train_precision_takes_the_dtypes_autocast_names(cls):
    import diffuvolume_amd as dv
    model = getattr(dv, cls)(192)
    assert model.train_precision == "f32"
    assert model.set_train_precision(torch.bfloat16) is model and model.train_precision == "bf16"
    assert model.set_train_precision(torch.float16).train_precision == "f16"
    assert model.set_train_precision(torch.bfloat16).train_precision == "bf16"
    for bad in (torch.float64, "bf16", torch.int8, "bfloat16", True):
        with pytest.raises(ValueError):
            model.set_train_precision(bad)
    assert model.train_precision == "bf16"                         # a refused value changes nothing
    assert model.set_train_precision(torch.float32).train_precision == "f32"
    assert model.set_train_precision("f16").train_precision == "f16"
    assert not [k for k in model.state_dict() if "precision" in k]


def test_precision_scope_bf16_is_per_thread_and_restored():
    from diffuvolume_amd import train3d
    assert train3d.PRECISIONS == ("f32", "f16", "bf16")
    assert train3d.ambient_precision() == "f32"
    seen = {}

    def other():
        seen["before"] = train3d.ambient_precision()
        with train3d.precision_scope("f16"):
            seen["inside"] = train3d.ambient_precision()
        seen["after"] = train3d.ambient_precision()

    with train3d.precision_scope("bf16"):
        assert train3d.ambient_precision() == "bf16"
        with train3d.precision_scope("f16"):
            assert train3d.ambient_precision() == "f16"
        assert train3d.ambient_precision() == "bf16"
        t = threading.Thread(target=other)
        t.start()
        t.join()
        assert train3d.ambient_precision() == "bf16"
    assert train3d.ambient_precision() == "f32"
    assert seen == {"before": "f32", "inside": "f16", "after": "f32"}    # a new thread starts at the default
    with pytest.raises(RuntimeError):
        with train3d.precision_scope("bf16"):
            raise RuntimeError("inside")
    assert train3d.ambient_precision() == "f32"
    with pytest.raises(ValueError):
        with train3d.precision_scope(torch.bfloat16):                  # the scope takes the names only
            pass


def test_public_surface_and_documents():
    import diffuvolume_amd as dv
    for name in ("conv3d_k3s1_bf16", "conv3d_weight_grad_bf16", "conv3d_k3s1_f16", "conv3d_weight_grad_f16"):
        assert name in dv.__all__ and callable(getattr(dv, name)), name
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "set_train_precision(torch.bfloat16)" in integration
    assert "conv3d_wgrad_bf16" in (ROOT / "DESIGN.md").read_text()
    assert "train_step_amp_bf16_bench" in (ROOT / "README.md").read_text()
    assert (ROOT / "profiles" / "train_step_amp_bf16_bench.json").exists()


# ------------------------------------------------------------------ the machine code
@pytest.fixture(scope="module", params=sorted(FILES))
def isa(request, tmp_path_factory):
    from diffuvolume_amd import _build
    out = tmp_path_factory.mktemp("isa") / f"{request.param}.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / f"{request.param}.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return FILES[request.param], out.read_text()


def test_each_file_is_one_kernel_on_its_own_matrix_instruction_without_spills(isa):
    elem, text = isa
    other = {"f16": "bf16", "bf16": "f16"}[elem]
    matrix = set(re.findall(r"\bv_mfma_\w+", text))
    assert matrix == {f"v_mfma_f32_16x16x32_{elem}"}, matrix          # its own instruction and no other (none of the twin's)
    assert f"v_mfma_f32_16x16x32_{other}" not in text
    assert ("v_cvt_pk_bf16_f32" in text) == (elem == "bf16")            # the hardware rounding, in the bf16 files only
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", text)]
    assert len(spills) == 1 and spills == [0]            # one kernel per file (SGPR spills go to VGPR lanes, not memory)
    assert private == [0]
