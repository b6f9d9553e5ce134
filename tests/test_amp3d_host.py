"""The fourth table of the C ABI (include/diffuvolume_hip_amp3d.h <-> _lib.AMP3D_SIGNATURES), the train-precision switch of
ACVNet_DDIM / PWCNet_ddim and the two fp16 kernels' machine code, as far as they can be checked without a GPU.

The table carries, beside each signature, the decision about the entry's pointer and bounds contract: `_lib.SIZE_ONLY`, or
`_lib.held_by(<file>::<test>)` naming the GPU test that holds it -- what tests/test_abi_arena_complete.py,
tests/test_stream_contract_host.py and tests/test_volume_train_host.py force for the first three tables."""
import ctypes
import json
import re
import subprocess
import threading
from pathlib import Path

import pytest

from test_volume_train_host import declarations

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
HEADER = INCLUDE / "diffuvolume_hip_amp3d.h"
FIXTURE = ROOT / "tests" / "golden" / "conv3d_wgrad_f16_plan.json"
ENTRIES = {"dv_conv3d_k3s1_f16_f32", "dv_conv3d_wgrad_f16_workspace_floats", "dv_conv3d_wgrad_f16_f32"}

MAX_WS_FLOATS = 12 << 20              # DV_WGRAD_MAX_WS_FLOATS (csrc/wgrad_splitk.h)
TZ, TY, TX, BLOCK, TARGET = 2, 2, 32, 32, 512


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_header_declares_exactly_the_fourth_table():
    from diffuvolume_amd import _lib
    decl = declarations(HEADER)
    assert set(decl) == set(_lib.AMP3D_SIGNATURES) == ENTRIES
    for name, (_, args, _) in _lib.AMP3D_SIGNATURES.items():
        assert len(args) == decl[name], name
    text = HEADER.read_text()
    for name, (res, args, _) in _lib.AMP3D_SIGNATURES.items():
        if res is ctypes.c_int:                                   # a launching entry: stream last, int return code
            assert args[-1] is _lib.P and re.search(rf"\bint\s+{name}\s*\([^)]*dv_stream_t\s+stream\s*\)", text), name


def test_the_fourth_table_is_disjoint_from_the_other_three():
    from diffuvolume_amd import _lib
    fourth = set(_lib.AMP3D_SIGNATURES)
    others = set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VOLUME_TRAIN_SIGNATURES)
    assert not fourth & others
    for other in ("diffuvolume_hip.h", "diffuvolume_hip_train.h", "diffuvolume_hip_volume_train.h"):
        assert not fourth & set(declarations(INCLUDE / other)), other
    assert not set(declarations(HEADER)) & others


def test_every_entry_names_its_decision_and_the_named_tests_exist():
    from diffuvolume_amd import _lib
    here = Path(__file__).resolve().parent
    held = 0
    for name, (res, _, why) in _lib.AMP3D_SIGNATURES.items():
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
    for name in _lib.AMP3D_SIGNATURES:
        assert "_set_" not in name and "_pack_weights" not in name and "packed" not in name, name
    before = {"DV_TRAIN_CONV3D"}
    assert before <= set(_env.KNOBS) and not [k for k in _env.KNOBS if "F16" in k and "3D" in k]
    for f in ("conv3d_f16.hip", "conv3d_wgrad_f16.hip"):
        text = (ROOT / "diffuvolume_amd" / "csrc" / f).read_text()
        assert "getenv" not in text and "DV_" not in re.sub(r"DV_(REQUIRE\w*|ERR_\w+|OK|WGRAD_MAX_WS_FLOATS)", "", text), f


def test_library_exports_and_load_types_the_fourth_table(built):
    from diffuvolume_amd import _lib
    raw = ctypes.CDLL(str(built))
    for name in _lib.AMP3D_SIGNATURES:
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
    lib = _lib.load()
    for name, (res, args, _) in _lib.AMP3D_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == len(args), name
    # refused before anything touches the device
    assert lib.dv_conv3d_k3s1_f16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, 3, 0, None) == -1
    assert lib.dv_conv3d_k3s1_f16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, 1, 0, None) == -3
    assert lib.dv_conv3d_wgrad_f16_f32(None, None, None, None, 1, 8, 2, 2, 8, 8, None) == -1


# ------------------------------------------------------------------ the workspace plan
def model_floats(b, cin, d, h, w, cout):
    """The plan of csrc/conv3d_wgrad_f16.hip through csrc/wgrad_splitk.h, in Python."""
    per = cout * cin * 27
    if min(b, cin, d, h, w, cout) < 1 or d * h * w >= 1 << 30 or per > MAX_WS_FLOATS:
        return 0
    nbricks = b * -(-d // TZ) * -(-h // TY) * -(-w // TX)
    mn = -(-cout // BLOCK) * -(-cin // BLOCK)
    splits = max(1, min(-(-TARGET // mn), MAX_WS_FLOATS // per, nbricks))
    return splits * per


def test_workspace_plan_is_pinned(built):
    from diffuvolume_amd import _lib
    lib = _lib.load()
    rows = json.loads(FIXTURE.read_text())["rows"]
    assert len(rows) >= 40
    splits = set()
    for r in rows:
        got = int(lib.dv_conv3d_wgrad_f16_workspace_floats(*r["args"]))
        assert got == r["floats"] == model_floats(*r["args"]), r
        assert got * 4 <= 48 << 20
        if got:
            b, cin, d, h, w, cout = r["args"]
            splits.add(got // (cout * cin * 27))
    assert sum(1 for r in rows if r["floats"] == 0) >= 14           # every refusal
    assert {1, 2, 512} <= splits and max(splits) == 512            # one brick, two bricks, the device-filling count
    assert (ROOT / "tools" / "make_golden_amp3d_plan.py").exists()


# ------------------------------------------------------------------ the train-precision switch
@pytest.mark.parametrize("cls", ["ACVNet_DDIM", "PWCNet_ddim"])
def test_set_train_precision_validates(cls):
    import diffuvolume_amd as dv
    model = getattr(dv, cls)(192)
    assert model.train_precision == "f32"
    assert model.set_train_precision("f16") is model and model.train_precision == "f16"
    for bad in ("bf16", "fp16", "", None, 16):
        with pytest.raises(ValueError):
            model.set_train_precision(bad)
    assert model.train_precision == "f16"
    assert model.set_train_precision("f32").train_precision == "f32"
    assert not [k for k in model.state_dict() if "precision" in k]


def test_precision_scope_is_per_thread_and_restored():
    from diffuvolume_amd import train3d
    assert train3d.ambient_precision() == "f32"
    seen = {}

    def other():
        seen["before"] = train3d.ambient_precision()
        with train3d.precision_scope("f16"):
            seen["inside"] = train3d.ambient_precision()

    with train3d.precision_scope("f16"):
        assert train3d.ambient_precision() == "f16"
        with train3d.precision_scope("f32"):
            assert train3d.ambient_precision() == "f32"
        assert train3d.ambient_precision() == "f16"
        t = threading.Thread(target=other)
        t.start()
        t.join()
    assert train3d.ambient_precision() == "f32"
    assert seen == {"before": "f32", "inside": "f16"}               # a new thread starts at the default
    with pytest.raises(ValueError):
        with train3d.precision_scope("f64"):
            pass
    with pytest.raises(RuntimeError):
        with train3d.precision_scope("f16"):
            raise RuntimeError("inside")
    assert train3d.ambient_precision() == "f32"
    assert train3d.takes_f16(3, 1, 32) and not train3d.takes_f16(3, 1, 1)
    assert not train3d.takes_f16(3, 2, 32) and not train3d.takes_f16(1, 1, 32)


def test_public_surface_and_documents():
    import diffuvolume_amd as dv
    for name in ("conv3d_train", "conv3d_k3s1_f16", "conv3d_weight_grad_f16", "train_precision_scope"):
        assert name in dv.__all__ and callable(getattr(dv, name)), name
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "set_train_precision" in integration and "GradScaler" in integration
    assert "conv3d_wgrad_f16" in (ROOT / "DESIGN.md").read_text()
    assert "train_step_amp_bench" in (ROOT / "README.md").read_text()


# ------------------------------------------------------------------ the machine code
@pytest.fixture(scope="module", params=["conv3d_f16", "conv3d_wgrad_f16"])
def isa(request, tmp_path_factory):
    from diffuvolume_amd import _build
    out = tmp_path_factory.mktemp("isa") / f"{request.param}.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / f"{request.param}.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return out.read_text()


def test_kernels_run_on_the_f16_matrix_instruction_without_spills(isa):
    assert "v_mfma_f32_16x16x32_f16" in isa
    assert "v_mfma_f32_16x16x4_f32" not in isa and not re.search(r"v_mfma_f32_\w+_f32\b", isa)
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert len(spills) == 1 and spills == [0]            # one kernel per file (SGPR spills go to VGPR lanes, not memory)
    assert private == [0]
