"""The sixth table of the C ABI (include/diffuvolume_hip_amp2d_bf16.h <-> _lib.AMP2D_BF16_SIGNATURES), train precision
"bf16" of IGEV's update block and the machine code of the four 16-bit kernel files of the block (one body in
csrc/conv2d_mp.h / csrc/conv2d_wgrad_cat_mp.h, instantiated for fp16 and for bf16), as far as they can be checked without a
GPU.  The method is tests/test_amp3d_bf16_host.py's, which pins the fifth table and stays as it is."""
import ctypes
import inspect
import re
import subprocess
import types
from pathlib import Path

import pytest
import torch

from test_volume_train_host import declarations

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "include"
HEADER = INCLUDE / "diffuvolume_hip_amp2d_bf16.h"
ENTRIES = {"dv_conv2d_bf16_pack_weights", "dv_conv2d_bf16_cat", "dv_conv2d_bf16_cat_ksplit", "dv_conv2d_bf16_cat_pair",
           "dv_conv2d_bf16_cat_pair_ksplit", "dv_conv2d_1in_bf16", "dv_gru_reset_mul_bf16", "dv_gru_blend_bf16",
           "dv_conv2d_wgrad_cat_bf16_workspace_floats", "dv_conv2d_wgrad_cat_bf16"}
FILES = {"conv2d_f16": "f16", "conv2d_wgrad_cat_f16": "f16", "conv2d_bf16": "bf16", "conv2d_wgrad_cat_bf16": "bf16"}

# What the parent commit's build (9a40de1, before the kernel bodies moved into the two headers) of the two fp16 files
# gives per kernel, compiled with _build.FLAGS for gfx950: (VGPRs, LDS bytes, scratch bytes).  The forward kernels are
# keyed by (k, N tiles), the weight-gradient kernels by k.
PARENT = "9a40de1"
PARENT_CONV2D_F16 = {(3, 4): (238, 74880, 0), (3, 1): (169, 47232, 0), (1, 4): (143, 28672, 0), (1, 1): (83, 25600, 0),
                     "ksplit_epilogue": (16, 0, 0), "pack": (14, 0, 0)}
PARENT_WGRAD_CAT_F16 = {1: (132, 40976, 0), 3: (452, 49168, 0)}


def twin(name):
    return name.replace("_bf16", "_f16")


@pytest.fixture(scope="module")
def built():
    from diffuvolume_amd import _build
    return _build.build()


def test_header_declares_exactly_the_sixth_table():
    from diffuvolume_amd import _lib
    decl = declarations(HEADER)
    assert set(decl) == set(_lib.AMP2D_BF16_SIGNATURES) == ENTRIES
    text = HEADER.read_text()
    for name, (res, args, _) in _lib.AMP2D_BF16_SIGNATURES.items():
        assert len(args) == decl[name], name
        assert (res, args) == _lib.SIGNATURES[twin(name)], name                  # the signature of the fp16 twin
        if res is ctypes.c_int:                                   # a launching entry: stream last, int return code
            assert args[-1] is _lib.P and re.search(rf"\bint\s+{name}\s*\([^)]*dv_stream_t\s+stream\s*\)", text), name
    assert "may be flushed to zero" in text and "v_cvt_pk_bf16_f32" in text
    assert "update.py:26-142" in text and "train_stereo.py:146-173" in text
    # the two entries that serve both element types have no twins, and say so where they are declared
    main = (INCLUDE / "diffuvolume_hip.h").read_text()
    assert "serve BOTH 16-bit element types" in main[:main.index("size_t dv_conv2d_f16_packed_bytes(")][-1200:]
    assert not [n for n in _lib.AMP2D_BF16_SIGNATURES if "packed_bytes" in n or "kslices" in n]


def test_the_sixth_table_is_disjoint_from_the_other_five():
    from diffuvolume_amd import _lib
    sixth = set(_lib.AMP2D_BF16_SIGNATURES)
    others = (set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VOLUME_TRAIN_SIGNATURES)
              | set(_lib.AMP3D_SIGNATURES) | set(_lib.AMP3D_BF16_SIGNATURES))
    assert not sixth & others
    for other in ("diffuvolume_hip.h", "diffuvolume_hip_train.h", "diffuvolume_hip_volume_train.h",
                  "diffuvolume_hip_amp3d.h", "diffuvolume_hip_amp3d_bf16.h"):
        assert not sixth & set(declarations(INCLUDE / other)), other
    assert not set(declarations(HEADER)) & others


def test_every_entry_names_its_decision_and_the_named_tests_exist():
    from diffuvolume_amd import _lib
    here = Path(__file__).resolve().parent
    kinds = {"size": 0, "packs": 0, "held": 0}
    for name, (res, _, why) in _lib.AMP2D_BF16_SIGNATURES.items():
        assert isinstance(why, str) and len(why) > 20, name
        if why == _lib.SIZE_ONLY:
            assert res is ctypes.c_size_t, name
            kinds["size"] += 1
            continue
        if why == _lib.PACKS_WEIGHTS:
            assert "_pack_weights" in name, name
            kinds["packs"] += 1
            continue
        assert why == _lib.held_by(why.split("held by: ")[1]), name
        fname, test = why.split("held by: ")[1].split("::")
        text = (here / fname).read_text()
        assert f"def {test}(" in text and name in text, (name, why)
        assert "pytest.mark.gpu" in text and "import arena" in text and "import streams" in text, fname
        kinds["held"] += 1
    assert kinds == {"size": 1, "packs": 1, "held": 8}


def test_no_hook_no_switch():
    from diffuvolume_amd import _env, _lib
    for name in _lib.AMP2D_BF16_SIGNATURES:
        assert "_set_" not in name, name
    assert not [k for k in _env.KNOBS if "BF16" in k]
    csrc = ROOT / "diffuvolume_amd" / "csrc"
    for f in ("conv2d_bf16.hip", "conv2d_wgrad_cat_bf16.hip", "gru_gates_bf16.hip", "conv2d_mp.h", "conv2d_wgrad_cat_mp.h",
              "gru_gates.h"):
        assert "getenv" not in (csrc / f).read_text(), f


def test_library_exports_and_load_types_the_sixth_table(built):
    from diffuvolume_amd import _lib
    raw = ctypes.CDLL(str(built))
    for name in _lib.AMP2D_BF16_SIGNATURES:
        assert hasattr(raw, name), f"{name} declared in the header but not exported"
    lib = _lib.load()
    for name, (res, args, _) in _lib.AMP2D_BF16_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and len(fn.argtypes) == len(args), name


def test_refusals_before_the_device_is_touched(built):
    from diffuvolume_amd import _lib
    lib = _lib.load()
    fake = 256                                                                 # never dereferenced: rejected first
    one, five = (ctypes.c_int * 1)(64), (ctypes.c_int * 5)(8, 8, 8, 8, 8)
    p1, p5 = (ctypes.c_void_p * 1)(fake), (ctypes.c_void_p * 5)(*[fake] * 5)
    # NULL -> -1
    assert lib.dv_conv2d_bf16_pack_weights(None, fake, 64, 64, 3, None) == -1
    assert lib.dv_conv2d_bf16_cat(p1, one, 1, None, 0, 0, 0, 0, 0, fake, 1, 4, 4, 8, 3, 0, None) == -1
    assert lib.dv_conv2d_bf16_cat_ksplit(p1, one, 1, fake, 0, 0, 0, 0, 0, None, fake, 2, 1, 4, 4, 8, 3, 0, None) == -1
    assert lib.dv_conv2d_bf16_cat_pair(p1, one, 1, fake, 0, 0, 0, fake, 0, 0, None, 1, 4, 4, 8, 8, 0, None) == -1
    assert lib.dv_conv2d_bf16_cat_pair_ksplit(None, one, 1, fake, 0, 0, 0, fake, 0, 0, fake, fake, 2, 1, 4, 4, 8, 8, 0, None) == -1
    assert lib.dv_conv2d_1in_bf16(fake, None, 0, fake, 1, 4, 4, 8, 3, 0, None) == -1
    assert lib.dv_gru_reset_mul_bf16(fake, fake, None, 16, None) == -1
    assert lib.dv_gru_blend_bf16(fake, None, fake, fake, 16, None) == -1
    assert lib.dv_conv2d_wgrad_cat_bf16(p1, one, 1, fake, fake, None, 1, 4, 32, 64, 3, None) == -1
    # k = 5 -> -3
    assert lib.dv_conv2d_bf16_pack_weights(fake, fake, 64, 64, 5, None) == -3
    assert lib.dv_conv2d_bf16_cat(p1, one, 1, fake, 0, 0, 0, 0, 0, fake, 1, 4, 4, 8, 5, 0, None) == -3
    assert lib.dv_conv2d_bf16_cat_ksplit(p1, one, 1, fake, 0, 0, 0, 0, 0, fake, fake, 2, 1, 4, 4, 8, 5, 0, None) == -3
    assert lib.dv_conv2d_wgrad_cat_bf16(p1, one, 1, fake, fake, fake, 1, 4, 32, 64, 5, None) == -3
    # five sources -> -2 from the weight gradient (a shape); the forward entries answer as their fp16 twins do
    assert lib.dv_conv2d_wgrad_cat_bf16(p5, five, 5, fake, fake, fake, 1, 4, 32, 64, 3, None) == -2
    a = (p5, five, 5, fake, 0, 0, 0, 0, 0, fake, 1, 4, 4, 8, 3, 0, None)
    assert lib.dv_conv2d_bf16_cat(*a) == lib.dv_conv2d_f16_cat(*a) != 0
    # n = 0 -> -2
    assert lib.dv_gru_blend_bf16(fake, fake, fake, fake, 0, None) == -2
    assert lib.dv_gru_reset_mul_bf16(fake, fake, fake, 0, None) == -2
    # every refusal of the fp16 twins on the same arguments
    for name, args in [("dv_conv2d_bf16_cat_pair", (p1, one, 1, fake, 0, 0, 0, fake, 0, 0, fake, 1, 4, 4, 8, 0, 0, None)),
                       ("dv_conv2d_bf16_cat_pair_ksplit", (p1, one, 1, fake, 0, 0, 0, fake, 0, 0, fake, None, 2, 1, 4, 4, 8, 8, 0, None)),
                       ("dv_conv2d_1in_bf16", (fake, fake, 0, fake, 1, 4, 4, 8, 4, 0, None)),
                       ("dv_conv2d_bf16_cat", (p1, one, 1, fake, 0, 0, 0, 0, 0, fake, 0, 4, 4, 8, 3, 0, None))]:
        rc = getattr(lib, name)(*args)
        assert rc < 0 and rc == getattr(lib, twin(name))(*args), name


def test_the_size_entry_shares_the_fp16_plan(built):
    """The shapes of tests/test_update_amp_host.py plus one four-source case."""
    from diffuvolume_amd import _lib
    lib = _lib.load()
    one, four, five = (ctypes.c_int * 1)(64), (ctypes.c_int * 4)(128, 128, 128, 128), (ctypes.c_int * 5)(8, 8, 8, 8, 8)
    mixed = (ctypes.c_int * 4)(7, 64, 1, 30)
    cases = [(one, 1, 1, 4, 32, 64, 3), (one, 1, 1, 4, 32, 64, 5), (five, 5, 1, 4, 32, 64, 3), (one, 1, 0, 4, 32, 64, 3),
             (four, 4, 4, 80, 184, 128, 3), (mixed, 4, 2, 9, 33, 65, 3), (mixed, 4, 2, 9, 33, 65, 1)]
    for args in cases:
        assert lib.dv_conv2d_wgrad_cat_bf16_workspace_floats(*args) == lib.dv_conv2d_wgrad_cat_f16_workspace_floats(*args), args[1:]
    assert lib.dv_conv2d_wgrad_cat_bf16_workspace_floats(one, 1, 1, 4, 32, 64, 3) == 64 * 64 * 9
    assert lib.dv_conv2d_wgrad_cat_bf16_workspace_floats(five, 5, 1, 4, 32, 64, 3) == 0
    assert lib.dv_conv2d_wgrad_cat_bf16_workspace_floats(mixed, 4, 2, 9, 33, 65, 3) > 0


# ------------------------------------------------------------------ the train-precision switch
def make_block():
    from diffuvolume_amd.synth import UPDATE_TRAIN_ARGS, UPDATE_TRAIN_HIDDEN
    from diffuvolume_amd.update import BasicMultiUpdateBlock
    block = BasicMultiUpdateBlock(types.SimpleNamespace(**UPDATE_TRAIN_ARGS), hidden_dims=UPDATE_TRAIN_HIDDEN)
    return block, (block, block.encoder, block.gru04, block.gru08, block.gru16, block.disp_head)


def test_set_train_precision_spelling_matrix_on_the_block_and_all_children():
    block, parts = make_block()
    assert all(m.train_precision == "f32" for m in parts)
    for given, reads in (("f16", "f16"), ("f32", "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16"),
                         (torch.float32, "f32"), (torch.bfloat16, "bf16")):
        assert block.set_train_precision(given) is block
        assert all(m.train_precision == reads for m in parts), given
    for bad in ("bf16", "fp16", None, 16, torch.float64, torch.int8, "bfloat16", True, ""):
        with pytest.raises(ValueError):
            block.set_train_precision(bad)
        assert all(m.train_precision == "bf16" for m in parts), bad        # a refused value changes nothing
    for child in parts[1:]:                                                 # every child is an entry of its own
        child.set_train_precision(torch.float32)
        assert child.train_precision == "f32" and block.train_precision == "bf16"
        child.set_train_precision(torch.bfloat16)
        with pytest.raises(ValueError):
            child.set_train_precision("bf16")
        assert child.train_precision == "bf16"
    assert not [k for k in block.state_dict() if "precision" in k]
    assert block.set_train_precision("f32").train_precision == "f32"


def test_the_bf16_plans_have_a_slot_of_their_own():
    from diffuvolume_amd import update
    assert update._TRAIN_SLOTS == {"f32": "train", "f16": "train16", "bf16": "trainbf16"}
    assert update._SLOT_ARGS["trainbf16"] == {"elem": "bf16"} and update._SLOT_ARGS["train16"] == {"f16": True}


def test_the_element_type_is_carried_beside_the_f16_flag():
    from diffuvolume_amd import train2d
    assert train2d._elem() is None and train2d._elem(True) == "f16" and train2d._elem(False, "bf16") == "bf16"
    assert train2d._elem(True, "f16") == "f16"
    for bad in ((True, "bf16"), (False, "f32"), (False, "fp16")):
        with pytest.raises(ValueError):
            train2d._elem(*bad)
    for fn in (train2d.conv2d_cat_weight_grad, train2d.conv_1in_relu, train2d.conv_cat, train2d.conv_gru,
               train2d._InputGradPlan.__init__, train2d.TrainConvPlan.__init__, train2d.GRUTrainPlan.__init__,
               train2d.Conv1InFn.forward):
        p = inspect.signature(fn).parameters
        assert p["f16"].default is False and p["elem"].default is None, fn
    assert list(inspect.signature(train2d.TrainConvPlan.__init__).parameters)[:4] == ["self", "conv", "act", "f16"]
    assert list(inspect.signature(train2d.conv2d_cat_weight_grad).parameters)[:4] == ["sources", "g", "k", "f16"]


def test_forward_train_amp_is_keyword_only_and_defaults_to_false():
    from diffuvolume_amd.igev_stereo_ddim import IGEVStereo_ddim
    p = inspect.signature(IGEVStereo_ddim.forward_train).parameters["amp"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert "torch.bfloat16" in IGEVStereo_ddim.forward_train.__doc__


def test_documents():
    integration = (ROOT / "INTEGRATION.md").read_text()
    assert "forward_train(" in integration and "amp=torch.bfloat16" in integration
    assert "its update block still refuses bf16 autocast" not in integration and "hourglass(8)" in integration
    design = (ROOT / "DESIGN.md").read_text()
    assert "conv2d_wgrad_cat_mp.h" in design and "conv2d_mp.h" in design and PARENT in design
    readme = (ROOT / "README.md").read_text()
    assert "conv2d_bf16.hip" in readme and "update_train_amp_bf16_bench" in readme


# ------------------------------------------------------------------ the machine code
@pytest.fixture(scope="module", params=sorted(FILES))
def isa(request, tmp_path_factory):
    from diffuvolume_amd import _build
    out = tmp_path_factory.mktemp("isa") / f"{request.param}.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / f"{request.param}.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return request.param, FILES[request.param], out.read_text()


def figures(text):
    """kernel name -> (VGPRs, LDS bytes, scratch bytes) from the metadata of an assembly file."""
    out = {}
    for block in text.split("  - .agpr_count:")[1:]:
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", block).group(1))
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = (get("vgpr_count"), get("group_segment_fixed_size"),
                                                              get("private_segment_fixed_size"))
    return out


def keyed(name, figs):
    """The figures of a file keyed as the PARENT_* tables are."""
    out = {}
    for kernel, f in figs.items():
        if name.startswith("conv2d_wgrad_cat"):
            out[int(re.search(r"HwGeoILi(\d)E", kernel).group(1))] = f
        elif "ksplit_epilogue" in kernel:
            out["ksplit_epilogue"] = f
        elif "pack_" in kernel:
            out["pack"] = f
        else:
            m = re.search(r"kernelILi(\d)ELi(\d)E", kernel)
            out[(int(m.group(1)), int(m.group(2)))] = f
    return out


def test_each_file_runs_on_its_own_matrix_instruction_without_scratch(isa):
    name, elem, text = isa
    other = {"f16": "bf16", "bf16": "f16"}[elem]
    matrix = set(re.findall(r"\bv_mfma_\w+", text))
    assert matrix == {f"v_mfma_f32_16x16x32_{elem}"}, matrix          # its own instruction and no other (none of the twin's)
    assert f"v_mfma_f32_16x16x32_{other}" not in text
    assert ("v_cvt_pk_bf16_f32" in text) == (elem == "bf16")            # the hardware rounding, in the bf16 files only
    figs = keyed(name, figures(text))
    parent = PARENT_WGRAD_CAT_F16 if name.startswith("conv2d_wgrad_cat") else PARENT_CONV2D_F16
    assert set(figs) == set(parent), sorted(map(str, figs))
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)]
    assert len(spills) == len(parent) and all(v == 0 for v in spills)
    for key, (vgpr, lds, scratch) in figs.items():
        pv, pl, ps = parent[key]
        print(f"REGS {name} {key}: vgpr {vgpr} lds {lds} scratch {scratch} (parent fp16 {pv} {pl} {ps})")
        if ps == 0:
            assert scratch == 0, (name, key)                          # no scratch where the fp16 twin has none
        if elem == "f16":                                             # the fp16 files: no worse than the parent's build
            assert vgpr <= pv and lds <= pl and scratch <= ps, (name, key, (vgpr, lds, scratch), parent[key])
