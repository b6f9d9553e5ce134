"""Static check of csrc/conv2d_f16.hip compiled for gfx950 (hipcc cross-compiles without a GPU): the convolution
kernels run on the fp16 matrix instruction (v_mfma_f32_16x16x32_f16) and no fp32 one, and none of them spills or uses
scratch memory."""
import re
import subprocess

import pytest

from diffuvolume_amd import _build


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "conv2d_f16.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / "conv2d_f16.hip"), "-o",
                    str(out)], check=True, capture_output=True, text=True)
    return out.read_text()


def kernels(text):
    """name -> body text of every kernel in the ISA file."""
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*s_endpgm", text, re.M | re.S):
        bodies[m.group(1)] = m.group(2)
    return bodies


def test_main_kernels_use_f16_mfma_only(isa):
    main = {n: b for n, b in kernels(isa).items() if "conv2d_f16_kernel" in n}
    assert len(main) == 4, sorted(main)                       # k in {1, 3} x N tiles in {1, 4}
    for name, body in main.items():
        assert "v_mfma_f32_16x16x32_f16" in body, name
        assert not re.search(r"v_mfma_f32_\w+_f32\b", body), name


def test_no_spills_no_scratch(isa):
    spills = [int(v) for v in re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert spills and all(v == 0 for v in spills)       # (SGPR spills go to VGPR lanes, not memory)
    assert private and all(v == 0 for v in private)
