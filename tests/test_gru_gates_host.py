"""Without a GPU: csrc/gru_gates.hip compiles for gfx950 without scratch.  The six gate entries share one kernel template
whose per-element arrays (`in`, `out`, `x`, `y`, `a`, `r`) are indexed by loop variables and handed to the functor by
pointer; they stay in registers only because every loop unrolls completely.  An array that does not shows up as a private
segment, which this test refuses (the gate kernels were held to the same figures when they were compiled with
csrc/conv2d_wgrad_cat.hip, tests/test_update_train_host.py)."""
import re
import subprocess

import pytest

from diffuvolume_amd import _build


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "gru_gates.s"
    flags = [f for f in _build.FLAGS if f != "-fPIC"]
    subprocess.run([_build._hipcc(), *flags, "--cuda-device-only", "-S", str(_build.CSRC / "gru_gates.hip"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out.read_text()


def test_gate_kernels_without_scratch(isa):
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\s*s_endpgm", isa, re.M | re.S)}
    assert len(bodies) == 12 and all("gru_map_kernel" in n for n in bodies), sorted(bodies)    # six functors x (float4, scalar)
    for name, body in bodies.items():
        assert "scratch_" not in body and "atomic" not in body, name
    assert ";;#ASMSTART" not in isa
    spills = [int(v) for v in re.findall(r"\.[sv]gpr_spill_count:\s+(\d+)", isa)]
    private = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert len(spills) == 24 and all(v == 0 for v in spills)
    assert len(private) == 12 and all(v == 0 for v in private)
