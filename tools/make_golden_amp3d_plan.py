"""The split-plan table of dv_conv3d_wgrad_f16_f32 (tests/golden/conv3d_wgrad_f16_plan.json): one row per call of
dv_conv3d_wgrad_f16_workspace_floats -- {"args": [B, Cin, D, H, W, Cout], "floats"} -- with the value the built library
returns.

tests/test_amp3d_host.py holds every later commit to this table, because the bits of a weight gradient depend on its
split count.  So the table is REGENERATED ONLY AT A COMMIT THAT INTENDS TO CHANGE THE PLAN (a new target, brick or clamp),
and that commit says so.  Before it writes, the script checks each value against the Python model of that test.

The sweep: the real layers at the benchmark's and the fixtures' planes, channel counts on both sides of the 32-channel
block edge, one and two bricks, a ragged range, the workspace cap and every refusal.

    python tools/make_golden_amp3d_plan.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import test_amp3d_host as T                          # noqa: E402
from diffuvolume_amd import _build                   # noqa: E402


def sweep():
    rows = []
    # the layers of the ACV and PCW stacks at batch 4, 256 x 512, and at the train-step fixtures' planes
    for b, d, h, w in ((4, 48, 64, 128), (1, 48, 16, 32), (2, 12, 8, 16)):
        rows += [[b, 32, d, h, w, 32], [b, 40, d, h, w, 32], [b, 64, d, h, w, 32]]
    rows += [[4, 64, 24, 32, 64, 64], [4, 128, 12, 16, 32, 128], [2, 64, 6, 8, 16, 64], [2, 128, 3, 4, 8, 128],
             [4, 8, 48, 64, 128, 8]]                                       # the full 512 splits
    # both sides of the block edge, either operand
    rows += [[2, c, 4, 6, 40, 32] for c in (1, 5, 31, 32, 33, 64, 65)] + [[2, 32, 4, 6, 40, c] for c in (1, 5, 31, 32, 33, 64, 65)]
    # one brick, two bricks (each axis and the batch), a ragged range, the workspace cap, one split that still fits
    rows += [[1, 8, 2, 2, 32, 8], [1, 8, 2, 2, 33, 8], [1, 8, 3, 2, 32, 8], [1, 8, 2, 3, 32, 8], [2, 8, 2, 2, 32, 8],
             [1, 8, 1, 1, 1, 8], [3, 128, 4, 6, 33, 128], [4, 160, 8, 8, 64, 160], [2, 682, 4, 4, 32, 682], [2, 683, 4, 4, 32, 683]]
    # refusals
    base = [2, 32, 4, 6, 40, 32]
    rows += [base[:i] + [v] + base[i + 1:] for i in range(6) for v in (0, -1)]
    rows += [[1, 8, 1 << 10, 1 << 10, 1 << 10, 8], [1, 1024, 2, 2, 8, 1024]]
    return rows


def main():
    _build.build()
    from diffuvolume_amd import _lib
    lib = _lib.load()
    out = []
    for args in sweep():
        floats = int(lib.dv_conv3d_wgrad_f16_workspace_floats(*args))
        assert floats == T.model_floats(*args), (args, floats, T.model_floats(*args))
        out.append({"args": args, "floats": floats})
    T.FIXTURE.write_text("{\"rows\": [\n" + ",\n".join(json.dumps(r) for r in out) + "\n]}\n")
    print(f"{T.FIXTURE}: {len(out)} rows")


if __name__ == "__main__":
    main()
