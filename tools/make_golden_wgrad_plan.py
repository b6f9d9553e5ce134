"""The split-plan table of the seven split-K weight gradients (tests/golden/wgrad_workspace_plan.json): one row per call of
a `*_workspace_floats` entry -- {"entry", "args", "floats"} -- with the value the built library returns.

tests/test_wgrad_plan_host.py holds every later commit to this table, because the bits of a weight gradient depend on its
split count.  So the table is REGENERATED ONLY AT A COMMIT THAT INTENDS TO CHANGE PLANS (a new target, tile or clamp), and
that commit says so; a refactor of the plan code leaves the file alone and must still pass.

The sweep (the branches tests/test_wgrad_plan_host.py asks for): channel counts on both sides of every tile edge, one and
two bricks, the workspace cap, the brick caps, the full 1024 splits of `fewin` and `deconv2d_k4`, every kernel variant,
1 .. 4 sources of the cat entries, and every refusal.  Before it writes, the script checks each value against the Python
model of that test, so a row whose branch is not the intended one is noticed here.

    python tools/make_golden_wgrad_plan.py"""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import test_wgrad_plan_host as T                     # noqa: E402
from diffuvolume_amd import _build                   # noqa: E402

C = T.CHANNELS
BIG = 1 << 14                                        # BIG * BIG = 2^28 pixels


def both_sides(make, fixed=32):
    """make(cin, cout) for every channel count on either side"""
    return [make(c, fixed) for c in C] + [make(fixed, c) for c in C]


def zeroed(args, positions):
    """args with 0, then -1, in each of the positions: the refusals of an empty or negative extent"""
    return [args[:i] + [v] + args[i + 1:] for i in positions for v in (0, -1)]


def sweep():
    rows = []

    def add(entry, *arg_lists):
        rows.extend({"entry": entry, "args": list(a)} for a in arg_lists)

    # conv3d: B, Cin, D, H, W, Cout, k, stride
    add("conv3d", *both_sides(lambda ci, co: [2, ci, 8, 16, 32, co, 3, 1]))
    for k, s in ((3, 2), (1, 1)):
        add("conv3d", *([2, ci, 8, 16, 32, co, k, s] for ci, co in ((1, 33), (33, 1), (146, 64), (64, 146), (512, 512))))
    add("conv3d", [1, 16, 2, 4, 16, 16, 3, 1], [2, 16, 2, 4, 16, 16, 3, 1],       # one brick, two bricks
        [1, 16, 3, 3, 15, 16, 3, 2], [2, 16, 3, 3, 15, 16, 3, 2], [1, 16, 2, 4, 16, 16, 1, 1], [1, 16, 4, 8, 32, 16, 3, 1],
        [2, 32, 16, 32, 64, 32, 3, 1], [4, 33, 16, 32, 64, 33, 3, 1],             # the workspace cap
        [2, 1024, 4, 8, 16, 1024, 3, 1], [1, 1024, 2, 4, 16, 1024, 3, 2])         # a split that does not fit: one
    add("conv3d", *zeroed([2, 32, 8, 16, 32, 32, 3, 1], range(6)))
    add("conv3d", *([2, 32, 8, 16, 32, 32, k, s] for k, s in ((2, 1), (5, 1), (1, 2), (3, 3), (3, 0), (0, 1))))

    # conv2d: B, Cin, H, W, Cout, k, dilation
    add("conv2d", *both_sides(lambda ci, co: [2, ci, 24, 80, co, 3, 1]))
    for k, d in ((1, 1), (3, 2), (3, 4), (3, 5), (3, 16)):
        add("conv2d", *([2, ci, 24, 80, co, k, d] for ci, co in ((1, 33), (33, 1), (146, 64), (512, 512))))
    add("conv2d", [1, 16, 4, 32, 16, 3, 1], [2, 16, 4, 32, 16, 3, 1], [1, 16, 2, 32, 16, 3, 16], [2, 16, 2, 32, 16, 3, 16],
        [1, 16, 4, 32, 16, 1, 1], [1, 16, 9, 65, 16, 3, 1], [2, 1200, 24, 80, 1200, 3, 1], [2, 1200, 24, 80, 1200, 3, 8])
    add("conv2d", *zeroed([2, 32, 24, 80, 32, 3, 1], range(5)))
    add("conv2d", *([2, 32, 24, 80, 32, k, d] for k, d in ((2, 1), (5, 1), (0, 1), (3, 0), (3, 17), (3, -1), (1, 17))))

    # the cat entries: channels | None, n_inputs, B, H, W, Cout, k
    for e, ty in (("cat", 2), ("cat_f16", 4)):
        add(e, *([[c], 1, 2, 20, 70, 64, 3] for c in C), *([[64], 1, 2, 20, 70, c, 3] for c in C))
        for k in (1, 3):
            add(e, *([ch, len(ch), 2, 5, 37, 70, k] for ch in ([40], [40, 24], [40, 24, 3], [40, 24, 3, 5])))
            add(e, [[128, 128, 128], 3, 4, 80, 184, 128, k], [[512], 1, 2, 20, 70, 512, k], [[146, 146], 2, 2, 20, 70, 33, k])
        add(e, [[16], 1, 1, ty, 32, 16, 3], [[16], 1, 2, ty, 32, 16, 3], [[16], 1, 1, ty + 1, 33, 16, 3],   # 1, 2, 4 bricks
            [[16], 1, 1, 8, 64, 16, 1],
            [[1], 1, 1, 1, 1, 4194241, 1], [[4194241], 1, 1, 1, 1, 1, 1],          # grids beyond 65535: cat_f16 refuses
            [[4194240], 1, 1, 1, 1, 1, 1])
        add(e, [None, 1, 2, 20, 28, 128, 3], [[128], 0, 2, 20, 28, 128, 3], [[1, 1, 1, 1, 1], 5, 2, 20, 28, 128, 3],
            [[128, 0], 2, 2, 20, 28, 128, 3], [[-1], 1, 2, 20, 28, 128, 3], [[0x3fffffff, 1], 2, 1, 1, 1, 1, 1],
            [[128], 1, 2, 20, 28, 128, 2], [[128], 1, 2, 20, 28, 128, 5], [[1], 1, 1, 1 << 15, 1 << 15, 1, 1],
            [[512], 1, 2, 20, 28, 4096, 3], [[512], 1, 2, 20, 28, 24577, 1])
        add(e, *zeroed([[128], 1, 2, 20, 28, 128, 3], (2, 3, 4, 5)))

    # deconv3d_k4: B, Ci, D, H, W, Co
    add("deconv3d_k4", *both_sides(lambda ci, co: [2, ci, 4, 8, 16, co]))
    add("deconv3d_k4", *([2, ci, 4, 8, 16, co] for ci, co in ((48, 32), (48, 16), (32, 16), (16, 32), (16, 8), (146, 146))))
    add("deconv3d_k4", [1, 16, 2, 4, 8, 8], [2, 16, 2, 4, 8, 8], [1, 16, 3, 5, 9, 8], [2, 320, 4, 8, 16, 320],
        [2, 512, 4, 8, 16, 512], [1, 512, 2, 4, 8, 512])
    add("deconv3d_k4", *zeroed([2, 32, 4, 8, 16, 16], range(6)))

    # deconv2d_k4: B, Ci, H, W, Co
    add("deconv2d_k4", *both_sides(lambda ci, co: [2, ci, 16, 64, co]))
    add("deconv2d_k4", *([2, ci, 128, 512, co] for ci, co in ((16, 3), (64, 1), (64, 9), (32, 32), (65, 4), (146, 146))))
    add("deconv2d_k4", [1, 32, 4, 16, 32], [2, 32, 4, 16, 32], [1, 64, 5, 17, 9], [2, 512, 16, 64, 512],
        [1, 1, BIG, BIG, 1], [1, 1, BIG, BIG - 1, 1], [2, 1024, 16, 64, 1024], [2, 1024, 16, 64, 768])
    add("deconv2d_k4", *zeroed([2, 32, 16, 64, 32], range(5)))

    # fewin: B, Cin, H, W, Cout, k, stride
    add("fewin", *([2, 3, 32, 64, c, 3, 1] for c in C), *([2, ci, 32, 64, 32, 3, 2] for ci in (1, 2, 3, 4)))
    for k in (3, 5, 7):
        for s in (1, 2):
            add("fewin", [2, 3, 32, 64, 64, k, s], [2, 3, 256 * s, 512 * s, 16, k, s], [1, 4, 33, 65, 17, k, s])
    add("fewin", [1, 3, 8, 16, 32, 3, 1], [2, 3, 8, 16, 32, 3, 1], [1, 3, 16, 32, 32, 3, 2], [2, 3, 16, 32, 32, 7, 2],
        [1, 3, 9, 17, 32, 3, 1], [2, 4, 32, 64, 64198, 7, 2], [2, 1, 32, 64, 1048560, 3, 1])
    add("fewin", *zeroed([2, 3, 32, 64, 32, 3, 1], range(5)))
    add("fewin", [2, 5, 32, 64, 32, 3, 1], [2, 3, 32, 64, 32, 1, 1], [2, 3, 32, 64, 32, 4, 1], [2, 3, 32, 64, 32, 9, 1],
        [2, 3, 32, 64, 32, 3, 0], [2, 3, 32, 64, 32, 3, 3], [1, 1, BIG, BIG, 1, 3, 1], [4097, 1, BIG - 1, BIG - 1, 1, 3, 1],
        [2, 4, 32, 64, 64199, 7, 2], [2, 1, 32, 64, 1048561, 3, 1])
    return rows


def main():
    _build.build()
    from diffuvolume_amd import _lib
    lib = _lib.load()
    rows = sweep()
    for r in rows:
        r["floats"] = int(T.call(lib, r["entry"], r["args"]))
        kind, m = T.model(r["entry"], r["args"])
        want = 0 if kind == "refused" else T.splits_of(**m)[0] * m["per"]
        assert r["floats"] == want, (r, kind, m)
    T.test_the_table_holds_every_branch(rows)
    text = "{\"rows\": [\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]}\n"
    T.FIXTURE.write_text(text)
    print(f"{T.FIXTURE}: {len(rows)} rows")


if __name__ == "__main__":
    main()
