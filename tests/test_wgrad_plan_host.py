"""Without a GPU: the split plans of the seven split-K weight gradients are what tests/golden/wgrad_workspace_plan.json
recorded.  The bits of a weight gradient depend on its split count (csrc/wgrad_splitk.h: dv_wgrad_splits and
dv_split_range), so the plan is pinned as a table: every row is one call of a `*_workspace_floats` entry and the value it
returned at the commit that wrote the table (tools/make_golden_wgrad_plan.py, which also explains when it is rewritten).

The second test keeps the table from passing vacuously.  `model()` below restates, in Python and per entry, the
quantities an entry hands to dv_wgrad_splits (or the reason it refuses), and `splits_of()` the clamp order, naming the
clamps that changed the count.  Every row must agree with the model, and every refusal (REFUSALS), kernel variant
(VARIANTS), channel count (CHANNELS, on either side), brick count and clamp that the second test names must have a row.

One branch the code has cannot have a row: the clamp to 65535 splits in `fewin` and `deconv2d_k4`.  Both ask for
ceil(1024 / blocks) <= 1024 splits, so that clamp never binds; the table instead holds, for both, a row that asks for the
full 1024 and gets them."""
import ctypes
import json

import pytest

from conftest import GOLDEN
from diffuvolume_amd import _build

FIXTURE = GOLDEN / "wgrad_workspace_plan.json"
MAX_WS = 12 << 20                       # floats: DV_WGRAD_MAX_WS_FLOATS
CHANNELS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 146, 512)
ENTRIES = {
    "conv3d": "dv_conv3d_wgrad_workspace_floats",                   # B, Cin, D, H, W, Cout, k, stride
    "conv2d": "dv_conv2d_wgrad_workspace_floats",                   # B, Cin, H, W, Cout, k, dilation
    "cat": "dv_conv2d_wgrad_cat_workspace_floats",                  # channels | None, n_inputs, B, H, W, Cout, k
    "cat_f16": "dv_conv2d_wgrad_cat_f16_workspace_floats",          # as cat
    "deconv3d_k4": "dv_deconv3d_k4s2_wgrad_workspace_floats",       # B, Ci, D, H, W, Co
    "deconv2d_k4": "dv_deconv2d_k4s2_wgrad_workspace_floats",       # B, Ci, H, W, Co
    "fewin": "dv_conv2d_fewin_wgrad_workspace_floats",              # B, Cin, H, W, Cout, k, stride
}


def cdiv(a, b):
    return -(-a // b)


def bricks(batch, dims, tile):
    n = batch
    for d, t in zip(dims, tile):
        n *= cdiv(d, t)
    return n


def model(entry, args):
    """-> ("refused", reason) or ("plan", dict(variant, cin, cout, want, per, nbricks, minb, clamp))."""
    def plan(variant, cin, cout, want, per, nbricks, minb, clamp):
        return "plan", dict(variant=variant, cin=cin, cout=cout, want=want, per=per, nbricks=nbricks, minb=minb, clamp=clamp)

    if entry == "conv3d":
        b, cin, d, h, w, cout, k, s = args
        if min(b, cin, d, h, w, cout) <= 0:
            return "refused", "shape"
        tile = {(3, 1): (2, 4, 16), (3, 2): (2, 2, 8), (1, 1): (2, 4, 16)}.get((k, s))
        if tile is None:
            return "refused", "k_stride"
        pad = (k - 1) // 2
        out = [(v + 2 * pad - k) // s + 1 for v in (d, h, w)]
        return plan(f"k{k}s{s}", cin, cout, cdiv(512, cdiv(cout, 32) * cdiv(cin, 32)), cout * cin * k ** 3,
                    bricks(b, out, tile), 1, False)
    if entry == "conv2d":
        b, cin, h, w, cout, k, dil = args
        if min(b, cin, h, w, cout) <= 0:
            return "refused", "shape"
        if k not in (1, 3):
            return "refused", "k"
        if not 1 <= dil <= 16:
            return "refused", "dilation"
        variant, tile = ("k1", (4, 32)) if k == 1 else ("k3d4", (4, 32)) if dil <= 4 else ("k3d16", (2, 32))
        return plan(variant, cin, cout, cdiv(512, cdiv(cout, 32) * cdiv(cin, 32)), cout * cin * k * k,
                    bricks(b, (h, w), tile), 1, False)
    if entry in ("cat", "cat_f16"):
        chans, n, b, h, w, cout, k = args
        if chans is None:
            return "refused", "channels_null"
        if not 1 <= n <= 4:
            return "refused", "n_inputs"
        if min(chans[:n]) <= 0:
            return "refused", "empty_source"
        cin = sum(chans[:n])
        if cin > 0x3fffffff:
            return "refused", "channel_sum"
        if k not in (1, 3):
            return "refused", "k"
        if min(b, h, w, cout) <= 0:
            return "refused", "shape"
        if h * w >= 1 << 30:
            return "refused", "plane"
        if cout * cin * k * k > MAX_WS:
            return "refused", "workspace"
        if entry == "cat_f16" and (cdiv(cout, 64) > 65535 or cdiv(cin, 64) > 65535):
            return "refused", "grid"                     # (cat does not refuse these: DESIGN.md, known differences)
        tile = (2, 32) if entry == "cat" else (4, 32)
        return plan(f"k{k}n{n}", cin, cout, 256 // (cdiv(cout, 64) * cdiv(cin, 64)), cout * cin * k * k,
                    bricks(b, (h, w), tile), 2, False)
    if entry == "deconv3d_k4":
        b, ci, d, h, w, co = args
        if min(b, ci, d, h, w, co) <= 0:
            return "refused", "shape"
        nm, nn = cdiv(ci, 16), cdiv(co, 16)
        mw = 3 if nm % 3 == 0 else 2 if nm >= 2 else 1
        nw = 2 if nn >= 2 else 1
        kw = 1 if mw * nw >= 4 else 4 // (mw * nw)
        waves = 4 * cdiv(nm, mw) * cdiv(nn, nw) * mw * nw * kw
        return plan(f"{mw}x{nw}x{kw}", ci, co, cdiv(2048, waves), ci * co * 64, bricks(b, (d, h, w), (2, 4, 8)), 1, False)
    if entry == "deconv2d_k4":
        b, ci, h, w, co = args
        if min(b, ci, h, w, co) <= 0:
            return "refused", "shape"
        if h * w >= 1 << 28:
            return "refused", "plane"
        if ci * co * 16 > MAX_WS:
            return "refused", "workspace"
        cob = co if co < 4 else 3 if cdiv(co, 3) * 3 < cdiv(co, 4) * 4 else 4
        nt = min(cdiv(ci, 16), 4)
        blocks = cdiv(co, cob) * cdiv(cdiv(ci, 16), nt)
        return plan(f"nt{nt}cob{cob}", ci, co, cdiv(1024, blocks), ci * co * 16, bricks(b, (h, w), (4, 16)), 2, True)
    if entry == "fewin":
        b, cin, h, w, cout, k, s = args
        if min(b, cin, h, w, cout) <= 0:
            return "refused", "shape"
        if cin > 4:
            return "refused", "cin"
        if k not in (3, 5, 7):
            return "refused", "k"
        if s not in (1, 2):
            return "refused", "stride"
        if h * w >= 1 << 28:
            return "refused", "plane"
        if b * h * w >= 1 << 40:
            return "refused", "batch_plane"
        if cout * cin * k * k > MAX_WS:
            return "refused", "workspace"
        if cdiv(cout, 16) > 65535:
            return "refused", "grid"
        out = ((h - 1) // s + 1, (w - 1) // s + 1)
        return plan(f"k{k}s{s}", cin, cout, cdiv(1024, cdiv(cout, 16)), cout * cin * k * k, bricks(b, out, (8, 16)), 2, True)
    raise KeyError(entry)


def splits_of(want, per, nbricks, minb, clamp, **_):
    """dv_wgrad_splits, and the names of the clamps that changed the count ("want" when none did)."""
    s, hits = want, []
    if s > MAX_WS // per:
        s = MAX_WS // per
        hits.append("workspace")
    if s > nbricks // minb:
        s = nbricks // minb
        hits.append("bricks" if minb == 1 else "half_bricks")
    if clamp and s > 65535:
        s = 65535
        hits.append("grid")
    if s < 1:
        s = 1
        hits.append("one")
    return s, hits or ["want"]


# every refusal an entry's size query can give
REFUSALS = {
    "conv3d": {"shape", "k_stride"},
    "conv2d": {"shape", "k", "dilation"},
    "cat": {"channels_null", "n_inputs", "empty_source", "channel_sum", "k", "shape", "plane", "workspace"},
    "cat_f16": {"channels_null", "n_inputs", "empty_source", "channel_sum", "k", "shape", "plane", "workspace", "grid"},
    "deconv3d_k4": {"shape"},
    "deconv2d_k4": {"shape", "plane", "workspace"},
    "fewin": {"shape", "cin", "k", "stride", "plane", "batch_plane", "workspace", "grid"},
}
VARIANTS = {
    "conv3d": {"k3s1", "k3s2", "k1s1"},
    "conv2d": {"k1", "k3d4", "k3d16"},
    "cat": {f"k{k}n{n}" for k in (1, 3) for n in (1, 2, 3, 4)},
    "cat_f16": {f"k{k}n{n}" for k in (1, 3) for n in (1, 2, 3, 4)},
    "deconv3d_k4": {"3x2x1", "3x1x1", "2x2x1", "2x1x2", "1x2x2", "1x1x4"},
    "fewin": {f"k{k}s{s}" for k in (3, 5, 7) for s in (1, 2)},
}


def call(lib, entry, args):
    fn = getattr(lib, ENTRIES[entry])
    if entry in ("cat", "cat_f16"):
        chans = None if args[0] is None else (ctypes.c_int * len(args[0]))(*args[0])
        return fn(chans, *args[1:])
    return fn(*args)


@pytest.fixture(scope="module")
def rows():
    return json.loads(FIXTURE.read_text())["rows"]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    from diffuvolume_amd import _lib
    return _lib.load()


def test_every_row_returns_the_recorded_value(lib, rows):
    assert 200 <= len(rows) <= 1000
    wrong = [(r["entry"], r["args"], r["floats"], got) for r in rows for got in [call(lib, r["entry"], r["args"])]
             if got != r["floats"]]
    assert not wrong, wrong[:10]


def test_the_table_holds_every_branch(rows):
    seen = {e: dict(refusals=set(), variants=set(), cin=set(), cout=set(), by=set(), nbricks=set(), want=set())
            for e in ENTRIES}
    for r in rows:
        kind, m = model(r["entry"], r["args"])
        s = seen[r["entry"]]
        if kind == "refused":
            assert r["floats"] == 0, r
            s["refusals"].add(m)
            continue
        splits, by = splits_of(**m)
        assert r["floats"] == splits * m["per"], (r, m)              # the model is the table's, row by row
        s["variants"].add(m["variant"])
        s["cin"].add(m["cin"])
        s["cout"].add(m["cout"])
        s["by"].update(by)
        s["nbricks"].add(m["nbricks"])
        if by == ["want"]:
            s["want"].add(m["want"])
    for e, s in seen.items():
        assert s["refusals"] == REFUSALS[e], (e, s["refusals"] ^ REFUSALS[e])
        assert s["variants"] >= VARIANTS.get(e, set()), (e, VARIANTS[e] - s["variants"])
        assert s["cout"] >= set(CHANNELS), (e, set(CHANNELS) - s["cout"])
        # `fewin` takes at most 4 input channels; the sums of the cat entries' sources pass through every count as well
        assert s["cin"] >= (set(CHANNELS) if e != "fewin" else {1, 2, 3, 4}), (e, set(CHANNELS) - s["cin"])
        assert {1, 2} <= s["nbricks"], (e, "one brick, two bricks")
        assert {"want", "one"} <= s["by"], (e, s["by"])
        assert ("bricks" if e in ("conv3d", "conv2d", "deconv3d_k4") else "half_bricks") in s["by"], (e, s["by"])
    # the workspace cap binds where a plan can reach it.  The cat entries refuse a split that does not fit, and their
    # 256 / blocks splits of at most 64 x 64 x 9 floats per block stay below the bound; so do the small tiles of `fewin`
    # and `deconv2d_k4` against their targets.  (conv2d reaches it only with a split that does not fit: 0 splits, then one.)
    for e in ("conv3d", "conv2d", "deconv3d_k4"):
        assert "workspace" in seen[e]["by"], e
    # the 65535 clamp cannot bind (docstring): the largest request there is, 1024 splits, is in the table and is granted
    for e in ("fewin", "deconv2d_k4"):
        assert "grid" not in seen[e]["by"] and 1024 in seen[e]["want"], e
