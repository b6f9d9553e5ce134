"""Every export of the C ABI has a decision about its stream: it is a row of the arena table (run behind a gate on a side
stream by tests/test_gpu_stream_contract.py), one of the weight packers or behind one of the autograd wrappers held there,
or it launches nothing.  A new export cannot arrive without falling into exactly one of the four groups."""
import re
from pathlib import Path

import test_gpu_stream_contract as SC
from diffuvolume_amd import _lib
from test_abi_arena_complete import EXCLUDED as ARENA_EXCLUDED, HOOK, SIZE_OR_CHOICE
from test_gpu_abi_arena import TABLE

INCLUDE = Path(__file__).resolve().parent.parent / "include"


def launches_nothing():
    """name -> reason, for the exports that take no stream: sizes, choices, the version, the error string and the hooks."""
    out = {n: r for n, r in ARENA_EXCLUDED.items() if r in (SIZE_OR_CHOICE, HOOK)}
    out.update({n: _lib.SIZE_ONLY for n, v in _lib.VOLUME_TRAIN_SIGNATURES.items() if v[2] == _lib.SIZE_ONLY})
    out["dv_upsample_softmax_regress_bwd_workspace_floats"] = _lib.SIZE_ONLY
    return out


def exports():
    return set(_lib.SIGNATURES) | set(_lib.TRAIN_SIGNATURES) | set(_lib.VOLUME_TRAIN_SIGNATURES)


def test_every_export_is_in_exactly_one_group():
    groups = {"a row of the arena table": {r.entry for r in TABLE},
              "the packer table": {p[1] for p in SC.PACKERS},
              "the wrapper table": {e for w in SC.WRAPPERS for e in w.entries},
              "launches nothing": set(launches_nothing())}
    names = exports()
    for what, members in groups.items():
        assert not members - names, f"{what} names no export: {sorted(members - names)}"
    where = {n: [what for what, members in groups.items() if n in members] for n in names}
    missing = sorted(n for n, w in where.items() if not w)
    twice = {n: w for n, w in where.items() if len(w) > 1}
    assert not missing, ("exports with no decision about their stream: add a row to tests/test_gpu_abi_arena.py, or a packer or "
                         f"a wrapper to tests/test_gpu_stream_contract.py: {missing}")
    assert not twice, f"exports in more than one group: {twice}"


def test_what_launches_nothing_takes_no_stream():
    """An exclusion is a size, a choice, the version, a string or a hook: every launching entry takes `stream` as its last
    argument, a pointer, and none of these ends in one; the only ones that return an int are the hooks, the `*_supported`
    and `*_kslices` choices and the version."""
    tables = {**_lib.SIGNATURES, **_lib.TRAIN_SIGNATURES, **{k: v[:2] for k, v in _lib.VOLUME_TRAIN_SIGNATURES.items()}}
    for name, reason in launches_nothing().items():
        assert isinstance(reason, str) and len(reason) > 20, name
        res, args = tables[name]
        assert res is not _lib.c_int or "_set_" in name or name.endswith(("_supported", "_kslices")) or name == "dv_version", name
        assert not args or args[-1] is not _lib.P, f"{name} is excluded as launching nothing and ends in a pointer (a stream?)"


def test_every_packer_is_in_the_packer_table():
    packers = {n for n in exports() if "_pack_weights" in n}
    assert packers == {p[1] for p in SC.PACKERS} and len(SC.PACKERS) == len(packers) == 13
    for sizer, packer, dims, wshape in SC.PACKERS:
        assert sizer in _lib.SIGNATURES and len(_lib.SIGNATURES[sizer][1]) == len(dims), sizer
        assert len(_lib.SIGNATURES[packer][1]) == 2 + len(dims) + 1, packer


def test_the_wrapper_table_covers_what_the_arena_leaves_to_other_tests():
    """The TRAINED(...) exclusions of the arena table, the regression tail's backward and every launching row of the third
    signature table."""
    must = {n for n, r in ARENA_EXCLUDED.items() if "training entry whose misaligned-view test already exists" in r}
    must.add("dv_upsample_softmax_regress_bwd_f32")
    must |= {n for n, v in _lib.VOLUME_TRAIN_SIGNATURES.items() if v[2] != _lib.SIZE_ONLY}
    assert must == {e for w in SC.WRAPPERS for e in w.entries}
    assert len({w.name for w in SC.WRAPPERS}) == len(SC.WRAPPERS)


def test_the_header_names_every_process_wide_hook():
    """The convention block of include/diffuvolume_hip.h says that nothing keeps global mutable state; the `dv_*_set_*`
    hooks are the exception and every one declared in a header is named there, next to the stream contract."""
    main = (INCLUDE / "diffuvolume_hip.h").read_text()
    block = main[:main.index("#ifndef")]
    declared = set()
    for h in INCLUDE.glob("*.h"):
        declared |= set(re.findall(r"^\s*int\s+(dv_\w+_set_\w+)\s*\(", h.read_text(), flags=re.M))
    assert declared, "no hook found: the pattern no longer matches the header"
    assert declared == {n for n in exports() if re.fullmatch(r"dv_\w+_set_\w+", n)}
    for name in sorted(declared):
        assert name in block, f"{name} is a process-wide hook the convention block does not name"
    assert "process-wide atomics" in block
    assert re.search(r"every launch and memset of an entry goes to `stream`, and no entry blocks the\s+\*?\s*host", block)
