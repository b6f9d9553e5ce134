"""Every inference plan and every reference-named operation takes the route, and produces the bits, recorded in
tests/golden/plan_dispatch.json (tools/make_golden_plan_dispatch.py: the cases, their shapes and what is recorded).

Per case three things are compared with the fixture: the kernel timer's records (tag, flops, bytes, issued, valu) with the
names of the entries launched, the SHA-256 of every output, and the SHA-256 of every tensor the plan holds (packed weight
images, folded scale / shift).  The fixture was recorded twice before the plans' plumbing was rewritten and the two
recordings agreed in every case, so every case is compared by its digests.
"""
import importlib.util
import json
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
_spec = importlib.util.spec_from_file_location("make_golden_plan_dispatch", ROOT / "tools" / "make_golden_plan_dispatch.py")
T = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(T)

GOLDEN = json.loads(T.GOLDEN.read_text())["cases"]


def test_fixture_covers_every_branch():
    """One case at least per branch, and the recording of a case shows the entry and the tag of each branch it names: a
    shape that drifts to another route is caught here by name, not only by a digest."""
    assert sorted(GOLDEN) == sorted(T.CASES)
    covered = set()
    for name, rec in GOLDEN.items():
        assert rec["branches"] == list(T.CASES[name][0]), name
        for branch in rec["branches"]:
            assert T.took(rec, branch), (name, branch, rec["entries"], [row[0] for row in rec["timed"]])
            covered.add(branch)
    assert covered == set(T.BRANCHES), set(T.BRANCHES) - covered


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_case_replays(name):
    got, want = T.run_case(name), GOLDEN[name]
    assert got["entries"] == want["entries"]
    assert got["timed"] == want["timed"]
    assert got["images"] == want["images"]
    assert got["outputs"] == want["outputs"]
