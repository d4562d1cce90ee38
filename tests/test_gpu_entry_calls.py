"""The Python warp entry points hand the C ABI what they handed it when tests/golden/entry_calls.json was recorded, and raise what they
raised: argument for argument, message for message (tests/entry_calls.py: the cases, the recording stub, how addresses are named).
No kernel of the library is launched."""
import json

import pytest

from bev_amd import _lib, warp
from tests import entry_calls
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def test_entry_points_pass_and_raise_what_was_recorded():
    import os
    with open(os.path.join(ROOT, "tests", "golden", "entry_calls.json")) as f:
        want = json.load(f)
    real = _lib.load()
    try:
        got = json.loads(json.dumps(entry_calls.record_all()))  # (tuples become lists, as in the fixture)
    finally:  # (record_all restores and clears too: the rest of the suite must see the real library whatever happened in it)
        _lib._lib = real
        warp._plans.clear()
        warp._class_tables.clear()
        warp._minv_cache.clear()
    assert _lib.load() is real
    assert list(got) == list(want), "the list of cases changed: %s" % sorted(set(got) ^ set(want))
    bad = ["%s%s" % (cid, entry_calls.first_difference(got[cid], want[cid])) for cid in want if got[cid] != want[cid]]
    assert not bad, "%d of %d cases differ from the recorded calls; the first: %s" % (len(bad), len(want), bad[0])
    # the steady-state call of a camera loop was recorded from the plan: no new plan, the same bound arguments as the call that made it
    for cid, steps in want.items():
        if cid.startswith("wp/twice_owned") or cid.startswith("wp/twice_callers"):
            assert steps[0]["plans"] == 1 and steps[1]["plans"] == 0 and steps[2] == steps[1], cid
            assert steps[1]["calls"] == [[steps[0]["plan"]["fn"], steps[0]["plan"]["args"] + ["stream"]]], cid
