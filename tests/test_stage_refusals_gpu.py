"""GPU test: every refusal of live 8 x 8 sessions of the four post-process stages returns the code and the exact text of
tests/golden/stage_refusals.json (see test_stage_refusals_host.py for where the recording comes from).  A refused call launches
nothing: the sessions still work afterwards."""
import json
import os

import numpy as np
import pytest

import stage_refusal_cases as src
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ACCEPTED = {"filter.enqueue.samples=0.with_counts", "filter.run.samples=0.with_counts"}  # the counts replace the sample count


def test_the_half_on_live_sessions_equals_the_recording(pt, gpu):
    want = json.load(open(os.path.join(GOLDEN, "stage_refusals.json")))
    cases = src.live_cases(pt)
    assert {entry for _, entry, _ in cases} >= src.LIVE_ENTRIES and len(src.LIVE_ENTRIES) == 24
    with src.live_sessions(pt) as env:
        got = src.play(pt, cases, env)
        # the sessions are as they were: none grew, the tone mapper still has no history
        e = np.zeros(1, np.float32)
        pt.check(pt.lib.pt_tonemap_exposure(env["tonemap"], e.ctypes.data_as(pt._fp)))
        assert e[0] == 1.0
    assert len(got) == len(cases)
    for cid, _, _ in cases:
        print(cid, got[cid])
        assert got[cid] == want[cid], cid
        assert (got[cid] == [0, ""]) == (cid in ACCEPTED), cid
