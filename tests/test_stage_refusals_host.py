"""CPU test: every refusal of the four post-process stages that comes before the device check returns the code and the exact
text of tests/golden/stage_refusals.json -- recorded on the library of the commit before the stages got their shared host
scaffold (csrc/pt_stage.h), so a refusal that the scaffold rewords, reorders or drops fails here."""
import json
import os

import stage_refusal_cases as src
from conftest import GOLDEN

PT_EINVAL = -1


def test_the_half_without_a_device_equals_the_recording(pt):
    want = json.load(open(os.path.join(GOLDEN, "stage_refusals.json")))
    cases = src.host_cases(pt)
    got = src.play(pt, cases)
    assert len(got) == len(cases)
    for cid, _, _ in cases:
        print(cid, got[cid])
        assert got[cid] == want[cid], cid
        assert got[cid][0] == PT_EINVAL and got[cid][1], cid


def test_the_list_reaches_every_entry_point_and_the_recording_holds_nothing_else(pt):
    host, live = src.host_cases(pt), src.live_cases(pt)
    assert {entry for _, entry, _ in host} >= src.HOST_ENTRIES and len(src.HOST_ENTRIES) == 32
    for stage in ("denoiser", "filter", "temporal", "tonemap"):
        assert sum(cid.startswith(stage + ".create") for cid, _, _ in host) >= 10, stage
    ids = [cid for cid, _, _ in host + live]
    assert len(ids) == len(set(ids))
    assert set(json.load(open(os.path.join(GOLDEN, "stage_refusals.json")))) == set(ids)
