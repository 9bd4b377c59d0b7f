"""CPU, gloo, the oracle as compute backend: every rank of every eager class of csmpn_hip.sharded calls the backend
stages and posts the collectives of torch.distributed in the order and with the sizes of the recorded fixture
(tests/golden/sharded_call_trace.json, section "cpu"; see tests/sharded_trace_helpers.py). The multi-rank RCCL path
cannot run on a one-GPU box: ranks that post mismatched collectives hang there, and this is the check that they do not."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharded_trace_helpers as T   # noqa: E402

CASES = [(case, world) for case, worlds in T.CPU_CASES.items() for world in worlds]


@pytest.fixture(scope="module")
def fixture():
    return T.load_fixture()["cpu"]


def test_fixture_holds_every_case(fixture):
    assert sorted(fixture) == sorted(f"{case}/w{world}" for case, world in CASES)
    for key, ranks in fixture.items():
        assert len(ranks) == int(key.rsplit("/w", 1)[1]) and all(ranks), key
        assert any(ev[0] == "edge_backward" for ev in ranks[0]), key
        if len(ranks) > 1:      # every rank posts the same collectives (the stage calls differ in their edge counts)
            posted = [[ev for ev in r if not ev[0].endswith("ward")] for r in ranks]
            assert all(p == posted[0] and p for p in posted), key


@pytest.mark.parametrize("case,world", CASES)
def test_call_trace_matches_fixture(fixture, case, world):
    want = fixture[f"{case}/w{world}"]
    got = [events for _, events in T.spawn(T.cpu_worker, world, case)]
    for rank in range(world):
        assert got[rank] == want[rank], (case, world, rank)
