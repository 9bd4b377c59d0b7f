"""GPU: the three graphed classes of csmpn_hip.sharded post, in two run() calls, the collectives and waits of the
recorded fixture (tests/golden/sharded_call_trace.json, section "gpu"): two gloo ranks sharing cuda:0 and the
single-process case, which posts none. Stage kernels: those of tests/test_sharded_gpu.py (Cl(3,0), 8 channels)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sharded_trace_helpers as T   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case,world", [(case, world) for case, worlds in T.GPU_CASES.items() for world in worlds])
def test_graphed_collectives_match_fixture(case, world):
    want = T.load_fixture()["gpu"][f"{case}/w{world}"]
    got = [events for _, events in T.spawn(T.gpu_worker, world, case)]
    assert len(want) == world
    for rank in range(world):
        assert got[rank] == want[rank], (case, world, rank)
    assert (world == 1) == (not any(got)), "a single process posts no collective, two ranks do"
