"""Dispatch and launch geometry of the library against its recorded snapshot (tests/golden/dispatch_snapshot.json, written
by tests/golden/make_dispatch_golden.py): for every stage of the recorded EGCL layers, standalone CEMLPs and fused
embeddings, at a small size and at one past the phased-backward thresholds, the kernel csmpn_last_kernel names and the
launch line CSMPN_DEBUG=1 prints (family, mode, grid, threads, LDS bytes, variant, RT / MT / H, share / phased, mirror) -
verbatim, under the default environment and under each family switch (one child process per environment: the switches
are read once). A shape the recorded library refused must be refused with the same code and text."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_dispatch_golden", os.path.join(GOLD, "make_dispatch_golden.py"))
dispatch = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dispatch)


@pytest.fixture(scope="module")
def recorded():
    with open(dispatch.FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("variant", list(dispatch.VARIANTS))
def test_dispatch_and_launch_geometry_match_the_recorded_snapshot(pkg, recorded, variant):
    want = recorded[variant]
    assert sorted(want) == sorted(f"{name}@{size}" for name in dispatch.VARIANTS[variant][1] for size in dispatch.SIZES), \
        "the cases no longer match the fixture"
    got = dispatch.run_variant(variant)
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key]["kernels"] == want[key]["kernels"], (variant, key)
        assert got[key]["log"] == want[key]["log"], (variant, key)
