"""The buffer-sizing contract of the library against its recorded snapshot (tests/golden/sizing_contract.npz, written by
tests/golden/make_sizing_golden.py): csmpn_cemlp_saved_floats (flags 0 and CSMPN_FLAG_SAVE_STATE),
csmpn_cemlp_saved_floats_per_row and csmpn_cemlp_workspace_bytes, for every swept shape and row count, under the default
environment and under each switch that enters the sizing. Host-only queries: no GPU. Callers allocate by these figures and
the kernels address by them, so every entry must be exactly what was recorded."""
import importlib.util
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_sizing_golden", os.path.join(GOLD, "make_sizing_golden.py"))
sizing = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sizing)


@pytest.fixture(scope="module")
def recorded():
    g = np.load(sizing.FIXTURE)
    assert np.array_equal(g["configs"], np.asarray(sizing.configs(), dtype=np.int32)), "the sweep no longer matches the fixture"
    assert tuple(g["rows"]) == sizing.ROWS
    return g


@pytest.mark.parametrize("env_name", list(sizing.ENVS))
def test_sizing_contract_matches_the_recorded_snapshot(pkg, recorded, tmp_path, env_name):
    got = sizing.measure_in_child(env_name, str(tmp_path / "sizes.npy"))
    want = recorded[env_name]
    assert got.shape == want.shape and got.dtype == want.dtype
    cols = ["per_row", "workspace_bytes"] + [f"saved(rows={r}, flags={f})" for r in sizing.ROWS for f in ("0", "SAVE_STATE")]
    bad = np.argwhere(got != want)
    first = [(tuple(int(v) for v in recorded["configs"][r]), cols[c], int(got[r, c]), int(want[r, c])) for r, c in bad[:8]]
    assert len(bad) == 0, f"{len(bad)} entries differ; (n, I0, C, blocks), query, got, recorded: {first}"
