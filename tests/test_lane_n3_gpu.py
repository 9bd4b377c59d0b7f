"""GPU: every Cl(3,0) lane kernel at 16 and 32 channels - cemlp_cm_fwd_kernel (cemlp_cm.hpp), cemlp_cmb_kernel (cemlp_cmb.hpp),
both cemlp_cmp_kernel instantiations (cemlp_cmp.hpp), the EGCL and MODE_PLAIN programs of cemlp_pq.hpp / k_pq_n3.hip - under
every switch that routes a launch to another of them, and each kernel's tile walk. Cases, groups, expected dispatch and tile
geometry: tests/lane_n3_helpers.py; their host-side checks: tests/test_lane_n3_cpu.py.

Each group of cases runs in one child process with CSMPN_DEBUG=1 CSMPN_QUIET=1 and the group's switches; the child runs the
HIP side and stores the tensors, the references are computed once per seed tag on the host. Every test asserts from the
`[csmpn] ...` lines of ITS case that each launch ran on the family lane_n3_helpers.EXPECTED states (derived from
csrc/dispatch.hip and csmpn_hip/ops.py, not read off a run) with the case's channels and rows, and from csmpn_last_kernel
behind each stage the instantiation (cemlp_cmb_kernel, cemlp_cmp_kernel<.., true|false>, cemlp_pq_fwd / bwd_kernel).

    group            environment                         16 channels                  32 channels
    default          -                                   cm forward, cmb backward     pq both ways, state saved
    recompute        CSMPN_SAVE_STATE=0                  as default                   pq forward, cmp <.., false>
    nopq             CSMPN_NO_PQ=1                       -                            cm forward, cmp <.., true>
    nopq-recompute   CSMPN_NO_PQ=1 CSMPN_SAVE_STATE=0    -                            cm forward without state, cmp <.., false>
    nocmbwd          CSMPN_NO_CM_BWD=1                   cm forward, general backward pq forward, general backward, no state regions
    nopq-nocmbwd     CSMPN_NO_PQ=1 CSMPN_NO_CM_BWD=1     -                            cm forward, general backward, no state regions
    det              CSMPN_DETERMINISTIC=1               as default, row-store forms  as default, row-store forms
    plain            -                                   -                            pq MODE_PLAIN 60 -> 32, 90 -> 32 -> 32, 32 -> 32
    plain-recompute  CSMPN_SAVE_STATE=0                  -                            pq forward, general backward

Small cases ((N, E) = (2, 1), (5, 3), (37, 101) rewired, (64, 258); 6 edge- and 3 node-attribute channels, attribute gradients
taken, aggr and the residual alternating) against the float64 oracle; walks - one sweep of the stage's grid + a whole tile + a
partial one - against the float64 twin; every walk case proves from its own log lines that rows > grid x rows per workgroup
iteration (pq 16, cm forward 64, cmb 128, cmp 32) with the grid at its cap for the launches its table says walk, and
rows <= that for the others. Group det: every case twice in the child, bit-identical.

Bound: general_helpers.check unchanged - max(1e-5, 4 x yardstick) per tensor, 10 x that per element; every yardstick is
asserted to be at most 1e-5 first (lane_n3_helpers.reference), so the bound is the floor.

test_sentinels: forward and backward through the C-ABI on a saved buffer of exactly csmpn_cemlp_saved_floats floats and a
workspace of exactly csmpn_cemlp_workspace_bytes bytes, each between two runs of sentinels with a NaN interior.

test_reference_comparison_can_fail: a stored HIP result mutated the way a walk bug would leave it must be rejected.
"""
import numpy as np
import pytest

import lane_n3_helpers as L
from lane_n3_helpers import CASES, SUITE

gpu = pytest.mark.gpu


def _tags(pred):
    return [t for t, c in CASES.items() if pred(c)]


def _result(tag):
    r = L.result(tag)
    print(tag, r["message"], *r["log"], sep="\n")
    assert r["ok"], r["message"]
    return r


@gpu
@pytest.mark.parametrize("tag", _tags(lambda c: c["kind"] in ("egcl", "cemlp")))
def test_lane_n3_against_float64(tag):
    """One case: the cap on its yardsticks, then y, d/dh (d/dx), both attribute gradients and every parameter gradient within
    the suite's bound of the float64 reference; the log of that very run shows each launch on its expected family and
    instantiation; a walk case walks exactly where its table says. Group det: two runs in the child, bit-identical."""
    c = CASES[tag]
    t64, t32 = L.reference(tag)
    r = _result(tag)
    for k in sorted(t64):
        print(f"  {k}: HIP err {L.relmax(r['got'][k].reshape(t64[k].shape), t64[k]):.2e}, yardstick {L.relmax(t32[k], t64[k]):.2e}")
    print(SUITE.compare(tag, r["got"], t64, t32))
    runs = L.launches(r)
    want = [""] + (["run 2"] if c["group"] == "det" else []) + (["labels"] if c["kind"] == "egcl" else [])
    assert [n for n, _, _ in runs] == want, r["log"]
    for note, ls, labels in runs:
        L.check_dispatch(tag, ls)
        L.check_walks(tag, ls, c["walks"])
        if note == "labels":
            L.check_labels(tag, labels)


@gpu
@pytest.mark.parametrize("tag", _tags(lambda c: c["kind"].startswith("guard_")))
def test_sentinels(tag):
    """Nothing is stored in front of or behind the saved buffer and the workspace, sized exactly as the sizing entry points
    say, and every result of forward and backward is finite although everything the kernels did not write themselves is NaN:
    with CSMPN_FLAG_SAVE_STATE and with flags 0; under CSMPN_NO_CM_BWD=1 the buffer has no state regions at all."""
    c = CASES[tag]
    r = _result(tag)
    got = r["got"]
    runs = L.launches(r)
    assert [n for n, _, _ in runs] == list(L.GUARD_VARIANTS), r["log"]
    sizes = {}
    for v, ls, labels in runs:
        as_group = L.guard_group(c["group"], v)
        L.check_dispatch(tag, ls, as_group)
        L.check_labels(tag, labels, as_group)
        intact = {k: bool(got[k]) for k in got if k.startswith(v + ".intact.")}
        finite = {k: bool(got[k]) for k in got if k.startswith(v + ".finite.")}
        assert len(intact) == (2 if c["kind"] == "guard_cemlp" else 4) and len(finite) >= 22, (sorted(intact), sorted(finite))
        assert all(intact.values()), (tag, [k for k, ok in intact.items() if not ok])
        assert all(finite.values()), (tag, [k for k, ok in finite.items() if not ok])
        sizes[v] = {k.split(".")[-1]: int(got[k]) for k in got if k.startswith(v + ".floats.")}
    # the state regions are there exactly where the table says a forward writes them: 3 tensors x 2 blocks x 32 channels x 8
    # blades on the rows rounded up to 16
    for name, floats in sizes["state"].items():
        rows = c["rows"] if c["kind"] == "guard_cemlp" else (c["E"] if name == "saved_e" else c["N"])
        extra = 3 * 2 * 32 * L.D * ((rows + 15) // 16 * 16) if L.saves_state(c["group"], 32) else 0
        assert floats - sizes["noflag"][name] == extra, (tag, name, floats, sizes["noflag"][name])


# ----------------------------------------------------------------------------------------------- the comparisons can fail
def _launch(r, stage):
    return next(l for l in L.launches(r)[0][1] if (l["mode"], l["bwd"]) == stage)


def _second_sweep_from_first(a, sweep):
    a = a.copy()
    a[sweep:] = a[:a.shape[0] - sweep]
    return a


def _zero_last_partial_tile(a):
    a = a.copy()
    a[(a.shape[0] - 1) // L.TILE * L.TILE:] = 0.0
    return a


def _zero_one_row(a):
    a = a.copy()
    a[a.shape[0] - 1] = 0.0
    return a


@gpu
@pytest.mark.parametrize("tag", ["n3-16-101@default", "walk-cm-16@default", "n3-32-258@default", "walk-pq-32@default",
                                 "n3-32-101@recompute", "walk-cmp-32@recompute"],
                         ids=["cm16-oracle", "cm16-twin", "pq-oracle", "pq-twin", "cmp-oracle", "cmp-twin"])
def test_reference_comparison_can_fail(tag):
    """Mutation guard on the tensors the case stored, sized by the case's own launches: the second sweep of y replaced by the
    first, the last partial tile of d/dh zeroed, one workgroup's share of a parameter gradient removed, one row of each
    attribute gradient zeroed. Each must be rejected by the comparison that passed."""
    c = CASES[tag]
    t64, t32 = L.reference(tag)
    r = L.result(tag)
    assert r["ok"], r["message"]
    SUITE.compare(tag, r["got"], t64, t32)
    f, b = _launch(r, L.NODE_F), _launch(r, L.NODE_B)
    held = f["grid"] * L.rows_per_iteration(f["family"], c["C"], 0)
    mutations = [("y", lambda a: _second_sweep_from_first(a, min(held, a.shape[0] // 2))),
                 ("gh", _zero_last_partial_tile),
                 ("g.node_model.layers.1.0.weight", lambda a: a * (1.0 - 1.0 / b["grid"])),
                 ("g.edge_model.layers.0.2.linear_left.bias", lambda a: a * (1.0 - 1.0 / _launch(r, L.EDGE_B)["grid"])),
                 ("g_edge_attr", _zero_one_row), ("g_node_attr", _zero_one_row)]
    for key, fn in mutations:
        bad = dict(r["got"])
        bad[key] = fn(r["got"][key])
        assert not np.array_equal(bad[key], r["got"][key]), key
        with pytest.raises(AssertionError):
            SUITE.compare(tag, bad, t64, t32)
