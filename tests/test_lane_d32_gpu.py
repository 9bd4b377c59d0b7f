"""GPU: every D = 32 lane-kernel instantiation - pl (cemlp_pl.hpp), plw (cemlp_plw.hpp), pg (cemlp_pg.hpp); Cl(5,0) and
Cl(4,1) at 8 / 16 / 24 / 28 / 32 channels - under every switch that routes a launch to another of them, and each family's
tile walk where a workgroup takes a second row tile. Cases, groups, expected dispatch and tile geometry:
tests/lane_d32_helpers.py.

Each group of cases runs in one child process with CSMPN_DEBUG=1 CSMPN_QUIET=1 and the group's switches; the child runs
the HIP side and stores the tensors, the references are computed once per shape on the host, and every test asserts from
the `[csmpn] <family> mode=.. bwd=.. ..` lines of ITS case that each launch ran on the family the table
lane_d32_helpers.EXPECTED states (derived from the eligibility functions of csrc/dispatch.hip, not read off a run), with
the case's channels, attribute channels and rows, and that no general-kernel and no wide line appears.

    group      environment             families reached
    default    -                       pl (8), plw (16), pg (24 / 28 / 32), both directions; the merged csmpn_egcl_backward
    recompute  CSMPN_SAVE_STATE=0      pl without state; pg forward with plw backward at 24 / 28 / 32
    nopg       CSMPN_NO_PG=1           plw forward and backward at 24 / 28 / 32
    plw8       CSMPN_PLW8=1            plw at 8 channels
    det        CSMPN_DETERMINISTIC=1   row-store forms, atomic-free parameter sums, the separate node / edge backward entries
    plain      -                       the two MODE_PLAIN plw instantiations (2 -> 28 in one block, 3 -> 28 -> 28)

Matrix ((algebra, channels) pairs per group; small = N 37 / E 101 rewired and N 64 / E 258, aggr and the residual
alternating, attribute gradients taken, against the float64 oracle with the float32 oracle as yardstick):

    default    small: Cl(5,0) x 16, 32 and Cl(4,1) x 24, 28 (the pairs without a parity test before) at both shapes;
               Cl(5,0) x 28, Cl(4,1) x 8, 32 at E 101; walks Cl(5,0) x 8 (pl), 16 (plw), 24 and 32 (pg); partitions
               Cl(4,1) x 16 (plw), 28 (pg): all ten pairs
    recompute  small: all ten pairs at both shapes; walks Cl(5,0) x 24, 32 (plw backward); partitions Cl(4,1) x 32
    det        small: all ten pairs at both shapes, each run twice in the child and compared with torch-level bit equality;
               walk Cl(5,0) x 16 (plw)
    nopg       small: both algebras x 24, 28, 32 at both shapes; walk Cl(5,0) x 28 (plw forward past 2048 rows)
    plw8       small: both algebras x 8 at both shapes
    plain      both CEMLPs on both algebras at 1 and 23 rows, on Cl(5,0) at 2069 rows (walks both ways), against
               cpu_twin.cemlp

Walks on Cl(5,0): against the float64 twin with the float32 twin as yardstick; each shape is one sweep of the grid + a few
whole tiles + a partial tile, and every walk case proves its walk from its own log: rows > grid x tile_rows for the launches
the case table says walk, rows <= grid x tile_rows for the others (tile_rows: 16 pg, 4 plw, 16 pl).

Walks on Cl(4,1): the float32 twin is 3e-4 .. 7e-2 off the float64 twin on the attribute gradients at these sizes, so the
size-independent properties the suite uses for S3 stand in: the node stage's full launch against launches that partition
its rows, the edge stage (aggr = sum, no residual) against launches that partition the edge list, through ops.HipBackend;
the full launch walks, every part launch is a one-sweep launch by its log line. Bounds of
test_node_stage_row_partition_full_size / test_edge_stage_additivity_full_size: 1e-5 of max|tensor| on row tensors, the
aggregate and d/dh, 1e-4 on parameter gradients. The cut is N // 3 + 5 (E // 3); at 16 channels the second part (2733 rows)
would itself pass the 2048-row sweep of the plw backward, so that case has three parts.

Bounds: general_helpers.check unchanged - max(1e-5, slack x yardstick) per tensor, 10 x that per element, slack 4 on
Cl(5,0), 10 on Cl(4,1). Conditioning, asserted on the references before a HIP result is looked at: a small Cl(4,1) case
passes `well_conditioned` and every yardstick is at most 5e-5 (no bound above 5e-4; seed offsets: lane_d32_helpers.RESEED);
every yardstick of a Cl(5,0) or `plain` case is at most 1e-5, so its bound is the floor.

test_*_comparison_can_fail: a stored HIP result mutated the way a walk bug would leave it - the rows of the second sweep of
y replaced by rows of the first, the last partial tile of gh zeroed, one workgroup's share of a parameter gradient dropped -
must be rejected by each kind of comparison (oracle, twin, partition).
"""
import numpy as np
import pytest

import lane_d32_helpers as L
from lane_d32_helpers import CASES, SUITE

gpu = pytest.mark.gpu


def _tags(pred):
    return [t for t, c in CASES.items() if pred(c)]


# ----------------------------------------------------------------------------------------------- host: the tables
def test_every_tag_in_exactly_one_group():
    for tag, c in CASES.items():
        assert L.group_of(tag) == c["group"]    # group_of asserts that exactly one predicate holds
    assert sorted(t for g in L.GROUPS for t in L.group_tags(g)) == sorted(CASES)
    assert set(L.EXPECTED) == set(L.GROUPS) == set(L.GROUP_ENV)


def test_expected_dispatch_covers_every_case():
    for tag, c in CASES.items():
        channels = c["widths"][2] if c["kind"] == "cemlp" else c["C"]
        want = L.EXPECTED[c["group"]][channels]
        assert set(want) == (set(L.EGCL_STAGES) if c["kind"] != "cemlp" else {L.PLAIN_F, L.PLAIN_B}), tag
        assert set(c["walks"]) <= set(want), tag


def test_walk_shapes_exceed_the_stated_sweep():
    """Every launch a case says walks has more rows than one sweep of its expected family holds (lane_d32_helpers.sweep_rows),
    less than two sweeps of the launch it was sized for, and no multiple of the tile; every other launch fits one sweep; a
    partition case's parts all fit one sweep."""
    rows_per_sweep = {("pg", 24, 0): 4096, ("pg", 32, 1): 4096, ("plw", 16, 0): 4096, ("plw", 16, 1): 2048, ("plw", 24, 0): 2048,
                      ("plw", 28, 1): 1024, ("plw", 32, 0): 2048, ("plw", 8, 0): 8192, ("plw", 8, 1): 4096, ("pl", 8, 0): 8192,
                      ("pl", 8, 1): 4096}
    for key, rows in rows_per_sweep.items():    # the table of the issue
        assert L.sweep_rows(*key) == rows, key
    walking = _tags(lambda c: c["walks"])
    assert len(walking) == 8 + 2 + 6
    for tag in walking:
        c = CASES[tag]
        channels = c["widths"][2] if c["kind"] == "cemlp" else c["C"]
        want = L.EXPECTED[c["group"]][channels]
        if c["kind"].startswith("part_"):
            want = {s: f for s, f in want.items() if s[0] == (2 if c["kind"] == "part_node" else 1)}
        for stage, family in want.items():
            rows, sweep = L.stage_rows(tag)(stage), L.sweep_rows(family, channels, stage[1])
            assert (rows > sweep) == (stage in c["walks"]), (tag, stage, rows, sweep)
            if stage in c["walks"]:
                assert rows % L.TILE_ROWS[family] != 0, (tag, stage)
            if c["kind"].startswith("part_"):
                assert all(hi - lo <= sweep for lo, hi in L.part_bounds(tag)), (tag, stage, L.part_bounds(tag))
        sized_for = min(L.stage_rows(tag)(s) / L.sweep_rows(want[s], channels, s[1]) for s in c["walks"])
        assert 1.0 < sized_for < 1.03, (tag, sized_for)


def test_coverage_matrix():
    pairs = lambda group, kind="egcl": {(c["metric"], c["C"]) for c in CASES.values() if c["group"] == group and c["kind"] != "cemlp"
                                        and (kind is None or c["kind"] == kind)}
    ten = {(m, C) for m in L.ALGS.values() for C in L.CHANNELS}
    assert pairs("default", None) == ten
    assert pairs("recompute") == ten and pairs("det") == ten
    assert pairs("nopg") == {(m, C) for m in L.ALGS.values() for C in (24, 28, 32)}
    assert pairs("plw8") == {(m, 8) for m in L.ALGS.values()}
    # the small matrix: both shapes of every pair in recompute and det, aggr and the residual both ways per algebra
    for group in ("recompute", "det"):
        small = [c for c in CASES.values() if c["group"] == group and c["ref"] == "oracle"]
        assert len(small) == 20 and {(c["N"], c["E"]) for c in small} == {(37, 101), (64, 258)}
        for m in L.ALGS.values():
            assert {(c["aggr"], c["residual"]) for c in small if c["metric"] == m} == {(a, r) for a in ("mean", "sum") for r in (True, False)}
    plain = [c for c in CASES.values() if c["group"] == "plain"]
    assert sorted((L.G.ALG_NAMES[c["metric"]], c["nl"], c["widths"][0], c["rows"]) for c in plain) == sorted(
        [(a, nl, i, r) for a in ("cl50", "cl41") for nl, i in ((1, 2), (2, 3)) for r in (1, 23)] + [("cl50", 1, 2, 2069), ("cl50", 2, 3, 2069)])


def test_conditioning_runs_on_the_host():
    """The references and their conditioning assertions need no GPU: the reseeded Cl(4,1) case of the small matrix."""
    tag = "lane-cl41-24-101@recompute"
    t64, t32 = L.reference(tag)
    assert set(t64) == set(t32) and len(t64) == 44


# ------------------------------------------------------------------------------------------------------------ the GPU
@gpu
@pytest.mark.parametrize("tag", _tags(lambda c: c["kind"] in ("egcl", "cemlp")))
def test_lane_d32_against_float64(tag):
    """One case: conditioning of its inputs, then output, d/d input, d/d attributes and every parameter gradient within the
    suite's bound of the float64 reference; the log of that very run shows each launch on its expected family; a walk case
    walks exactly where its table says. Group det: two runs in the child, bit-identical."""
    c = CASES[tag]
    t64, t32 = L.reference(tag)
    r = L.result(tag)
    print(tag, r["message"], *r["log"], sep="\n")
    assert r["ok"], r["message"]
    print(SUITE.compare(tag, r["got"], t64, t32))
    runs = L.launches(r)
    assert [n for n, _ in runs] == (["", "run 2"] if c["group"] == "det" else [""]), r["log"]
    for _, ls in runs:
        L.check_dispatch(tag, ls, L.stage_rows(tag))
        L.check_walks(tag, ls, c["walks"])


# Row-local tensors of the node stage (out, d/dh, d/d agg, d/d node_attr: the same arithmetic on the same rows in the full
# launch and in a part): measured bit-identical on one MI355X in all three cases -> asserted so
NODE_ROWS_EXACT = ("row0", "row1", "row2", "row3")


@gpu
@pytest.mark.parametrize("tag", _tags(lambda c: c["kind"].startswith("part_")))
def test_lane_d32_cl41_partition(tag):
    """Cl(4,1) where the full launch of a stage walks: it equals its parts, each a one-sweep launch by its own log line.
    Measured on one MI355X: the node stage's row tensors are bit-identical between the full launch and the parts in all three
    cases (asserted); the edge stage's aggregate and scattered d/dh are sums over other sets of edges and differ by
    5.8e-8 .. 1.2e-7 of max|tensor|, the parameter gradients of both stages by 3.9e-8 .. 5.1e-7 (bounds 1e-5 / 1e-4)."""
    c = CASES[tag]
    r = L.result(tag)
    print(tag, r["message"], *r["log"], sep="\n")
    assert r["ok"], r["message"]
    runs = L.launches(r)
    bounds = L.part_bounds(tag)
    assert [n for n, _ in runs] == ["full"] + [f"p{k}" for k in range(c["parts"])], r["log"]
    L.check_dispatch(tag, runs[0][1], L.stage_rows(tag))
    L.check_walks(tag, runs[0][1], c["walks"])
    for (_, ls), (lo, hi) in zip(runs[1:], bounds):
        L.check_dispatch(tag, ls, lambda stage: hi - lo)
        L.check_walks(tag, ls, ())
    exact = NODE_ROWS_EXACT if c["kind"] == "part_node" else ()
    loose = L.compare_partition(tag, r["got"])
    print({k: f"{v:.2e}" for k, v in loose.items()})
    L.compare_partition(tag, r["got"], exact)


def _second_sweep_from_first(a, sweep):
    a = a.copy()
    a[sweep:] = a[:a.shape[0] - sweep]
    return a


def _zero_last_partial_tile(a, tile):
    a = a.copy()
    a[a.shape[0] // tile * tile:] = 0.0
    return a


def _launch(r, stage, note=""):
    ls = dict(L.launches(r))[note]
    return next(l for l in ls if (l["mode"], l["bwd"]) == stage)


def _walk_mutations(r, y_key, gh_key, g_key, fwd, bwd, note=""):
    """(tensor, mutation) the way a walk bug would leave a result, sized by the case's own launches."""
    f, b = _launch(r, fwd, note), _launch(r, bwd, note)
    return [(y_key, lambda a: _second_sweep_from_first(a, min(f["grid"] * L.TILE_ROWS[f["family"]], a.shape[0] // 2))),
            (gh_key, lambda a: _zero_last_partial_tile(a, L.TILE_ROWS[b["family"]])),
            (g_key, lambda a: a * (1.0 - 1.0 / b["grid"]))]


@gpu
@pytest.mark.parametrize("tag", ["lane-cl50-16-101@default", "walk-cl50-plw-16@default"], ids=["oracle", "twin"])
def test_reference_comparison_can_fail(tag):
    """Mutation guard (as test_egcl_golden_can_fail) on the tensors the case stored: each must be rejected."""
    t64, t32 = L.reference(tag)
    r = L.result(tag)
    assert r["ok"], r["message"]
    SUITE.compare(tag, r["got"], t64, t32)
    for key, fn in _walk_mutations(r, "y", "gh", "g.node_model.layers.1.0.weight", L.NODE_F, L.NODE_B):
        bad = dict(r["got"])
        bad[key] = fn(r["got"][key])
        assert not np.array_equal(bad[key], r["got"][key]), key
        with pytest.raises(AssertionError):
            SUITE.compare(tag, bad, t64, t32)


@gpu
def test_partition_comparison_can_fail():
    tag = "part-node-cl41-28@default"
    r = L.result(tag)
    assert r["ok"], r["message"]
    L.compare_partition(tag, r["got"], NODE_ROWS_EXACT)
    for key, fn in _walk_mutations(r, "full.row0", "full.row1", "full.g0", L.NODE_F, L.NODE_B, note="full"):
        bad = dict(r["got"])
        bad[key] = fn(r["got"][key])
        assert not np.array_equal(bad[key], r["got"][key]), key
        with pytest.raises(AssertionError):
            L.compare_partition(tag, bad)
