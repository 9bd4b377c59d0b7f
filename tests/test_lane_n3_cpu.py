"""Host side of tests/test_lane_n3_gpu.py (no GPU): the case table, the expected-dispatch table, the tile geometry and the
coverage of tests/lane_n3_helpers.py, and the condition every case's inputs must meet before a kernel is held to the bound -
each yardstick (float32 oracle against float64 oracle; float32 twin against float64 twin on the walks) at most 1e-5, so that
`check`'s bound max(1e-5, 4 x yardstick) is its floor on every tensor.

The references are computed once per seed tag and kept for the session (lane_n3_helpers.yardsticks): the GPU tests of the same
session read the same ones.
"""
import pytest

import lane_n3_helpers as L
from lane_n3_helpers import CASES


def _tags(pred):
    return [t for t, c in CASES.items() if pred(c)]


def test_every_tag_in_exactly_one_group():
    for tag, c in CASES.items():
        assert L.group_of(tag) == c["group"]    # group_of asserts that exactly one predicate holds
    assert sorted(t for g in L.GROUPS for t in L.group_tags(g)) == sorted(CASES)
    assert set(L.EXPECTED) == set(L.GROUPS) == set(L.GROUP_ENV) == set(L.MEMBERS)
    assert {b for bases in L.MEMBERS.values() for b in bases} == set(L.BASES)    # no seed tag without a case


def test_expected_dispatch_covers_every_case():
    for tag, c in CASES.items():
        want = L.expected(tag)    # a KeyError here: a case in a group whose table has no row for its width or its stages
        assert set(want) == set(L.stages_of(c)) and set(c["walks"]) <= set(want), tag
        for stage in want:
            assert L.expected_label(c["group"], L.channels_of(c), stage)
        if c["kind"].startswith("guard_"):
            for v in L.GUARD_VARIANTS:
                assert set(L.expected(tag, L.guard_group(c["group"], v))) == set(want), (tag, v)
    # the switches act as the table says: a lane backward only where the group leaves cm's saved regions; pq only without CSMPN_NO_PQ
    for group, env in L.GROUP_ENV.items():
        for row in L.EXPECTED[group].values():
            assert ("CSMPN_NO_CM_BWD" in env) == all(f == L.GENERAL for s, f in row.items() if s[1]), group
            assert "CSMPN_NO_PQ" not in env or "pq" not in row.values(), group


def test_walk_shapes_exceed_the_stated_sweep():
    """Every launch a case says walks has more rows than one sweep of its expected kernel holds (lane_n3_helpers.sweep_rows),
    less than 1.03 sweeps of the launch the case was sized for, and no multiple of the tile; every other lane launch fits one
    sweep."""
    stated = {("cm", 16, 0): 768 * 4 * 16, ("cm", 16, 1): 256 * 8 * 16, ("cm", 32, 0): 256 * 4 * 16, ("cm", 32, 1): 256 * 2 * 16,
              ("pq", 32, 0): 768 * 16, ("pq", 32, 1): 768 * 16}
    assert stated[("cm", 16, 0)] == 49152 and stated[("cm", 16, 1)] == 32768 and stated[("cm", 32, 1)] == 8192
    for key, rows in stated.items():
        assert L.sweep_rows(*key) == rows, key
    walking = _tags(lambda c: c["walks"])
    assert len(walking) == 3 + 1 + 2 + 2 + 3    # default, recompute, nopq / nopq-recompute, det, plain
    for tag in walking:
        c = CASES[tag]
        channels, rows_of = L.channels_of(c), L.stage_rows(tag)
        ratios = []
        for stage, family in L.expected(tag).items():
            assert family != L.GENERAL, (tag, stage)
            sweep = L.sweep_rows(family, channels, stage[1])
            assert (rows_of(stage) > sweep) == (stage in c["walks"]), (tag, stage, rows_of(stage), sweep)
            if stage in c["walks"]:
                assert rows_of(stage) % L.TILE != 0 and rows_of(stage) - sweep > 16, (tag, stage)
                ratios.append(rows_of(stage) / sweep)
        assert 1.0 < min(ratios) < 1.03, (tag, ratios)
    for tag in _tags(lambda c: not c["walks"] and not c["kind"].startswith("guard_")):
        c = CASES[tag]
        for stage, family in L.expected(tag).items():
            assert family == L.GENERAL or L.stage_rows(tag)(stage) <= L.sweep_rows(family, L.channels_of(c), stage[1]), (tag, stage)


def test_coverage_matrix():
    """Every LaneEntry of cm_inst.inc and k_pq_n3.hip, forward and backward, with and without saved state where both exist, is
    the expected kernel of some case; each at a walk; the small matrix alternates aggr and the residual per family."""
    covered, walked = set(), set()
    for tag, c in CASES.items():
        if c["kind"].startswith("guard_"):
            continue
        channels = L.channels_of(c)
        for (mode, bwd), family in L.expected(tag).items():
            if family == L.GENERAL:
                continue
            shape = (c["nl"], c["widths"][0]) if mode == 0 else None
            state = L.saves_state(c["group"], channels) if channels == 32 else None
            key = (family, channels, mode, shape, bwd, state)
            covered.add(key)
            if (mode, bwd) in c["walks"]:
                walked.add(key)
    want = set()
    for mode in (1, 2):
        # cm_inst.inc: cm_entry<16, EDGE, 2, 6>, <16, NODE, 2, 3>, <32, EDGE, 2, 6>, <32, NODE, 2, 3>; cmb at 16 channels, cmp <true> / <false> at 32
        want |= {("cm", 16, mode, None, bwd, None) for bwd in (0, 1)}
        want |= {("cm", 32, mode, None, bwd, state) for bwd in (0, 1) for state in (True, False)}
        # k_pq_n3.hip: pq_entry<EDGE, 2, 6>, <NODE, 2, 3>: the forward with and without state, the backward on the state
        want |= {("pq", 32, mode, None, 0, True), ("pq", 32, mode, None, 0, False), ("pq", 32, mode, None, 1, True)}
    for shape in L.PLAIN_PROGRAMS:    # pq_entry<PLAIN, 1, 60>, <PLAIN, 2, 90>, <PLAIN, 1, 32>
        want |= {("pq", 32, 0, shape, 0, True), ("pq", 32, 0, shape, 0, False), ("pq", 32, 0, shape, 1, True)}
    assert covered == want, (sorted(want - covered, key=str), sorted(covered - want, key=str))
    # a walk of every kernel: all but the pq forwards without state (the same tile loop; their backward is cmp or general)
    assert want - walked == {k for k in want if k[0] == "pq" and k[4] == 0 and k[5] is False}, sorted(want - walked, key=str)
    # the small matrix: all four shapes where the group changes a launch of the width; aggr and the residual both ways per width
    shapes = {(n, e) for n, e, _ in L.SMALL_SHAPES}
    for group, widths in (("recompute", (32,)), ("nopq", (32,)), ("nopq-recompute", (32,)), ("nocmbwd", (16, 32)), ("det", (16, 32))):
        for C in widths:
            small = [c for c in CASES.values() if c["group"] == group and c["kind"] == "egcl" and c["ref"] == "oracle" and c["C"] == C]
            assert {(c["N"], c["E"]) for c in small} == shapes, (group, C)
            assert {c["aggr"] for c in small} == {"mean", "sum"} and {c["residual"] for c in small} == {True, False}, (group, C)
    assert {(c["C"], c["E"]) for c in CASES.values() if c["group"] == "default" and c["ref"] == "oracle"} == {(16, 101), (32, 258)}
    # sentinels: each forward that writes state (pq edge / node / two-block plain; cm edge / node at 32 channels) at 23 or 39 rows
    # and at a walk size, and the same programs where the buffer has no state regions
    guards = {(c["group"], c["kind"], c.get("E", c.get("rows"))) for c in CASES.values() if c["kind"].startswith("guard_")}
    assert guards == {("default", "guard_egcl", 39), ("default", "guard_egcl", 12341), ("plain", "guard_cemlp", 23),
                      ("plain", "guard_cemlp", 12341), ("nopq", "guard_egcl", 39), ("nopq", "guard_egcl", 16437),
                      ("nocmbwd", "guard_egcl", 39), ("nocmbwd", "guard_egcl", 12341), ("nocmbwd", "guard_cemlp", 23),
                      ("nopq-nocmbwd", "guard_egcl", 39), ("nopq-nocmbwd", "guard_egcl", 16437)}


@pytest.mark.parametrize("base", [b for b, c in L.BASES.items() if c["ref"]])
def test_yardstick_cap(base):
    """The inputs of every seed tag deserve the floor: the float32 reference run is within 1e-5 of the float64 one on every
    tensor (host only; RESEED holds the offsets of the tags whose first seed is not)."""
    tag = next(t for t, c in CASES.items() if c["seed_tag"] == base)
    t64, t32, yard = L.yardsticks(tag)
    c = CASES[tag]
    assert set(t64) == set(t32) and len(t64) == (2 + 10 * c["nl"] if c["kind"] == "cemlp" else 4 + 40)
    worst = max(yard, key=yard.get)
    print(f"{base}: worst yardstick {yard[worst]:.2e} ({worst})")
    assert yard[worst] <= L.YARD, f"{base}: yardstick of {worst} is {yard[worst]:.3e} > {L.YARD:.0e}"
    assert L.reference(tag)[0] is t64
