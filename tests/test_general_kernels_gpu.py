"""GPU: the general row-tile kernels (cemlp_kernel.hpp, parity-split cemlp_ps.hpp) - what every shape without a kernel
family of its own falls to - against a float64 reference, with the configuration each case ran read back from the library.

The suite is dense around the lane families and the wide kernel; this file covers the fallback underneath them: the four
storage variants of make_plan (csrc/plan.hip: VAR_WAVE 0, VAR_GROUP 1, VAR_GROUP_NM 2, VAR_GLOBAL 3), 16- and 32-row tiles,
1 .. 4 channel tiles per row tile (MT), z aliasing the input tile (share), the block-by-block backward (phased), standalone
CEMLPs of 1 .. 4 blocks, and Cl(4,0) / Cl(3,1), which nothing compared below 65 channels before.

Reference and bound (tests/general_helpers.py): the float64 oracle (oracle/ref_path.py) on seeded O.synthetic_complex inputs
and O.init_*_params(randomize=True); for the two cases where a workgroup walks many row tiles the float64 C++ twin. Every
tensor - output, d/dh or d/dx, d/d edge_attr and d/d node_attr wherever the case has attributes, every parameter gradient -
within max(1e-5, slack x the float32 reference's own error against float64), tensor-level and element-wise (`check`);
slack 4 on the definite metrics, 10 on Cl(3,1) / Cl(4,1) with the negative-generator blades of the input scaled by 0.02.

Inputs of the indefinite EGCL cases: besides the 0.02 scaling they must be well conditioned, judged by the references alone
(general_helpers.well_conditioned, asserted in the child before the comparison): the float32 C++ twin, which sums in another
order than the float32 oracle, is itself within the bound of every tensor. egcl-cl31-48 with the seed of its tag is not: the
float32 oracle is up to 9.8e-5 off float64 there, the float32 twin misses the bound on 19 of 44 tensors (worst
g.edge_model.layers.0.2.linear_left.bias: twin 2.3e-5, oracle 1.2e-6, bound 1.2e-5) and the general kernels gave 1.6e-5 on
that tensor - between the two float32 references, so no kernel error; the case takes the next seed (general_helpers.RESEED),
same shape, algebra and bound, and is then at 0.14 x its bound (worst tensor), like the others.

Every case proves which configuration it ran: the switches are read once per process and the backward runs on autograd's
thread, so each case runs - and is compared - in a child process with CSMPN_DEBUG=1 (one child per environment and group of
cases: n4, n5, cemlp, nolanes [CSMPN_NO_PG/_PLW/_PL/_CL=1], h2 [CSMPN_FORCE_H=2], phased [CSMPN_PHASED_MIN_ROWS=64], walk;
started one after another, none after a child that did not end cleanly). The `[csmpn] mode=.. bwd=.. var=..` lines between
the case's two markers are its launches: the per-case test asserts the comparison passed, that exactly the stages of the
case appear with the case's row counts, and that no family line (pq / pg / plw / pl / cl / cm) and no wide line appears.
test_coverage_of_planner_configurations asserts over the union of the PASSED cases: var 0, 1, 3 forward and backward, var 2
backward, MT 1 .. 4, H=2 forward and backward, share=1, phased=1, ps=1 and ps=0 on D = 32, lds=0 on n = 4 and on n = 5,
all six algebras, CEMLPs of 1 .. 4 blocks. Nothing about the variant of a case is hard-coded in the tests.

Not reachable: var=2 in a FORWARD launch. choose_variant gets mirror_bytes = 0 for a forward, so its VAR_GROUP test
(`fit(mirror_bytes)`) is the no-mirror test (`fit(0)`) already; every forward whose tiles fit the LDS logs var=1 (or 0) with
mirror=0, e.g. the edge forward of egcl-cl40-48, whose backward is var=2: `mode=1 bwd=0 var=1 .. MT=3 RT=1 .. mirror=0`.

Cases (tests/general_helpers.py::CASES): what each was chosen for, and the planner's decision per stage - ef / nf / nb / eb =
edge / node forward / backward, f / b for a CEMLP; v = var, RT = row tiles per workgroup - as make_plan's arithmetic gives
it for the case's widths (tile_layout / choose_variant with 160 KiB of LDS; 35 product paths at n = 4, 56 at n = 5). The
tests do not rely on this column: they read the decision from the log of the run they compared.

    egcl-cl40-5: n = 4 narrow: var 0 (single-wave tiles, weights in LDS), fewer rows than a tile
        plan: ef v0 MT1 RT5; nf v0 MT1 RT8; nb v0 MT1 RT4 share; eb v0 MT1 RT4
    egcl-cl40-8: n = 4 at the lane width of n = 3: var 0, sum, no residual
        plan: ef v0 MT1 RT8; nf v0 MT1 RT7; nb v0 MT1 RT3; eb v0 MT1 RT4 share
    egcl-cl40-12: 12 channels (no multiple of 16), no attributes, isolated nodes + duplicates
        plan: ef v0 MT1 RT8; nf v0 MT1 RT5; nb v0 MT1 RT2; eb v0 MT1 RT4 share
    egcl-cl40-20: MT 2, hidden 12 != out 20
        plan: ef v1 MT2 RT3; nf v1 MT2 RT2; nb v1 MT2 RT1; eb v1 MT2 RT2 share
    egcl-cl40-33: MT 3 with one channel in the last tile; backward without mirror (var 2)
        plan: ef v1 MT3 RT2; nf v1 MT3 RT1; nb v2 MT3 RT1; eb v2 MT3 RT1 share
    egcl-cl40-48: backward tiles fit the LDS only without the gradient mirror (var 2)
        plan: ef v1 MT3 RT1; nf v1 MT3 RT1; nb v2 MT3 RT1 share; eb v2 MT3 RT1
    egcl-cl40-64: MT 4; forward in LDS, node stages in global scratch (lds=0 on n = 4)
        plan: ef v1 MT4 RT1; nf v3 MT4 RT1 lds=0; nb v3 MT4 RT1 lds=0; eb v2 MT4 RT1 share
    egcl-cl31-5: Cl(3,1) narrow, rewired
        plan: ef v0 MT1 RT5; nf v0 MT1 RT8; nb v0 MT1 RT4 share; eb v0 MT1 RT4
    egcl-cl31-8: Cl(3,1) var 0, no attributes
        plan: ef v0 MT1 RT8; nf v0 MT1 RT8; nb v0 MT1 RT4 share; eb v0 MT1 RT4
    egcl-cl31-12: Cl(3,1), hidden 20 != out 12: MT 2 from the hidden width
        plan: ef v1 MT2 RT3; nf v1 MT2 RT3; nb v1 MT2 RT2 share; eb v1 MT2 RT2 share
    egcl-cl31-20: Cl(3,1) MT 2, rewired
        plan: ef v1 MT2 RT3; nf v1 MT2 RT2; nb v1 MT2 RT1; eb v1 MT2 RT2 share
    egcl-cl31-33: Cl(3,1) MT 3, ragged last channel tile
        plan: ef v1 MT3 RT2; nf v1 MT3 RT1; nb v2 MT3 RT1; eb v2 MT3 RT1 share
    egcl-cl31-48: Cl(3,1) var 2 backward
        plan: ef v1 MT3 RT1; nf v1 MT3 RT1; nb v2 MT3 RT1 share; eb v2 MT3 RT1
    egcl-cl31-64: Cl(3,1) MT 4, global scratch in the node stages
        plan: ef v1 MT4 RT1; nf v3 MT4 RT1 lds=0; nb v3 MT4 RT1 lds=0; eb v2 MT4 RT1 share
    egcl-cl50-5: D = 32, at most 8 channels: the parity-split kernels (ps=1)
        plan: ef v0 MT1 RT4 ps; nf v0 MT1 RT4 ps; nb v0 MT1 RT2 ps; eb v0 MT1 RT2 ps
    egcl-cl50-12: D = 32 outside the lane widths, ps=0, MT 1
        plan: ef v0 MT1 RT3; nf v0 MT1 RT2; nb v0 MT1 RT1 share; eb v0 MT1 RT1
    egcl-cl50-20: D = 32, MT 2, hidden 12 != out 20
        plan: ef v1 MT2 RT1; nf v1 MT2 RT1; nb v2 MT2 RT1 share; eb v1 MT2 RT1 share
    egcl-cl50-40: D = 32 from 36 channels on: global scratch both ways
        plan: ef v3 MT3 RT1 lds=0; nf v3 MT3 RT1 lds=0; nb v3 MT3 RT1 lds=0; eb v3 MT3 RT1 lds=0
    egcl-cl50-48: D = 32, MT 3, global scratch
        plan: ef v3 MT3 RT1 lds=0; nf v3 MT3 RT1 lds=0; nb v3 MT3 RT1 lds=0; eb v3 MT3 RT1 lds=0
    egcl-cl50-64: D = 32, MT 4, global scratch
        plan: ef v3 MT4 RT1 lds=0; nf v3 MT4 RT1 lds=0; nb v3 MT4 RT1 lds=0; eb v3 MT4 RT1 lds=0
    egcl-cl41-12: Cl(4,1) MT 1, no attributes
        plan: ef v0 MT1 RT5; nf v0 MT1 RT2; nb v0 MT1 RT1 share; eb v0 MT1 RT1
    egcl-cl41-20: Cl(4,1) MT 2, rewired, no residual
        plan: ef v1 MT2 RT1; nf v1 MT2 RT1; nb v2 MT2 RT1 share; eb v2 MT2 RT1
    egcl-cl41-40: Cl(4,1), hidden 24 != out 40, global scratch
        plan: ef v3 MT3 RT1 lds=0; nf v3 MT3 RT1 lds=0; nb v3 MT3 RT1 lds=0; eb v3 MT3 RT1 lds=0
    egcl-cl41-48: Cl(4,1) MT 3, global scratch
        plan: ef v3 MT3 RT1 lds=0; nf v3 MT3 RT1 lds=0; nb v3 MT3 RT1 lds=0; eb v3 MT3 RT1 lds=0
    egcl-cl41-64: Cl(4,1) MT 4, global scratch
        plan: ef v3 MT4 RT1 lds=0; nf v3 MT4 RT1 lds=0; nb v3 MT4 RT1 lds=0; eb v3 MT4 RT1 lds=0
    nolane-cl50-28: the hulls width with CSMPN_NO_PG / _PLW / _PL
        plan: ef v1 MT2 RT1; nf v3 MT2 RT2 lds=0; nb v3 MT2 RT2 lds=0; eb v2 MT2 RT1 share
    nolane-cl41-16: a wide parity-lane width with those families off
        plan: ef v0 MT1 RT2; nf v0 MT1 RT1; nb v1 MT1 RT1 share; eb v1 MT1 RT1 share
    nolane-cl30-8: S1's width with CSMPN_NO_CL
        plan: ef v0 MT1 RT8; nf v0 MT1 RT6; nb v0 MT1 RT4; eb v0 MT1 RT3
    cemlp-cl30-1: 1 block, 1 row
        plan: f v0 MT1 RT6; b v0 MT1 RT4
    cemlp-cl30-2: 2 blocks 70 -> 48 -> 48, 17 rows
        plan: f v1 MT3 RT2; b v2 MT3 RT1 share
    cemlp-cl30-3: 3 blocks: two saved block inputs, 100 rows
        plan: f v0 MT1 RT5; b v0 MT1 RT4
    cemlp-cl30-4: 4 blocks 70 -> 48 x 4
        plan: f v1 MT3 RT2; b v2 MT3 RT1 share
    cemlp-cl40-1: n = 4, 1 block 70 -> 48
        plan: f v1 MT3 RT1; b v2 MT3 RT1 share
    cemlp-cl40-2: n = 4, 2 blocks
        plan: f v0 MT1 RT6; b v0 MT1 RT3 share
    cemlp-cl40-3: n = 4, 3 blocks, 1 row
        plan: f v1 MT3 RT1; b v2 MT3 RT1 share
    cemlp-cl40-4: n = 4, 4 blocks 20 -> 12 x 4
        plan: f v0 MT1 RT5; b v0 MT1 RT1
    cemlp-cl41-1: D = 32, 1 block
        plan: f v0 MT1 RT3; b v0 MT1 RT1
    cemlp-cl41-2: D = 32, 2 blocks 70 -> 48 -> 48, 1 row, global scratch
        plan: f v3 MT3 RT1 lds=0; b v3 MT3 RT1 lds=0
    cemlp-cl41-3: D = 32, 3 blocks
        plan: f v0 MT1 RT2; b v0 MT1 RT1 share
    cemlp-cl41-4: D = 32, 4 blocks in global scratch
        plan: f v3 MT3 RT1 lds=0; b v3 MT3 RT1 lds=0
    cemlp-cl30-share: share=1: z aliases the input tile
        plan: f v0 MT1 RT6; b v0 MT1 RT3 share
    h2-cl30-5: CSMPN_FORCE_H=2: 32-row tiles, 37 / 101 rows
        plan: ef v0 MT1 RT5 H2; nf v0 MT1 RT8 H2; nb v0 MT1 RT4 H2; eb v0 MT1 RT4 H2
    h2-cl20-7: CSMPN_FORCE_H=2 on Cl(2,0)
        plan: ef v0 MT1 RT8 H2; nf v0 MT1 RT8 H2; nb v0 MT1 RT4 H2; eb v0 MT1 RT4 H2
    phased-cemlp-cl30-3: phased=1: the block-by-block backward, 3 blocks
        plan: f v1 MT2 RT4; b v1 MT2 RT2 phased
    phased-cemlp-cl30-4: 4 blocks of 48 above the phased threshold
        plan: f v1 MT3 RT2; b v2 MT3 RT1 share
    phased-egcl-cl20-40: the NBA width above the phased threshold
        plan: ef v1 MT3 RT2; nf v1 MT3 RT2; nb v1 MT3 RT1 phased; eb v1 MT3 RT1
    walk-cl20-40: tile walk with tiles in LDS (twin)
        plan: ef v1 MT3 RT2; nf v1 MT3 RT2; nb v1 MT3 RT1 phased; eb v1 MT3 RT1
    walk-cl50-40: tile walk with tiles in global scratch (twin)
        plan: ef v3 MT3 RT1 lds=0; nf v3 MT3 RT1 lds=0; nb v3 MT3 RT1 lds=0; eb v3 MT3 RT1 lds=0

Deterministic mode: a hard request on an n = 4 shape must fail with CSMPN_ERR_UNSUPPORTED and run_rows' text
(test_deterministic_refused_on_n4); the Cl(2,0) 40-channel case - two runs bit-identical and within the bound - is held by
tests/test_deterministic.py::test_bit_reproducible / ::test_parity_vs_oracle already and not repeated.
test_comparison_can_fail keeps the comparison honest: a parameter gradient scaled by 1 + 1e-3 must be rejected.
"""
import numpy as np
import pytest
import torch

import general_helpers as H
from general_helpers import CASES, GROUPS, group_of, group_tags, run_group

pytestmark = pytest.mark.gpu

EGCL_STAGES = {(1, 0), (2, 0), (2, 1), (1, 1)}    # (mode, bwd): edge / node forward, node / edge backward
CEMLP_STAGES = {(0, 0), (0, 1)}


def _result(tag):
    return run_group(group_of(tag))[tag]


@pytest.mark.parametrize("tag", list(CASES))
def test_general_kernels_against_float64(tag):
    """One case of tests/general_helpers.py::CASES, compared in its group's child process: output, d/d input, d/d attributes
    and every parameter gradient within the suite's bound; and the log of that very run shows the stages of the case on the
    general kernels - no lane family, no wide kernel."""
    r = _result(tag)
    print(tag, r["message"], *r["log"], sep="\n")
    assert r["ok"], r["message"]
    assert not r["other"], r["other"]
    stages = EGCL_STAGES if CASES[tag]["kind"] == "egcl" else CEMLP_STAGES
    assert {(l["mode"], l["bwd"]) for l in r["launches"]} == stages, r["log"]
    rows = {CASES[tag]["N"], CASES[tag]["E"]} if CASES[tag]["kind"] == "egcl" else {CASES[tag]["rows"]}
    assert {l["rows"] for l in r["launches"]} == rows, r["log"]


def _launches(pred=lambda tag: True):
    """(tag, launch) of every general-kernel launch of a case that PASSED its comparison in the same process."""
    out = []
    for group in GROUPS:
        for tag, r in run_group(group).items():
            if r["ok"] and not r["other"] and pred(tag):
                out += [(tag, l) for l in r["launches"]]
    return out


def test_coverage_of_planner_configurations():
    """The union over all compared cases holds every configuration the planner has for these kernels. (A forward launch
    never takes var = 2: see the module docstring.)"""
    L = _launches()
    seen = lambda **kw: sorted({tag for tag, l in L if all(l[k] == v for k, v in kw.items())})
    missing = []
    want = [dict(var=v, bwd=b) for v in (0, 1, 3) for b in (0, 1)] + [dict(var=2, bwd=1)]
    want += [dict(MT=m) for m in (1, 2, 3, 4)] + [dict(H=2, bwd=0), dict(H=2, bwd=1), dict(share=1), dict(phased=1)]
    for kw in want:
        tags = seen(**kw)
        print(kw, "witnessed by", tags)
        if not tags:
            missing.append(kw)
    # ps = 1 and ps = 0 on D = 32; global scratch on n = 4 and n = 5; every algebra; CEMLPs of 1..4 blocks
    by_n = lambda n: lambda tag: len(CASES[tag]["metric"]) == n
    for what, pred, kw in [("ps=1 on D=32", by_n(5), dict(ps=1)), ("ps=0 on D=32", by_n(5), dict(ps=0)),
                           ("lds=0 on n=4", by_n(4), dict(lds=0)), ("lds=0 on n=5", by_n(5), dict(lds=0))]:
        tags = sorted({tag for tag, l in _launches(pred) if all(l[k] == v for k, v in kw.items())})
        print(what, "witnessed by", tags)
        if not tags:
            missing.append(what)
    for metric, name in H.ALG_NAMES.items():
        if not _launches(lambda tag: CASES[tag]["metric"] == metric):
            missing.append(name)
    for nl in (1, 2, 3, 4):
        cem = lambda tag: CASES[tag]["kind"] == "cemlp" and CASES[tag]["nl"] == nl and max(CASES[tag]["widths"][1:]) <= 64
        if not {l["bwd"] for _, l in _launches(cem)} == {0, 1}:
            missing.append(f"standalone CEMLP of {nl} blocks")
    assert not missing, missing
    # the global-scratch launches are VAR_GLOBAL, and only they
    assert all((l["lds"] == 0) == (l["var"] == 3) for _, l in L)


def test_h2_cases_have_ragged_32_row_tiles():
    for tag in group_tags("h2"):
        r = _result(tag)
        assert r["ok"] and r["launches"] and all(l["H"] == 2 for l in r["launches"]), r["log"]
        for l in r["launches"]:
            assert l["rows"] % 32 != 0 and l["rows"] > 32, l


@pytest.mark.parametrize("tag", group_tags("walk"))
def test_walk_cases_walk(tag):
    """From the case's own log: every stage has more rows than grid x RT row tiles hold, so every workgroup ran its tile
    loop more than once; the last sweep is ragged (rows no multiple of the tile) and leaves workgroups with a masked pass."""
    r = _result(tag)
    assert r["ok"], r["message"]
    assert {(l["mode"], l["bwd"]) for l in r["launches"]} == EGCL_STAGES, r["log"]
    sweeps = []
    for l in r["launches"]:
        per_sweep = l["grid"] * l["RT"] * 16 * l["H"]
        assert l["rows"] > per_sweep and l["rows"] % (16 * l["H"]) != 0, l
        sweeps.append(l["rows"] / per_sweep)
    # just above the largest sweep of the case (the forward's; a backward holds fewer tiles per workgroup and walks further):
    # all but a few workgroups run their last pass fully masked
    assert min(sweeps) < 1.01, sweeps
    placed = {l["lds"] > 0 for l in r["launches"]}
    assert placed == ({True} if tag == "walk-cl20-40" else {False}), r["log"]


def test_comparison_can_fail():
    """Mutation guard (as test_egcl_golden_can_fail): a parameter gradient scaled by 1 + 1e-3, a zeroed output, a dropped
    element of d/dh and a sign flip of d/d edge_attr must each be rejected by the comparison the cases go through."""
    tag = "egcl-cl40-8"
    got, t64, t32 = H.compute(tag)
    H.compare(tag, got, t64, t32)

    def drop_one(a):
        a.flat[np.abs(a).argmax()] = 0.0
        return a
    for key, fn in [("g.edge_model.layers.0.0.weight", lambda a: a * (1.0 + 1e-3)), ("y", lambda a: a * 0.0), ("gh", drop_one),
                    ("g_edge_attr", lambda a: -a), ("g.node_model.layers.1.3.a", lambda a: a * (1.0 + 1e-3))]:
        bad = dict(got)
        bad[key] = fn(got[key].copy())
        with pytest.raises(AssertionError):
            H.compare(tag, bad, t64, t32)


@pytest.mark.parametrize("metric,C", [(H.CL40, 12), (H.CL31, 48)], ids=["cl40-12", "cl31-48"])
def test_deterministic_refused_on_n4(metric, C):
    """A hard deterministic request on an n = 4 shape of the general kernels fails with CSMPN_ERR_UNSUPPORTED and the text
    run_rows gives - it does not run the float atomics - and the atomic path of the same layer still runs afterwards.
    (Cl(2,0) at 40 channels, two bit-identical runs within the bound: test_deterministic.py::test_bit_reproducible and
    ::test_parity_vs_oracle hold that case already.)"""
    pkg = H._pkg()
    from csmpn_hip import native, ops
    h, ei, ea, na = (t.to(H.dev()) for t in H.O.synthetic_complex(H.O.Algebra(list(metric)), 20, 70, C, seed=5))
    torch.manual_seed(6)
    layer = pkg.EGCL(pkg.CliffordAlgebra(tuple(metric)), C, C, C, edge_attr_features=6, node_attr_features=3).to(H.dev())
    ops.set_deterministic(True)
    try:
        with pytest.raises(native.CsmpnError, match=f"error {native.ERR_UNSUPPORTED}: CSMPN_FLAG_DETERMINISTIC: this shape is "
                                                    "served neither by the lane kernels"):
            layer(h, ei, ea, na)
            torch.cuda.synchronize()
    finally:
        ops.set_deterministic(None)
    assert bool(torch.isfinite(layer(h, ei, ea, na)).all())
