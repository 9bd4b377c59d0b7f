"""The float64 reference of tests/embed_helpers.py and its case table, checked without a GPU.

* Against the hulls stage fixture: on the batch and parameters of tests/golden/model_hulls.npz the reference of the edge and
  triangle rows reproduces `f64/embedding/rows` of stages_hulls.npz (every 8th row of the embedding, recorded from the
  imported reference's own embed_simplicial_complex).
* Every case's float32 yardsticks meet the cap (1e-5) under which the suite's bound max(1e-5, 4 x yardstick) is read.
* The index tables have the properties the cases claim; row, tile and group counts are as in the case table.
"""
import math
import os

import numpy as np
import pytest
import torch

import embed_helpers as E
from embed_helpers import BASES, CASES, CLAMP_BASES
from general_helpers import CL50, relmax

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_reference_reproduces_the_hulls_stage_fixture(pkg):
    """`f64/embedding/rows` is stored as float32, so agreement is required to one float32 rounding of each element (half a
    unit in the last place, 2^-24 relative, plus 1e-12 of the tensor's scale for the entries near zero). Measured: 39 rows of
    dimension >= 1 among the 43 stored ones; the largest difference is 4.65e-8 of the tensor's scale and 0.50 units in the
    last place of the element at its worst."""
    from test_model_harness import load_batch
    g = np.load(os.path.join(GOLD, "model_hulls.npz"))
    st = np.load(os.path.join(GOLD, "stages_hulls.npz"))
    fix = st["f64/embedding/rows"]
    assert fix.dtype == np.float32    # the precision the bound below is written for
    batch = load_batch(pkg, g)
    plan = batch.plan(2)
    B, vr = batch.num_graphs, plan["vertex_rows"]
    inp = batch.input.double()
    pos = inp[vr].reshape(B, -1, 5)
    inp = inp.index_copy(0, vr, (pos - pos.mean(dim=1, keepdim=True)).reshape(-1, 5))    # hulls_cssmpnn.py:145-148
    feat = E.O.embed_grade(E._alg(CL50, torch.float64), inp.unsqueeze(1), 1)
    full = torch.full((batch.x_ind.shape[0], 28, 32), float("nan"), dtype=torch.float64)
    for d in (1, 2):
        prefix = f"p/cl_feature_embedding.{d}."
        p = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
        assert len(p) == 10 * d
        y = E.reference_run(CL50, feat, plan["verts"][d], math.factorial(d + 1), p, None, torch.float64)["y"]
        full[plan["rows"][d]] = torch.from_numpy(y)
    stored = torch.arange(0, full.shape[0], 8)
    keep = (batch.node_types[stored] >= 1).numpy()
    mine, want = full[stored].numpy()[keep], fix.astype(np.float64)[keep]
    assert keep.sum() >= 20 and np.isfinite(mine).all()
    scale = np.abs(want).max()
    diff = np.abs(mine - want)
    print(f"{keep.sum()} rows, max diff {diff.max() / scale:.2e} of the scale, {(diff / np.spacing(np.abs(want).astype(np.float32))).max():.2f} ulp")
    assert (diff <= 2.0 ** -24 * np.abs(mine) + 1e-12 * scale).all(), float((diff / scale).max())


@pytest.fixture(scope="module")
def refs():
    """(float64, float32) runs of every seed tag: `reference` asserts the cap on every yardstick."""
    return {b: E.reference(b, table=E.clamped if b in CLAMP_BASES else None) for b in list(BASES) + list(CLAMP_BASES)}


def test_every_float32_yardstick_is_under_the_cap(refs):
    """The condition of the bound, asserted case by case inside embed_helpers.reference (the clamp cases on their clamped
    table). Measured, worst tensor of each case: 6.7e-7 .. 6.1e-6, nearly always g.layers.0.1.a; y 6e-8 .. 5e-7; the seeds that
    were above the cap and their figures: embed_helpers.RESEED."""
    worst = {}
    for b, (t64, t32) in refs.items():
        yard = {k: relmax(t32[k], t64[k]) for k in t64}
        assert set(t64) == set(t32) and len(t64) == 1 + 10 * (BASES.get(b) or CLAMP_BASES[b])["nl"]
        k = max(yard, key=yard.get)
        assert yard[k] <= E.YARD, (b, k, yard[k])
        worst[b] = (k, yard[k], yard["y"])
    for b, (k, v, y) in worst.items():
        print(f"{b:26s} {v:.2e} ({k}), y {y:.2e}")
    assert not E.RESEED or all(b in BASES or b in CLAMP_BASES for b in E.RESEED)


def test_sweep_cells_that_can_be_served_are_under_the_cap():
    """The cells of the predicate sweep the two instantiated programs can serve (out 28; 2 inputs in one block, 3 in two)."""
    for an in E.ALGS:
        for in_f, nl in ((2, 1), (3, 2)):
            c = E.sweep_case(an, 28, in_f, nl)
            E.reference(c["seed_tag"], c)


def test_tables_hold_what_the_cases_claim():
    S, P = E.S_ROWS, E.POISON_ROWS
    for b, c in list(BASES.items()) + list(CLAMP_BASES.items()):
        feat, verts, p, gout = E.case_inputs(c, E.SUITE.seed_of(b))
        rows, no, ns = c["nsimp"] * c["n_orders"], c["n_orders"], c["nsimp"]
        assert verts.dtype == torch.int32 and tuple(verts.shape) == (rows, c["nv"]) and tuple(feat.shape) == (S, c["kpv"], 32)
        assert tuple(gout.shape) == (ns, 28, 32) and c["nv"] * c["kpv"] == c["in_f"] <= 8
        simp = verts.reshape(ns, no * c["nv"])
        if c["kind"] == "clamp":
            assert int(verts.min()) == -1 and int(verts.max()) > S and int((verts == S).sum()) == 1
            inside = E.clamped(verts)
            assert int(inside.min()) == 0 and int(inside.max()) == S - 1
            assert not bool((feat.abs() >= E.POISON).any())
            continue
        # the last 8 feature rows: unreferenced, large and finite
        assert int(verts.min()) == 0 and int(verts.max()) == S - P - 1 and int(verts[0, 0]) == 0 and int(verts[-1, -1]) == S - P - 1
        assert bool((feat[S - P:] == E.POISON).all()) and float(feat[:S - P].abs().max()) < 10.0
        if ns >= 3:
            assert bool((simp[1] == E.SAME_ID).all())
        if ns >= 5:
            assert torch.equal(simp[ns - 2], simp[2]) and ns - 2 != 2
    # every group of 5 or 23 simplices holds all four properties; the one-, two- and three-simplex tables what fits
    assert all(c["nsimp"] >= 5 for b, c in BASES.items() if not b.startswith(("edges-", "tris-")))


def test_case_table_geometry():
    geo = lambda b: E.geometry(BASES[b])
    want_edges = {1: (2, 1, 1), 2: (4, 1, 1), 3: (6, 2, 2), 5: (10, 3, 3), 23: (46, 12, 12)}      # rows, tiles, groups
    want_tris = {1: (6, 2, 1), 2: (12, 3, 1), 3: (18, 5, 2), 5: (30, 8, 3), 23: (138, 35, 12)}
    for an in E.ALGS:
        for ns in E.SMALL:
            assert tuple(geo(f"edges-{an}-{ns}").values()) == want_edges[ns]
            assert tuple(geo(f"tris-{an}-{ns}").values()) == want_tris[ns]
        assert tuple(geo(f"abi-{an}-o6-v2k1").values()) == (42, 11, 4) and tuple(geo(f"abi-{an}-o1-v1k2").values()) == (7, 2, 2)
        assert (BASES[f"abi-{an}-o2-v1k3"]["nl"], BASES[f"abi-{an}-o1-v3k1"]["nl"], BASES[f"abi-{an}-o6-v2k1"]["nl"]) == (2, 2, 1)
    # triangles: 2 simplices fill exactly one 12-row group; 1, 3, 5 and 23 end in a group with one simplex and a half tile
    for ns in (1, 3, 5, 23):
        rows = 6 * ns
        assert rows % 12 == 6 and rows % 4 == 2
    # the walks: the forward cap is 512 workgroups, the backward's 256
    e, t = geo("walk-edges-cl50-1031"), geo("walk-tris-cl50-1031")
    assert tuple(e.values()) == (2062, 516, 516) and e["tiles"] - E.FWD_CAP == 4 and e["tiles"] > E.BWD_CAP
    assert tuple(t.values()) == (6186, 1547, 516) and t["groups"] > E.FWD_CAP and t["tiles"] > E.BWD_CAP
    assert t["rows"] - (t["groups"] - 1) * 12 == 6 and t["tiles"] - (t["groups"] - 1) * 3 == 2    # last group: two tiles, one simplex
    assert t["rows"] > E.FWD_CAP * 4 * 3 and e["rows"] > E.FWD_CAP * 4 and min(e["rows"], t["rows"]) > E.BWD_CAP * 4
    for b, c in BASES.items():
        assert c["walk"] == (E.geometry(c)["groups"] > E.FWD_CAP), b


def test_groups_and_members():
    for tag, c in CASES.items():
        assert E.group_of(tag) == c["group"]
    assert sorted(t for g in E.GROUPS for t in E.group_tags(g)) == sorted(CASES)
    assert sorted(E.MEMBERS["default"]) == sorted(BASES) and len(BASES) == 2 * (10 + 4) + 2
    rec = E.MEMBERS["recompute"]
    assert all(BASES[b]["nl"] == 2 for b in rec) and "walk-tris-cl50-1031" in rec and len(rec) == 2 * (5 + 2) + 1
    assert len(E.sweep_cells()) == 2 * 6 * 6 and len(E.REFUSALS) == 7
