"""The references of tests/glue_helpers.py are validated here, without a GPU, before tests/test_glue_kernels_gpu.py holds
the kernels of csrc/glue.hip to them:

* on the inputs of the readout fixtures recorded from the imported reference models (tests/golden/readout_{hulls,motion,
  nba,md17}.npz, make_model_golden.py) the float64 run of the helper's references reproduces the fixtures' `f64/*`
  tensors - every loss part, d/dx and the head's parameter gradients - to 1e-12 relmax. The fixtures keep `f64/gx`
  rounded to float32 (make_model_golden.py: `.astype(np.float32)`), so 1e-12 cannot hold for that one tensor: ours is
  rounded the same way and must then agree to one float32 rounding step (2^-23 of each element, ties in the rounding
  included). md17's head is a CEMLP in front of the MVLinear: the CEMLP runs on the float64 oracle
  (oracle/ref_path.py), as in test_traj_readout_composed_vs_fixture_cpu, and its parameter gradients are compared too;
* ops.readout_traj_tables on the CPU equals the Python-loop construction for every trajectory case, the in-place refill
  (`out=`, `vertices_per_graph=`) to a second batch of the same shapes included;
* for every case the float32 run of the reference meets the bound of DESIGN.md §2 against the float64 run with factor 1 in
  place of 4 (the element-wise part is what can fail) and is finite everywhere - the unscored rows of T2 / T5 / T6 and the
  |d| = 0 items included -, so the GPU test never rests on an ill-conditioned input.
"""
import os

import numpy as np
import pytest
import torch

import glue_helpers as G
from oracle import ref_path as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIX_TOL = 1e-12


def _fixture_check(name, g, got):
    for k, t in got.items():
        truth = g[f"f64/{k}"]
        mine = t.detach().double().numpy()
        assert mine.shape == truth.shape, (name, k, mine.shape, truth.shape)
        if truth.dtype == np.float32:       # gx: stored rounded to float32
            r = mine.astype(np.float32).astype(np.float64)
            t64 = truth.astype(np.float64)
            assert np.all(np.abs(r - t64) <= 2.0 ** -23 * np.abs(t64)), (name, k, float(np.abs(r - t64).max()))
        elif np.abs(truth).max() == 0:
            assert np.all(mine == 0), (name, k)
        else:
            assert G.relmax(mine, truth) <= FIX_TOL, (name, k, G.relmax(mine, truth))
    assert {k for k in g.files if k.startswith("f64/")} == {"f64/" + k for k in got}, name


def _graph_sizes(g, B):
    """(vertex rows, vertices per graph) of a fixture batch: the vertices are the rows of node type 0."""
    vr = torch.from_numpy(np.nonzero(g["b/node_types"] == 0)[0]).long()
    gov = torch.from_numpy(g["b/x_ind_batch"])[vr]
    assert bool((gov[1:] >= gov[:-1]).all())
    return vr, tuple(torch.bincount(gov, minlength=B).tolist())


def test_mse_reference_reproduces_hulls_fixture():
    g = np.load(os.path.join(GOLD, "readout_hulls.npz"))
    ptr = g["ptr"]
    inp = dict(x=torch.from_numpy(g["x"]), weight=torch.from_numpy(g["p/0.weight"]), bias=torch.from_numpy(g["p/0.bias"]),
               sizes=tuple(int(b - a) for a, b in zip(ptr[:-1], ptr[1:])), target=torch.from_numpy(g["target"]),
               wl=torch.from_numpy(g["wl"]))
    r = G.mse_reference(inp, torch.float64)
    _fixture_check("hulls", g, {"loss": r["loss"], "pred": r["pred"], "gx": r["gx"], "g/0.weight": r["gw"], "g/0.bias": r["gb"]})


def test_traj_reference_reproduces_motion_fixture():
    """motion_cssmpnn.py:150-163: one out channel, residual on the positions, the loss is the per-vertex MSE."""
    g = np.load(os.path.join(GOLD, "readout_motion.npz"))
    B = g["b/x_ind_ptr"].shape[0] - 1
    vr, sizes = _graph_sizes(g, B)
    inp = dict(n=3, sizes=sizes, vrows=vr, unscored_last=0, x=torch.from_numpy(g["x"]), weight=torch.from_numpy(g["p/0.weight"]),
               loc=torch.from_numpy(g["b/pos"])[vr], target=torch.from_numpy(g["b/y"]), g_vertex=torch.from_numpy(g["w/loss"]))
    r = G.traj_reference(inp, torch.float64, use=("vertex",))
    _fixture_check("motion", g, {"loss": r["per_vertex"], "gx": r["gx"], "g/0.weight": r["gw"],
                                 "g/0.bias": torch.zeros(1, 1, 1, dtype=torch.float64)})


def test_traj_reference_reproduces_nba_fixture():
    """nba_cssmpnn.py:176-188: no residual, the last agent of a graph (the ball) is not scored, loss = ADE."""
    g = np.load(os.path.join(GOLD, "readout_nba.npz"))
    B = g["b/x_ind_ptr"].shape[0] - 1
    vr, sizes = _graph_sizes(g, B)
    gg = torch.zeros(B, 3, dtype=torch.float64)      # `loss` and `ade_loss` are the same tensor: their weights add (in float64)
    gg[:, 1] = torch.from_numpy(g["w/loss"].astype(np.float64) + g["w/ade_loss"].astype(np.float64))
    gg[:, 2] = torch.from_numpy(g["w/fde_loss"].astype(np.float64))
    inp = dict(n=2, sizes=sizes, vrows=vr, unscored_last=1, x=torch.from_numpy(g["x"]), weight=torch.from_numpy(g["p/weight"]),
               loc=None, target=torch.from_numpy(g["b/y"]), g_graph=gg)
    r = G.traj_reference(inp, torch.float64, use=("graph",))
    pg = r["per_graph"]
    _fixture_check("nba", g, {"loss": pg[:, 1], "ade_loss": pg[:, 1], "fde_loss": pg[:, 2], "gx": r["gx"], "g/weight": r["gw"],
                              "g/bias": torch.zeros(1, 40, 1, dtype=torch.float64)})


def test_traj_reference_reproduces_md17_fixture_through_the_oracle_cemlp():
    """md17_cssmpnn.py:165-176: CEMLP (float64 oracle) on the vertex rows, MVLinear, residual on loc, MSE / ADE / FDE."""
    g = np.load(os.path.join(GOLD, "readout_md17.npz"))
    B = g["b/x_ind_ptr"].shape[0] - 1
    vr, sizes = _graph_sizes(g, B)
    alg = G.algebra(3)
    p = {k[2:]: torch.from_numpy(g[k]).double().requires_grad_(True) for k in g.files if k.startswith("p/")}
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    z = O.cemlp(alg, x.index_select(0, vr), p, prefix="0.")
    _pred, pg, _pv = G.traj_forward(z, p["1.weight"], torch.from_numpy(g["b/loc"])[vr], torch.from_numpy(g["b/y"]), sizes, None, 0, 3)
    names = {"loss": 0, "ade_loss": 1, "fde_loss": 2}
    total = sum((pg[:, j] * torch.from_numpy(g[f"w/{k}"]).double()).sum() for k, j in names.items())
    keys = sorted(p)
    grads = torch.autograd.grad(total, [x] + [p[k] for k in keys], allow_unused=True)
    got = {k: pg[:, j] for k, j in names.items()}
    got["gx"] = grads[0]
    for k, gr in zip(keys, grads[1:]):
        got["g/" + k] = gr if gr is not None else torch.zeros_like(p[k])
    assert bool((got["g/1.bias"] == 0).all())
    _fixture_check("md17", g, got)


@pytest.mark.parametrize("tag", sorted(G.TRAJ_CASES))
def test_traj_tables_equal_loop_construction(pkg, tag):
    from csmpn_hip import ops
    c = G.TRAJ_CASES[tag]

    def loop_and_args(second):
        sizes, vrows, S = G.traj_topology(tag, second)
        want = G.traj_tables_loop(sizes, vrows, S, c["unscored_last"])
        kw = dict(unscored_last=c["unscored_last"])
        if vrows is not None:
            kw.update(vertex_rows=vrows, n_rows=S)
        return sizes, want, want["graph_of_vertex"].long(), kw

    def same(got, want):
        for k, w in want.items():
            assert (w is None) == (got[k] is None), (tag, k)
            if w is not None:
                assert got[k].dtype == torch.int32 and torch.equal(got[k], w), (tag, k)

    sizes, want, gov, kw = loop_and_args(False)
    first = ops.readout_traj_tables(gov, len(sizes), **kw)
    same(first, want)
    ptrs = {k: v.data_ptr() for k, v in first.items() if v is not None}
    sizes2, want2, gov2, kw2 = loop_and_args(True)
    assert sizes2 != sizes and not torch.equal(want2["graph_of_vertex"], want["graph_of_vertex"])
    again = ops.readout_traj_tables(gov2, len(sizes2), out=first, vertices_per_graph=torch.tensor(sizes2), **kw2)
    same(again, want2)
    assert {k: v.data_ptr() for k, v in again.items() if v is not None} == ptrs     # refilled in place


def _well_conditioned(name, truth, ref32):
    for k in sorted(truth):
        assert bool(torch.isfinite(ref32[k]).all()) and bool(torch.isfinite(truth[k]).all()), (name, k)
        G.check(f"{name}.{k}", ref32[k].double().numpy(), truth[k].numpy(), ref32[k].double().numpy(), 1.0)


TRAJ_RUNS = [(t, ("graph", "vertex")) for t in sorted(G.TRAJ_CASES)] + [(t, (u,)) for t in G.TRAJ_ALONE for u in ("graph", "vertex")]


@pytest.mark.parametrize("tag,use", TRAJ_RUNS, ids=[f"{t}-{'+'.join(u)}" for t, u in TRAJ_RUNS])
def test_traj_float32_reference_meets_the_bound(tag, use):
    truth, ref32 = G.traj_truth(tag, use)
    _well_conditioned(tag, truth, ref32)
    G.traj_exact_zeros(G.traj_inputs(tag), truth)
    G.traj_exact_zeros(G.traj_inputs(tag), ref32)


def test_traj_zero_distance_reference_is_finite_and_meets_the_bound():
    """The |d| = 0 items of T5 (ZERO_TIES of the GPU test): the subgradient-0 convention, no NaN in either dtype."""
    truth, ref32 = G.traj_truth("T5", ("graph", "vertex"), G.T5_TIES)
    _well_conditioned("T5-ties", truth, ref32)
    inp = G.traj_inputs("T5")
    v = G.T5_TIES[0][0]
    assert float(truth["per_vertex"][v]) == 0 and bool((truth["gx"][inp["vrows"][v]] == 0).all())


@pytest.mark.parametrize("tag", sorted(G.MSE_CASES))
def test_mse_float32_reference_meets_the_bound(tag):
    truth, ref32 = G.mse_truth(tag)
    _well_conditioned(tag, truth, ref32)
    inp = G.mse_inputs(tag)
    for b, s in enumerate(inp["sizes"]):
        if s == 0:
            assert float(truth["pred"][b]) == 0 and float(truth["loss"][b]) == float(inp["target"][b].double() ** 2)
    assert bool((truth["gx"][sum(inp["sizes"]):] == 0).all()) and bool((truth["gx"][:, :, 1:] == 0).all())


@pytest.mark.parametrize("tag", sorted(G.ATTR_CASES))
def test_type_attr_float32_reference_meets_the_bound(tag):
    for bad in (False, True):
        inp = G.attr_inputs(tag, bad)
        for use in (("node", "edge"), ("node",), ("edge",)):
            if ("node" in use and not inp["S"] and len(use) == 1) or ("edge" in use and not inp["E"] and len(use) == 1):
                continue
            t64, t32 = G.attr_backward(inp, torch.float64, use), G.attr_backward(inp, torch.float32, use)
            G.check(f"{tag}.{use}", t32.double().numpy(), t64.numpy(), t32.double().numpy(), 1.0)
    inp = G.attr_inputs(tag)
    rows, chunk = inp["S"] + inp["E"], G.attr_det_chunk_rows(inp["S"] + inp["E"], inp["K"])
    parts = sum(G.attr_backward(inp, torch.float64, rows=(lo, min(lo + chunk, rows))) for lo in range(0, rows, chunk))
    assert G.relmax(parts.numpy(), G.attr_backward(inp, torch.float64).numpy()) <= 1e-13     # the chunks partition the rows


def test_type_attr_case_table_reaches_what_it_names():
    rows = lambda c: c["S"] + c["E"]
    A = G.ATTR_CASES
    assert A["A1"]["T"] * A["A1"]["K"] == 64 and A["A2"]["T"] * A["A2"]["K"] == 64 and A["A4"]["T"] * A["A4"]["K"] == 63
    assert -(-rows(A["A3"]) // (256 // 64)) == 275 and G.attr_det_chunk_rows(rows(A["A3"]), 64) == 8      # two passes of 4 rows
    assert 256 // 7 == 36 and 256 - 36 * 7 == 4 and A["A4"]["S"] == 0
    assert 256 % A["A5"]["K"] != 0 and A["A5"]["S"] * A["A5"]["K"] > 256


@pytest.mark.parametrize("tag", sorted(G.ROWS_CASES))
def test_simplex_rows_reference_places_the_grades(tag):
    """The reference against the algebra's blade order: every block's features sit on the blades of its grade
    (oracle/tables.py), everything else is 0, and an id outside [0, S) gives the features of row 0."""
    inp = G.rows_inputs(tag)
    out = G.rows_reference(inp)
    alg = G.algebra(inp["n"])
    vpr, ch = inp["verts"].shape[1], 0
    for f, grade in zip(inp["feats"], inp["grades"]):
        K = f.shape[1]
        sl = alg.grade_slices[grade]
        blk = out[:, ch:ch + vpr * K]
        mask = torch.zeros(1 << inp["n"], dtype=torch.bool)
        mask[sl] = True
        assert bool((blk[..., ~mask] == 0).all())
        for r in (0, out.shape[0] - 1):
            for v in range(vpr):
                i = int(inp["verts"][r, v])
                i = i if 0 <= i < inp["S"] else 0
                assert torch.equal(blk[r, v * K:(v + 1) * K][:, sl], f[i])
        ch += vpr * K
    assert ch == out.shape[1]
    if G.ROWS_CASES[tag]["outside"]:
        v = inp["verts"]
        assert int((v < 0).sum()) > 0 and int((v >= inp["S"]).sum()) > 0
