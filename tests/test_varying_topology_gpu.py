"""Replaying the captured training step on batches of changing topology (GPU): the per-batch index tables built on the
device (csmpn_simplex_tables) against SimplicialBatch.plan(), the in-place CSR rebuild against a fresh CSR, the in-place
refresh of a whole batch, the four task models on the padded forms of their reference fixtures, the isolation of the filler
rows, and GraphedTrainStep(capacity=...) against the eager loop over unpadded batches."""
import copy
import os

import numpy as np
import pytest
import torch

import test_model_harness as H
import varying_helpers as V

pytestmark = pytest.mark.gpu
GUARD = -77


def _dev():
    return torch.device("cuda:0")


def _table_cases(pkg, name):
    """(padded CPU batch, max_dim)."""
    from csmpn.data import complexes as cx
    if name == "rips":                       # the Rips batch of the CPU tests at the capacity of seeds 1..4
        bs = [V.rips_batch(s) for s in V.RIPS_COUNTS]
        return cx.pad_batch(bs[0], cx.capacity_of(bs)), 2
    if name == "many_workgroups":            # ~1 200 rows: the scan crosses several workgroups of 256 rows
        b = V.rips_batch(11, n_graphs=40, points=8, dis=2.0)
        assert b.node_types.shape[0] > 4 * 256
        return cx.pad_batch(b, cx.capacity_of([b], slack=0.1)), 2
    if name == "max_dim_3":                  # the 4-simplex's faces up to tetrahedra: 24 vertex orders
        x_dict, adj = cx.lift(5, [(0, 1, 2, 3, 4)], 3)
        b = cx.collate([cx.to_complex(5, x_dict, adj, 3) for _ in range(3)])
        rows, edges = V.counts_of(b, 3)
        return cx.pad_batch(b, cx.BatchCapacity((rows[0], rows[1] + 2, rows[2] + 1, rows[3] + 3), edges + 9)), 3
    b = V.rips_batch(5, dis=1e-3)            # no two points that close: vertices only
    rows, edges = V.counts_of(b)
    assert rows[1:] == (0, 0)
    if name == "dimension_of_fillers_only":
        return cx.pad_batch(b, cx.BatchCapacity((rows[0], 3, 2), edges + 4)), 2
    assert name == "empty_dimension"         # n_2 = 0
    return cx.pad_batch(b, cx.BatchCapacity((rows[0], 2, 0), edges + 1)), 2


def _guarded(shape, dtype, dev, pad=16):
    """A tensor of `shape` inside a larger buffer of guard values: (view, whole buffer, offset)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), GUARD, dtype=dtype, device=dev)
    return whole[pad:pad + n].view(shape), whole, pad


def _outside_untouched(whole, pad, n):
    return bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())


def _run_tables(ops, b, max_dim, counts, status):
    """csmpn_simplex_tables on device batch b into guarded buffers of the given row counts."""
    dev = b.x_ind.device
    fact = [1, 2, 6, 24]
    bufs = {"rows": [_guarded((counts[d],), torch.int64, dev) for d in range(max_dim + 1)],
            "verts": [_guarded((counts[d] * fact[d], d + 1), torch.int64, dev) for d in range(max_dim + 1)],
            "verts_i32": [_guarded((counts[d] * fact[d], d + 1), torch.int32, dev) for d in range(max_dim + 1)],
            "graph_of_vertex": _guarded((counts[0],), torch.int64, dev),
            "vertices_per_graph": _guarded((b.num_graphs,), torch.int64, dev),
            "types_i32": _guarded((b.node_types.shape[0],), torch.int32, dev)}
    ws = ops.simplex_tables_workspace(b.node_types.shape[0], max_dim, dev)
    ops.simplex_tables(b.x_ind, b.node_types, b.x_ind_batch, b.x_ind_ptr, max_dim, [t[0] for t in bufs["rows"]],
                       [t[0] for t in bufs["verts"]], [t[0] for t in bufs["verts_i32"]], bufs["graph_of_vertex"][0],
                       bufs["vertices_per_graph"][0], bufs["types_i32"][0], status, ws)
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("case", ["rips", "many_workgroups", "max_dim_3", "dimension_of_fillers_only", "empty_dimension"])
def test_simplex_tables_match_plan(pkg, case):
    from csmpn_hip import ops
    padded, max_dim = _table_cases(pkg, case)
    b = padded.to(_dev())
    plan = b.plan(max_dim)
    counts = [int(r.shape[0]) for r in plan["rows"]]
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _run_tables(ops, b, max_dim, counts, status)
    assert int(status.item()) == 0
    for d in range(max_dim + 1):
        assert torch.equal(got["rows"][d][0], plan["rows"][d]), d
        assert torch.equal(got["verts"][d][0], plan["verts"][d]), d
        assert torch.equal(got["verts_i32"][d][0], plan["verts"][d].to(torch.int32)), d     # the models' lazy verts_i32
        for k in ("rows", "verts", "verts_i32"):
            view, whole, pad = got[k][d]
            assert _outside_untouched(whole, pad, view.numel()), (k, d)
    assert torch.equal(got["graph_of_vertex"][0], plan["graph_of_vertex"])
    assert torch.equal(got["vertices_per_graph"][0], plan["vertices_per_graph"])
    assert torch.equal(got["types_i32"][0], b.node_types.to(torch.int32))                   # the models' lazy types_i32
    for k in ("graph_of_vertex", "vertices_per_graph", "types_i32"):
        view, whole, pad = got[k]
        assert _outside_untouched(whole, pad, view.numel()), k


def test_simplex_tables_refuse_max_dim_4(pkg):
    from csmpn_hip import native, ops
    dev = _dev()
    b = V.rips_batch(1).to(dev)
    S, B = b.node_types.shape[0], b.num_graphs
    x5 = torch.zeros(S, 5, dtype=torch.int64, device=dev)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)
    assert native.lib().csmpn_simplex_tables_workspace_bytes(S, 4) == 0
    assert native.lib().csmpn_simplex_tables_workspace_bytes(S, 3) > 0
    with pytest.raises(native.CsmpnError, match=f"error {native.ERR_UNSUPPORTED}:"):
        ops.simplex_tables(x5, b.node_types, b.x_ind_batch, b.x_ind_ptr, 4, [i64(4) for _ in range(5)],
                           [i64(4, d + 1) for d in range(5)], None, i64(4), i64(B), None, None,
                           ops.simplex_tables_workspace(S, 3, dev))


def test_simplex_tables_wrong_expected_count(pkg):
    """More rows of a type than expected: nothing is written past the buffer; fewer: the tail keeps its contents; both set
    the dimension's status bit, and the device goes on working."""
    from csmpn_hip import ops
    padded, max_dim = _table_cases(pkg, "rips")
    b = padded.to(_dev())
    plan = b.plan(2)
    n = [int(r.shape[0]) for r in plan["rows"]]
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    wrong = [n[0], n[1] - 2, n[2] + 3]
    got = _run_tables(ops, b, 2, wrong, status)
    assert int(status.item()) == (1 << 1) | (1 << 2)
    for k in ("rows", "verts", "verts_i32"):
        for d in range(3):
            view, whole, pad = got[k][d]
            assert _outside_untouched(whole, pad, view.numel()), (k, d)
    assert torch.equal(got["rows"][0][0], plan["rows"][0]) and torch.equal(got["verts"][0][0], plan["verts"][0])
    assert torch.equal(got["rows"][1][0], plan["rows"][1][:n[1] - 2]) and torch.equal(got["verts"][1][0], plan["verts"][1][:2 * (n[1] - 2)])
    assert torch.equal(got["rows"][2][0][:n[2]], plan["rows"][2]) and bool((got["rows"][2][0][n[2]:] == GUARD).all())
    assert torch.equal(got["verts"][2][0][:6 * n[2]], plan["verts"][2]) and bool((got["verts"][2][0][6 * n[2]:] == GUARD).all())
    # the status word is sticky and the next, correct, call is served
    again = _run_tables(ops, b, 2, n, status)
    assert int(status.item()) == (1 << 1) | (1 << 2)
    assert all(torch.equal(again["rows"][d][0], plan["rows"][d]) and torch.equal(again["verts"][d][0], plan["verts"][d]) for d in range(3))


def test_csr_rebuild_in_place(pkg):
    from csmpn_hip import ops
    dev = _dev()
    g = torch.Generator().manual_seed(5)
    N, E = 157, 3001
    ei_a = torch.randint(0, N, (2, E), generator=g).to(dev)
    ei_b = torch.randint(0, N, (2, E), generator=g)
    ei_b[1, :900] = 3                                         # a hub
    ei_b = ei_b.to(dev)
    csr = ops.Csr(ei_a, N)
    csr.source_order()
    tensors = lambda c: [c.perm, c.src, c.dst, c.deg, c.row_ptr, *c.source_order()]
    ptrs = [t.data_ptr() for t in tensors(csr)]
    assert csr.rebuild_(ei_b) is csr
    fresh = ops.Csr(ei_b, N)
    for a, b in zip(tensors(csr), tensors(fresh)):
        assert torch.equal(a, b)
    assert [t.data_ptr() for t in tensors(csr)] == ptrs
    assert ops.get_csr(ei_b, N) is csr                        # re-stamped on the tensor
    ws = csr._ws.data_ptr()
    csr.rebuild_(ei_a)                                        # the workspace is kept from the first rebuild on
    assert csr._ws.data_ptr() == ws and torch.equal(csr.src, ops.Csr(ei_a, N).src)
    with pytest.raises(RuntimeError):
        csr.rebuild_(ei_b[:, :-1].contiguous())


def _with_lazy_tables(batch, form):
    """plan(), csr() and every table the models add lazily, through the models' own builders."""
    from csmpn.models import simplicial_mpnn as M
    plan = batch.plan(2)
    batch.csr().source_order()
    S, B = int(batch.node_types.shape[0]), batch.num_graphs
    batch.lazy_table(plan, "verts_i32", M._verts_i32_builder(plan, S))
    batch.lazy_table(plan, "types_i32", M._types_i32_builder(batch, 3))
    batch.lazy_table(plan, "ei_i32", M._ei_i32_builder(batch))
    batch.lazy_table(plan, "ptr_i32", M._ptr_i32_builder(batch))
    kw = {"md17": {}, "motion": dict(vertex_rows=plan["vertex_rows"], n_rows=S),
          "nba": dict(vertex_rows=plan["vertex_rows"], n_rows=S, unscored_last=1)}[form]
    batch.lazy_table(plan, "traj", M._traj_builder(plan, B, **kw))
    return plan


def _flat_tables(batch):
    plan, csr = batch._plan, batch._csr
    out = {f"rows{d}": t for d, t in enumerate(plan["rows"])}
    out.update({f"verts{d}": t for d, t in enumerate(plan["verts"])})
    out.update({f"verts_i32_{d}": t for d, t in enumerate(plan["verts_i32"])})
    out.update(graph_of_vertex=plan["graph_of_vertex"], vertices_per_graph=plan["vertices_per_graph"],
               types_i32=plan["types_i32"], ei_src=plan["ei_i32"][0], ei_dst=plan["ei_i32"][1], ptr_i32=plan["ptr_i32"])
    out.update({f"traj_{k}": t for k, t in plan["traj"].items() if t is not None})
    out.update(perm=csr.perm, src=csr.src, dst=csr.dst, deg=csr.deg, row_ptr=csr.row_ptr,
               src_row_ptr=csr.source_order()[0], src_order=csr.source_order()[1])
    out.update({k: getattr(batch, k) for k in batch._names})
    return out


@pytest.mark.parametrize("form", ["md17", "motion", "nba"])
def test_refresh_rebuilds_every_table_in_place(pkg, form):
    """SimplicialBatch.refresh_ onto a batch of another topology: every tensor and table equals that of a fresh device
    batch, at the address it had before - the three forms of the trajectory-readout tables included - and, from
    device-resident raw tensors, without a host round trip."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    raws = [V.rips_batch(s, md17=True) for s in (1, 2)]
    cap = cx.capacity_of(raws)
    feats = V.SIMPLEX_FEATURES["md17"]
    a = cx.pad_batch(raws[0], cap, feats).to(dev)
    _with_lazy_tables(a, form)
    before = {k: t.data_ptr() for k, t in _flat_tables(a).items()}
    nxt = cx.pad_batch(raws[1], cap, feats)
    assert a.refresh_(nxt) is a
    fresh = nxt.to(dev)
    _with_lazy_tables(fresh, form)
    got, want = _flat_tables(a), _flat_tables(fresh)
    assert sorted(got) == sorted(want) and ("traj_trow" in got) == (form == "nba") and ("traj_vrows" in got) == (form != "md17")
    for k in want:
        assert torch.equal(got[k], want[k]), k
        assert got[k].data_ptr() == before[k], k
    assert int(a._plan["status"].item()) == 0 and (a.n_real_rows, a.n_real_edges) == (nxt.n_real_rows, nxt.n_real_edges)
    assert ops.get_csr(a.edge_index, int(a.node_types.shape[0])) is a._csr
    # no host round trip: back onto the first batch, from raw tensors that live on the device
    back = cx.pad_batch(raws[0], cap, feats).to(dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a.refresh_(back)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    first = cx.pad_batch(raws[0], cap, feats).to(dev)
    _with_lazy_tables(first, form)
    want = _flat_tables(first)
    got = _flat_tables(a)
    assert all(torch.equal(got[k], want[k]) for k in want)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("kind", ["md17", "hulls", "motion", "nba"])
def test_padded_model_fixture_gpu(pkg, kind, deterministic):
    """The reference fixture of every task model on its fixture batch padded with 3 spare 1-simplices, 2 spare 2-simplices
    and 7 spare adjacencies, at the tolerances of test_model_fixture_gpu."""
    from csmpn_hip import ops
    dev = _dev()
    g = np.load(os.path.join(H.GOLD, f"model_{kind}.npz"))
    batch = V.padded_fixture(kind, H.load_batch(pkg, g)).to(dev)
    ops.set_deterministic(True if deterministic else None)
    try:
        model = H.build(pkg, kind, g, dev)
        loss, parts = model(batch)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(None)
    H._check_against_fixture(g, loss, parts, model, tol=3e-5 if kind == "nba" else 1e-5)


@pytest.mark.parametrize("kind", ["md17", "hulls", "motion", "nba"])
def test_filler_rows_are_isolated(pkg, kind):
    """Deterministic mode, the same padded batch with zero and with random normal filler features: loss, loss parts and
    every parameter gradient bit for bit - the filler rows get exactly zero upstream gradient and nothing real reads them;
    shapes, and with them the summation orders, are the same."""
    from csmpn_hip import ops
    dev = _dev()
    g = np.load(os.path.join(H.GOLD, f"model_{kind}.npz"))
    padded = V.padded_fixture(kind, H.load_batch(pkg, g))
    from csmpn.data.complexes import SimplicialBatch
    tensors = {k: getattr(padded, k).clone() for k in padded._names}
    gen = torch.Generator().manual_seed(1)
    for k in V.SIMPLEX_FEATURES[kind]:
        tensors[k][padded.n_real_rows:] = torch.randn(tensors[k][padded.n_real_rows:].shape, generator=gen)
        assert float(tensors[k][padded.n_real_rows:].abs().max()) > 0.5
    noisy = SimplicialBatch(**tensors)
    results = []
    ops.set_deterministic(True)
    try:
        for b in (padded, noisy):
            model = H.build(pkg, kind, g, dev)
            loss, parts = model(b.to(dev))
            loss.backward()
            torch.cuda.synchronize()
            results.append((loss.detach(), {k: v.detach() for k, v in parts.items()},
                            {k: p.grad for k, p in model.named_parameters() if p.grad is not None}))
    finally:
        ops.set_deterministic(None)
    (la, pa, ga), (lb, pb, gb) = results
    assert torch.equal(la, lb) and sorted(pa) == sorted(pb) and sorted(ga) == sorted(gb) and len(ga) > 20
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k


def _replay_case(pkg, kind):
    from csmpn.models import simplicial_mpnn as M
    if kind == "md17":
        return M.MD17SimplicialMPNN(), [V.rips_batch(s, md17=True) for s in (1, 2, 3, 4)], ["loc", "vel", "charges", "y"], \
            V.rips_batch(1, dis=3.0, md17=True)
    return M.HullsSimplicialMPNN(hidden_features=28, num_layers=3), [H._hull_batch(pkg, s) for s in (9, 10, 9, 10)], \
        ["input", "target"], H._hull_batch(pkg, 9, n_graphs=5)


@pytest.mark.parametrize("kind", ["md17", "hulls"])
def test_graphed_step_on_changing_topology_matches_eager(pkg, kind):
    """Eight Adam steps over four batches of different topology: the eager loop on the unpadded batches (a fresh device
    batch per step) against ONE captured step replayed on the padded ones - the bound of
    test_graphed_train_step_matches_eager (1e-3 relative) on the losses and the final parameters."""
    from csmpn.data import complexes as cx
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    torch.manual_seed(7)
    model_e, batches, features, too_large = _replay_case(pkg, kind)
    model_e = model_e.to(dev)
    model_g = copy.deepcopy(model_e)
    opt_e = torch.optim.Adam(model_e.parameters(), lr=1e-3)
    opt_g = torch.optim.Adam(model_g.parameters(), lr=1e-3, capturable=True)
    eager, graphed = [], []
    for step in range(8):
        loss, _ = model_e(batches[step % 4].to(dev))
        opt_e.zero_grad(set_to_none=True)
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    cap = cx.capacity_of(batches)
    gs = GraphedTrainStep(model_g, opt_g, batches[0], features, capacity=cap)
    for step in range(8):
        if step == 5:      # a batch over the capacity: refused before anything is launched, and the step goes on working
            with pytest.raises(ValueError):
                gs.step(batch=too_large)
        graphed.append(float(gs.step(batch=batches[step % 4]).detach()))
    assert gs.status() == 0
    eager, graphed = np.asarray(eager), np.asarray(graphed)
    print(kind, "eager", eager, "graphed", graphed)
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    worst = max(float((pe - pg).detach().abs().max()) / max(float(pe.detach().abs().max()), 1e-2)
                for pe, pg in zip(model_e.parameters(), model_g.parameters()))
    print(kind, "worst relative parameter difference", worst)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
