"""The convex-hull lift on the device (GPU): csmpn_hull_lift against
pad_batch(collate([hull_complex(..., method="exact")]), capacity) on the float64 copy of the same float32 points, exactly, on
the smallest shapes that reach each part of lift_hull_kernel<2..5> and of the scatter with the facet table; the volumes
against hull_facets' double values and over two calls; batches that do not fit; SimplicialBatch.relift_(points, hull=True)
without a host round trip or an allocation; the hulls model on a re-lifted batch against the host-lifted one, bit for bit;
GraphedTrainStep.step(points=..., hull=True) against the eager loop."""
import copy

import numpy as np
import pytest
import torch

import det_step_helpers as D
import hull_lift_helpers as H

pytestmark = pytest.mark.gpu

VOLUME_GUARD = -77.0


def _dev():
    return torch.device("cuda:0")


def _volume_buffer(n_graphs, pad=64):
    whole = torch.full((n_graphs + 2 * pad,), VOLUME_GUARD, dtype=torch.float32, device=_dev())
    return whole[pad:pad + n_graphs], whole


def _volume_guards_intact(view, whole, pad=64):
    return bool((whole[:pad] == VOLUME_GUARD).all()) and bool((whole[pad + view.numel():] == VOLUME_GUARD).all())


def _lift(ops, pts, n_graphs, max_dim, cap, bufs, status, volume, ws=None):
    dev = _dev()
    p = torch.from_numpy(pts).to(dev)
    if ws is None:
        ws = ops.hull_lift_workspace(n_graphs, pts.shape[0] // n_graphs, max_dim, dev)
    v = {key: t[0] for key, t in bufs.items()}
    ops.hull_lift(p, n_graphs, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                  v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws, volume=volume)
    torch.cuda.synchronize()
    return v


def _within_one_spacing(got32, want64):
    """Every float32 volume within one float32 spacing of the host form's double value."""
    got = np.asarray(got32, dtype=np.float32)
    return bool(np.all(np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(got)).astype(np.float64)))


@pytest.mark.parametrize("name", list(H.CASES))
def test_structure_and_volume_match_host(pkg, name):
    from csmpn_hip import ops
    pts, max_dim, cap, want, volumes = H.reference(name)
    B = H.CASES[name][0]
    bufs = H.buffers(cap, B, _dev())
    vol, vol_whole = _volume_buffer(B)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts, B, max_dim, cap, bufs, status, vol)
    assert int(status.item()) == 0
    assert H.differences(got, want) == []
    assert H.guards_intact(bufs) is None and _volume_guards_intact(vol, vol_whole)
    first = vol.cpu().numpy().copy()
    assert _within_one_spacing(first, volumes), (first, volumes)
    vol.fill_(VOLUME_GUARD)
    _lift(ops, pts, B, max_dim, cap, bufs, status, vol)                   # the same bits over two calls
    assert np.array_equal(vol.cpu().numpy().view(np.uint32), first.view(np.uint32))
    if name == "exact_capacity_3x8_r5":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    if name == "task_3x8_r5":                                              # a NULL volume is accepted
        _lift(ops, pts, B, max_dim, cap, bufs, status, None)
        assert int(status.item()) == 0 and H.differences(got, want) == []


def _short_capacity(kind, rows, edges):
    from csmpn.data.complexes import BatchCapacity
    return {"dimension_1": (BatchCapacity((rows[0], rows[1] - 1, rows[2] + 2), edges + 7), 1 << 1),
            "dimension_2": (BatchCapacity((rows[0], rows[1] + 3, rows[2] - 1), edges + 7), 1 << 2),
            "adjacencies": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges - 1), 1 << 3),
            "no_filler_row": (BatchCapacity(tuple(rows), edges + 7), 1 << 4)}[kind]


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row"])
def test_batch_that_does_not_fit_changes_nothing(pkg, kind):
    """4 x 6 points in R^3 at a capacity they miss by one (or, for bit 4, at their exact rows with spare adjacencies) over
    buffers that hold other points (vertex 4 inside: a smaller hull) at that capacity: the bit is set, every buffer - the
    volumes included - keeps every bit, and the next fitting call is served."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    big, small = H.make_points("normal", 21, 4, 6, 3), H.make_points("interior", 22, 4, 6, 3)
    big_counts = H.counts_of(H.host_lift(big, 4, 2), 2)
    small_raw = H.host_lift(small, 4, 2)
    small_counts = H.counts_of(small_raw, 2)
    assert small_counts[1] < big_counts[1] - 1 and small_counts[2] < big_counts[2] - 1 and small_counts[3] < big_counts[3] - 1
    cap, bit = _short_capacity(kind, big_counts[:3], big_counts[3])
    padded = cx.pad_batch(small_raw, cap)
    want = {key: getattr(padded, key) for key in H.STRUCTURE}
    want["counts"] = torch.tensor(small_counts, dtype=torch.int64)
    bufs = H.buffers(cap, 4, _dev())
    vol, vol_whole = _volume_buffer(4)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.hull_lift_workspace(4, 6, 2, _dev())
    got = _lift(ops, small, 4, 2, cap, bufs, status, vol, ws)
    assert int(status.item()) == 0 and H.differences(got, want) == []
    assert _within_one_spacing(vol.cpu().numpy(), H.host_volumes(small, 4))
    before = {key: t[1].clone() for key, t in bufs.items()}
    vol_before = vol_whole.clone()
    _lift(ops, big, 4, 2, cap, bufs, status, vol, ws)
    assert int(status.item()) == bit
    for key, t in bufs.items():
        assert torch.equal(t[1], before[key]), key
    assert torch.equal(vol_whole.view(torch.int32), vol_before.view(torch.int32))
    got = _lift(ops, small, 4, 2, cap, bufs, status, vol, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert H.differences(got, want) == [] and H.guards_intact(bufs) is None
    assert torch.equal(vol_whole.view(torch.int32), vol_before.view(torch.int32))


def test_first_batch_over_the_capacity_is_refused(pkg):
    from csmpn.data import complexes as cx
    pts, raw = H.hulls_case(1)
    c = H.counts_of(raw, 2)
    cap = cx.BatchCapacity((c[0], c[1] - 1, c[2]), c[3])
    with pytest.raises(ValueError, match="does not fit"):
        cx.hull_batch_device(torch.from_numpy(pts).to(_dev()), 4, cap)


def test_relift_needs_no_host(pkg):
    """The second and third relift_(points, hull=True) run with synchronisation made an error and allocate nothing; the batch
    then holds the third point set: structure, `input`, `target` (the device's volumes), and every table of plan() and the
    CSR as a fresh device batch has them."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    cases = [H.hulls_case(s) for s in (1, 2, 3)]
    cap = cx.capacity_of([c[1] for c in cases])
    on_dev = [torch.from_numpy(c[0]).to(dev) for c in cases]
    b = cx.hull_batch_device(on_dev[0], 4, cap)
    first = cx.pad_batch(cases[0][1], cap, ("input",))
    for k in first._names:
        if k != "target":
            assert torch.equal(getattr(b, k).cpu(), getattr(first, k)), k
    assert _within_one_spacing(b.target.cpu().numpy(), H.host_volumes(cases[0][0], 4))
    b.csr().source_order()
    ptrs = {k: getattr(b, k).data_ptr() for k in b._names}
    b.relift_(on_dev[1], hull=True)                        # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0], hull=True)
        b.relift_(on_dev[2], None, None, None, True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {k: getattr(b, k).data_ptr() for k in b._names} == ptrs
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    padded = cx.pad_batch(cases[2][1], cap, ("input",))
    assert sorted(padded._names) == sorted(b._names)
    for k in padded._names:
        if k != "target":
            assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k
    assert _within_one_spacing(b.target.cpu().numpy(), H.host_volumes(cases[2][0], 4))
    assert b._plan["lift_counts"].tolist() == H.counts_of(cases[2][1], 2)
    fresh = padded.to(dev)
    plan = fresh.plan(2)
    for d in range(3):
        assert torch.equal(b._plan["rows"][d], plan["rows"][d]) and torch.equal(b._plan["verts"][d], plan["verts"][d]), d
    assert torch.equal(b._plan["graph_of_vertex"], plan["graph_of_vertex"])
    csr = fresh.csr()
    for k in ("perm", "src", "dst", "deg", "row_ptr"):
        assert torch.equal(getattr(b._csr, k), getattr(csr, k)), k
    assert ops.get_csr(b.edge_index, cap.rows) is b._csr
    with pytest.raises(ValueError, match="exactly one"):
        b.relift_(on_dev[0], 1.6, hull=True)
    # one workspace serves all three lifts: the same batch takes a Rips and a kNN lift of other points (R^3, 8 per graph)
    assert b._plan["lift_ws"].numel() >= ops.hull_lift_workspace(4, 8, 2, dev).numel()


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_hulls_model_on_relifted_batch_is_bit_identical(pkg):
    """Deterministic mode as the bit-for-bit step tests set it: loss and every parameter gradient of the hulls model on a
    batch that relift_(hull=True) built over another complex, and on the host-lifted, padded batch moved to the device with
    the device's volumes as its targets (the comparison isolates the structure) - the same bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    first, second = H.hulls_case(3), H.hulls_case(1)
    cap = cx.capacity_of([first[1], second[1]])
    torch.manual_seed(11)
    model_a = M.HullsSimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = cx.hull_batch_device(torch.from_numpy(first[0]).to(dev), 4, cap)
        b.relift_(torch.from_numpy(second[0]).to(dev), hull=True)
        loss_a, grads_a = _loss_and_grads(model_a, b)
        host = cx.pad_batch(second[1], cap, ("input",)).to(dev)
        assert _within_one_spacing(b.target.cpu().numpy(), H.host_volumes(second[0], 4))
        host.target.copy_(b.target)
        loss_b, grads_b = _loss_and_grads(model_b, host)
    assert int(b._plan["lift_status"].item()) == 0
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def _eager_and_graphed_losses(cases, dev):
    """Eight Adam steps over the four point sets: (losses of the eager loop on the unpadded host-lifted batches, losses of ONE
    captured step fed with step(points=..., hull=True) - the choice once as the step's default and once in the call -, the
    two models, the step)."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    torch.manual_seed(7)
    model_e = M.HullsSimplicialMPNN().to(dev)
    model_g = copy.deepcopy(model_e)
    opt_e = torch.optim.Adam(model_e.parameters(), lr=1e-3)
    opt_g = torch.optim.Adam(model_g.parameters(), lr=1e-3, capturable=True)
    eager, graphed = [], []
    for step in range(8):
        loss, _ = model_e(cases[step % 4][1].to(dev))
        opt_e.zero_grad(set_to_none=True)
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    cap = cx.capacity_of([c[1] for c in cases])
    gs = GraphedTrainStep(model_g, opt_g, cases[0][1], ["input", "target"], capacity=cap, hull=True)
    on_dev = [torch.from_numpy(c[0]).to(dev) for c in cases]
    for step in range(8):
        how = {} if step % 2 else {"hull": True}
        graphed.append(float(gs.step(points=on_dev[step % 4], **how).detach()))
    return np.asarray(eager), np.asarray(graphed), model_e, model_g, gs, on_dev


def test_graphed_step_on_device_lifted_points_matches_eager(pkg):
    """Eight Adam steps over four point sets, the eager loop on the unpadded host-lifted batches against ONE captured step fed
    with nothing but step(points=..., hull=True), within the 1e-3 of test_graphed_train_step_matches_eager: on the default
    (atomic) path the eight losses and status() == 0; in deterministic mode the losses AND every parameter with its floor of
    1e-2 (tests/test_knn_lift_gpu.py says why the parameters are compared there alone)."""
    dev = _dev()
    cases = [H.hulls_case(s) for s in (1, 2, 3, 4)]
    eager, graphed, _, _, gs, _ = _eager_and_graphed_losses(cases, dev)
    assert gs.status() == 0
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    with D.deterministic(torch_flag=True, request=True):
        eager, graphed, model_e, model_g, gs, on_dev = _eager_and_graphed_losses(cases, dev)
    assert gs.status() == 0
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
    with pytest.raises(ValueError):
        gs.step(points=on_dev[0], dis=1.6, hull=True)
