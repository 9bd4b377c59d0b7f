"""The Rips lift on the device (GPU): csmpn_rips_lift against pad_batch(collate([rips_complex(...)]), capacity) on the float64
copy of the same float32 points, exactly; batches that do not fit; SimplicialBatch.relift_ without a host round trip or an
allocation; the md17 model on a re-lifted batch against the host-lifted one, bit for bit; GraphedTrainStep.step(points=...)
against the eager loop."""
import copy

import numpy as np
import pytest
import torch

import det_step_helpers as D
import rips_lift_helpers as R
import varying_helpers as V

pytestmark = pytest.mark.gpu
GUARD = -77


def _dev():
    return torch.device("cuda:0")


def _guarded(shape, dev, pad=64):
    """An int64 tensor of `shape` inside a larger buffer of guard values: (view, whole buffer, offset)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), GUARD, dtype=torch.int64, device=dev)
    return whole[pad:pad + n].view(shape), whole, pad


def _buffers(cap, n_graphs, dev, cols=None):
    S, E, nd = cap.rows, cap.edges, cap.max_dim + 1
    shapes = dict(x_ind=(S, nd if cols is None else cols), node_types=(S,), batch=(S,), x_ind_batch=(S,), ptr=(n_graphs + 1,),
                  x_ind_ptr=(n_graphs + 1,), edge_index=(2, E), edge_types=(E, 2), counts=(nd + 1,))
    return {k: _guarded(s, dev) for k, s in shapes.items()}


def _guards_intact(bufs):
    for k, (view, whole, pad) in bufs.items():
        n = view.numel()
        if not (bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())):
            return k
    return None


def _lift(ops, pts, n_graphs, dis, max_dim, cap, bufs, status, ws=None, edge_types=True, counts=True):
    dev = _dev()
    p = torch.from_numpy(pts).to(dev)
    if ws is None:
        ws = ops.rips_lift_workspace(n_graphs, pts.shape[0] // n_graphs, max_dim, dev)
    v = {k: t[0] for k, t in bufs.items()}
    ops.rips_lift(p, n_graphs, dis, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                  v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"] if edge_types else None,
                  v["counts"] if counts else None, status, ws)
    torch.cuda.synchronize()
    return v


@pytest.mark.parametrize("name", list(R.CASES))
def test_structure_matches_host_lift(pkg, name):
    from csmpn_hip import ops
    pts, dis, max_dim, cap, want = R.reference(name)
    B = R.CASES[name][0]
    bufs = _buffers(cap, B, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts, B, dis, max_dim, cap, bufs, status)
    assert int(status.item()) == 0
    assert R.differences(got, want) == []
    assert _guards_intact(bufs) is None
    if name == "exact_capacity":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    if name == "all_mask_bits_3x64":         # an edge at vertex 0 and one at vertex 63: both ends of the mask are in use
        edges = want["x_ind"][want["node_types"] == 1]
        assert int(edges[:, 0].min()) == 0 and int(edges[:, 1].max()) == 63


def test_wider_x_ind_and_optional_outputs(pkg):
    """x_ind with a spare column (it is zeroed), edge_types = NULL and counts = NULL: their buffers are not touched."""
    from csmpn_hip import ops
    pts, dis, max_dim, cap, want = R.reference("rips_seed2")
    bufs = _buffers(cap, 4, _dev(), cols=4)
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts, 4, dis, max_dim, cap, bufs, status, edge_types=False, counts=False)
    assert int(status.item()) == 0
    wide = torch.zeros(cap.rows, 4, dtype=torch.int64)
    wide[:, :3] = want["x_ind"]
    rest = {k: w for k, w in want.items() if k not in ("x_ind", "edge_types", "counts")}
    assert R.differences(got, rest) == [] and torch.equal(got["x_ind"].cpu(), wide)
    assert bool((bufs["edge_types"][1] == GUARD).all()) and bool((bufs["counts"][1] == GUARD).all())
    assert _guards_intact(bufs) is None


def _short_capacity(kind):
    from csmpn.data.complexes import BatchCapacity
    (rows, edges) = V.RIPS_COUNTS[1]                       # the counts of rips_seed1: (24, 25, 11), 377
    return {"dimension_1": (BatchCapacity((rows[0], rows[1] - 1, rows[2] + 2), edges + 7), 1 << 1),
            "dimension_2": (BatchCapacity((rows[0], rows[1] + 3, rows[2] - 1), edges + 7), 1 << 2),
            "adjacencies": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges - 1), 1 << 3),
            "no_filler_row": (BatchCapacity(rows, edges + 7), 1 << 4)}[kind]


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row"])
def test_batch_that_does_not_fit_changes_nothing(pkg, kind):
    """rips_seed1 at a capacity it misses by one (or, for bit 4, at its exact rows with spare adjacencies) over buffers that
    hold rips_seed4 at that capacity: the bit is set, every buffer keeps every bit, and the next fitting call is served."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    cap, bit = _short_capacity(kind)
    big, dis, max_dim, _, big_want = R.reference("rips_seed1")
    small = R.reference("rips_seed4")[0]
    assert big_want["counts"].tolist() == list(V.RIPS_COUNTS[1][0]) + [V.RIPS_COUNTS[1][1]]
    padded = cx.pad_batch(R.host_lift(small, 4, dis, max_dim), cap)
    want = {k: getattr(padded, k) for k in R.STRUCTURE}
    want["counts"] = R.reference("rips_seed4")[4]["counts"]
    bufs = _buffers(cap, 4, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.rips_lift_workspace(4, 6, max_dim, _dev())
    got = _lift(ops, small, 4, dis, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == 0 and R.differences(got, want) == []
    before = {k: t[1].clone() for k, t in bufs.items()}
    _lift(ops, big, 4, dis, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == bit
    for k, t in bufs.items():
        assert torch.equal(t[1], before[k]), k
    got = _lift(ops, small, 4, dis, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert R.differences(got, want) == [] and _guards_intact(bufs) is None


def _md17_device_batch(cx, case, cap, dev):
    pts, vf, y, _ = case
    return cx.rips_batch_device(torch.from_numpy(pts).to(dev), 4, R.MD17_DIS, cap, features={"y": y},
                                vertex_features=vf)


def _md17_capacity(cx, cases):
    return cx.capacity_of([c[3] for c in cases])


def test_first_batch_over_the_capacity_is_refused(pkg):
    from csmpn.data import complexes as cx
    cases = [R.md17_case(s) for s in (1, 4)]
    cap = cx.capacity_of([cases[1][3]])                    # seed 4 is the smaller complex
    with pytest.raises(ValueError, match="does not fit"):
        _md17_device_batch(cx, cases[0], cap, _dev())


def test_relift_needs_no_host(pkg):
    """The second and third relift_ run with synchronisation made an error and allocate nothing; the batch then holds the
    third point set: structure, features, and every table of plan() and the CSR as a fresh device batch has them."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    cases = [R.md17_case(s) for s in (1, 2, 3)]
    cap = _md17_capacity(cx, cases)
    b = _md17_device_batch(cx, cases[0], cap, dev)
    b.csr().source_order()
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}) for c in cases]
    ptrs = {k: getattr(b, k).data_ptr() for k in b._names}
    b.relift_(on_dev[1][0], R.MD17_DIS, on_dev[1][1])      # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0][0], R.MD17_DIS, on_dev[0][1])
        b.relift_(on_dev[2][0], R.MD17_DIS, on_dev[2][1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {k: getattr(b, k).data_ptr() for k in b._names} == ptrs
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    padded = cx.pad_batch(cases[2][3], cap, R.MD17_VERTEX_FEATURES)
    for k in padded._names:
        if k != "y":                                       # the target is not part of the lift
            assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k
    assert b._plan["lift_counts"].tolist() == R.counts_of(cases[2][3], 2)
    fresh = padded.to(dev)
    plan = fresh.plan(2)
    for d in range(3):
        assert torch.equal(b._plan["rows"][d], plan["rows"][d]) and torch.equal(b._plan["verts"][d], plan["verts"][d]), d
    assert torch.equal(b._plan["graph_of_vertex"], plan["graph_of_vertex"])
    csr = fresh.csr()
    for k in ("perm", "src", "dst", "deg", "row_ptr"):
        assert torch.equal(getattr(b._csr, k), getattr(csr, k)), k
    assert all(torch.equal(x, y) for x, y in zip(b._csr.source_order(), csr.source_order()))
    assert ops.get_csr(b.edge_index, cap.rows) is b._csr


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_md17_model_on_relifted_batch_is_bit_identical(pkg):
    """Deterministic mode as the bit-for-bit step tests set it (torch.use_deterministic_algorithms(True) and
    ops.set_deterministic(True), det_step_helpers.deterministic): loss and every parameter gradient of the md17 model on a
    batch that relift_ built over another complex, and on the host-lifted, padded batch moved to the device - the same bits.
    (With the request alone the torch ops of the model's backward use float atomics: two runs on the SAME host-lifted batch
    then differ in 246 of the 247 gradients by up to 1.9e-7, measured on one MI355X.)"""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    first, second = R.md17_case(3), R.md17_case(1)
    cap = _md17_capacity(cx, [first, second])
    torch.manual_seed(11)
    model_a = M.MD17SimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = _md17_device_batch(cx, first, cap, dev)
        b.relift_(torch.from_numpy(second[0]).to(dev), R.MD17_DIS, {k: v.to(dev) for k, v in second[1].items()})
        b.y.copy_(second[2])
        loss_a, grads_a = _loss_and_grads(model_a, b)
        host = cx.pad_batch(second[3], cap, R.MD17_VERTEX_FEATURES).to(dev)
        loss_b, grads_b = _loss_and_grads(model_b, host)
    assert int(b._plan["lift_status"].item()) == 0
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def test_graphed_step_on_device_lifted_points_matches_eager(pkg):
    """Eight Adam steps over four point sets: the eager loop on the unpadded host-lifted batches against ONE captured step
    fed with step(points=...), within the 1e-3 of test_graphed_train_step_matches_eager."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    cases = [R.md17_case(s) for s in (1, 2, 3, 4)]
    torch.manual_seed(7)
    model_e = M.MD17SimplicialMPNN().to(dev)
    model_g = copy.deepcopy(model_e)
    opt_e = torch.optim.Adam(model_e.parameters(), lr=1e-3)
    opt_g = torch.optim.Adam(model_g.parameters(), lr=1e-3, capturable=True)
    eager, graphed = [], []
    for step in range(8):
        loss, _ = model_e(cases[step % 4][3].to(dev))
        opt_e.zero_grad(set_to_none=True)
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    cap = _md17_capacity(cx, cases)
    gs = GraphedTrainStep(model_g, opt_g, cases[0][3], ["loc", "vel", "charges", "y"], capacity=cap, rips_dis=R.MD17_DIS)
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}, c[2].to(dev)) for c in cases]
    for step in range(8):
        pts, vf, y = on_dev[step % 4]
        graphed.append(float(gs.step(features={"y": y}, points=pts, vertex_features=vf).detach()))
    assert gs.status() == 0
    eager, graphed = np.asarray(eager), np.asarray(graphed)
    print("eager", eager, "graphed", graphed)
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
    with pytest.raises(ValueError):
        gs.step(points=on_dev[0][0], batch=cases[0][3])
