"""The k-nearest-neighbour clique lift on the device (GPU): csmpn_knn_lift against
pad_batch(collate([knn_clique_complex(...)]), capacity) on the float64 copy of the same float32 points, exactly, on the
smallest shapes that reach each part of lift_knn_kernel and of the scatter without the vertex block; batches that do not
fit; SimplicialBatch.relift_(points, knn=k) without a host round trip or an allocation; the md17 model on a re-lifted batch
against the host-lifted one, bit for bit; GraphedTrainStep.step(points=..., knn=k) against the eager loop; the Rips and the
kNN entry on one complete graph."""
import copy

import numpy as np
import pytest
import torch

import det_step_helpers as D
import knn_lift_helpers as K

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _lift(ops, pts, n_graphs, k, max_dim, cap, bufs, status, ws=None):
    dev = _dev()
    p = torch.from_numpy(pts).to(dev)
    if ws is None:
        ws = ops.knn_lift_workspace(n_graphs, pts.shape[0] // n_graphs, max_dim, dev)
    v = {key: t[0] for key, t in bufs.items()}
    ops.knn_lift(p, n_graphs, k, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                 v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws)
    torch.cuda.synchronize()
    return v


@pytest.mark.parametrize("name", list(K.CASES))
def test_structure_matches_host_lift(pkg, name):
    from csmpn_hip import ops
    pts, k, max_dim, cap, want = K.reference(name)
    B = K.CASES[name][0]
    bufs = K.buffers(cap, B, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts, B, k, max_dim, cap, bufs, status)
    assert int(status.item()) == 0
    assert K.differences(got, want) == []
    assert K.guards_intact(bufs) is None
    if name == "exact_capacity_16x21":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]


def _short_capacity(kind, rows, edges):
    from csmpn.data.complexes import BatchCapacity
    return {"dimension_1": (BatchCapacity((rows[0], rows[1] - 1, rows[2] + 2), edges + 7), 1 << 1),
            "dimension_2": (BatchCapacity((rows[0], rows[1] + 3, rows[2] - 1), edges + 7), 1 << 2),
            "adjacencies": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges - 1), 1 << 3),
            "no_filler_row": (BatchCapacity(tuple(rows), edges + 7), 1 << 4)}[kind]


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row"])
def test_batch_that_does_not_fit_changes_nothing(pkg, kind):
    """4 x 6 points at k = 3 at a capacity they miss by one (or, for bit 4, at their exact rows with spare adjacencies) over
    buffers that hold other points at k = 2 at that capacity: the bit is set, every buffer keeps every bit, and the next
    fitting call is served."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    big, small = K.make_points("normal", 21, 4, 6, 3), K.make_points("normal", 22, 4, 6, 3)
    big_counts = K.counts_of(K.host_lift(big, 4, 3, 2), 2)
    small_raw = K.host_lift(small, 4, 2, 2)
    small_counts = K.counts_of(small_raw, 2)
    assert small_counts[1] < big_counts[1] - 1 and small_counts[2] < big_counts[2] - 1 and small_counts[3] < big_counts[3] - 1
    cap, bit = _short_capacity(kind, big_counts[:3], big_counts[3])
    padded = cx.pad_batch(small_raw, cap)
    want = {key: getattr(padded, key) for key in K.STRUCTURE}
    want["counts"] = torch.tensor(small_counts, dtype=torch.int64)
    bufs = K.buffers(cap, 4, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.knn_lift_workspace(4, 6, 2, _dev())
    got = _lift(ops, small, 4, 2, 2, cap, bufs, status, ws)
    assert int(status.item()) == 0 and K.differences(got, want) == []
    before = {key: t[1].clone() for key, t in bufs.items()}
    _lift(ops, big, 4, 3, 2, cap, bufs, status, ws)
    assert int(status.item()) == bit
    for key, t in bufs.items():
        assert torch.equal(t[1], before[key]), key
    got = _lift(ops, small, 4, 2, 2, cap, bufs, status, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert K.differences(got, want) == [] and K.guards_intact(bufs) is None


def _md17_device_batch(cx, case, cap, dev):
    pts, vf, y, _ = case
    return cx.knn_batch_device(torch.from_numpy(pts).to(dev), 4, K.MD17_K, cap, features={"y": y}, vertex_features=vf)


def test_first_batch_over_the_capacity_is_refused(pkg):
    from csmpn.data import complexes as cx
    case = K.md17_case(1)
    c = K.counts_of(case[3], 2)
    cap = cx.BatchCapacity((c[0], c[1] - 1, c[2]), c[3])
    with pytest.raises(ValueError, match="does not fit"):
        _md17_device_batch(cx, case, cap, _dev())


def test_relift_needs_no_host(pkg):
    """The second and third relift_(points, knn=3) run with synchronisation made an error and allocate nothing; the batch
    then holds the third point set: structure, features, and every table of plan() and the CSR as a fresh device batch has
    them."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    cases = [K.md17_case(s) for s in (1, 2, 3)]
    cap = cx.capacity_of([c[3] for c in cases])
    b = _md17_device_batch(cx, cases[0], cap, dev)
    b.csr().source_order()
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}) for c in cases]
    ptrs = {k: getattr(b, k).data_ptr() for k in b._names}
    b.relift_(on_dev[1][0], vertex_features=on_dev[1][1], knn=K.MD17_K)      # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0][0], None, on_dev[0][1], knn=K.MD17_K)
        b.relift_(on_dev[2][0], knn=K.MD17_K, vertex_features=on_dev[2][1])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {k: getattr(b, k).data_ptr() for k in b._names} == ptrs
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    padded = cx.pad_batch(cases[2][3], cap, K.MD17_VERTEX_FEATURES)
    for k in padded._names:
        if k != "y":                                       # the target is not part of the lift
            assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k
    assert b._plan["lift_counts"].tolist() == K.counts_of(cases[2][3], 2)
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
        b.relift_(on_dev[0][0], 1.6, on_dev[0][1], knn=K.MD17_K)


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_md17_model_on_relifted_batch_is_bit_identical(pkg):
    """Deterministic mode as the bit-for-bit step tests set it (torch.use_deterministic_algorithms(True) and
    ops.set_deterministic(True), det_step_helpers.deterministic): loss and every parameter gradient of the md17 model on a
    batch that relift_(knn=3) built over another complex, and on the host-lifted, padded batch moved to the device - the
    same bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    first, second = K.md17_case(3), K.md17_case(1)
    cap = cx.capacity_of([first[3], second[3]])
    torch.manual_seed(11)
    model_a = M.MD17SimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = _md17_device_batch(cx, first, cap, dev)
        b.relift_(torch.from_numpy(second[0]).to(dev), vertex_features={k: v.to(dev) for k, v in second[1].items()}, knn=K.MD17_K)
        b.y.copy_(second[2])
        loss_a, grads_a = _loss_and_grads(model_a, b)
        host = cx.pad_batch(second[3], cap, K.MD17_VERTEX_FEATURES).to(dev)
        loss_b, grads_b = _loss_and_grads(model_b, host)
    assert int(b._plan["lift_status"].item()) == 0
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def _eager_and_graphed_losses(cases, dev):
    """Eight Adam steps over the four point sets: (losses of the eager loop on the unpadded host-lifted batches, losses of ONE
    captured step fed with step(points=..., knn=3) - the k once as the step's default and once in the call -, the two
    models, the step)."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
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
    cap = cx.capacity_of([c[3] for c in cases])
    gs = GraphedTrainStep(model_g, opt_g, cases[0][3], ["loc", "vel", "charges", "y"], capacity=cap, knn=K.MD17_K)
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}, c[2].to(dev)) for c in cases]
    for step in range(8):
        pts, vf, y = on_dev[step % 4]
        how = {} if step % 2 else {"knn": K.MD17_K}
        graphed.append(float(gs.step(features={"y": y}, points=pts, vertex_features=vf, **how).detach()))
    return np.asarray(eager), np.asarray(graphed), model_e, model_g, gs, on_dev


def test_graphed_step_on_device_lifted_points_matches_eager(pkg):
    """Eight Adam steps over four point sets, the eager loop on the unpadded host-lifted batches against ONE captured step fed
    with step(points=..., knn=3), within the 1e-3 of test_graphed_train_step_matches_eager.

    On the default (atomic) path, the one a training loop runs: the eight losses and status() == 0. In deterministic mode
    (fixed-order reductions, as the bit-for-bit test above): the losses AND every parameter with its floor of 1e-2. The
    parameters are not compared on the atomic path: Adam divides the gradient by the root of its second moment, so for a
    weight whose gradient is of the size of the rounding of its own sum the update is decided by that rounding and moves by
    the order of lr per step, and on the atomic path that rounding changes with the order in which the float atomics land.
    Two runs of the parameter comparison on the atomic path on identical code, on one MI355X, gave 2.4e-5 in one entry of
    one 4-column weight (|w| <= 6.8e-3, bound 1e-5) in one run and passed in the other; the eight losses of the failing run
    were within 1.5e-5 relative. With the order fixed the two loops differ by the batch they were given."""
    dev = _dev()
    cases = [K.md17_case(s) for s in (1, 2, 3, 4)]
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
        gs.step(points=on_dev[0][0], dis=1.6, knn=K.MD17_K)


def test_rips_and_knn_entries_agree_on_a_complete_graph(pkg):
    """One call of csmpn_rips_lift (dis = inf) and one of csmpn_knn_lift (k = V - 1, and k above it) on the same 3 x 7 points:
    the same rows; the adjacency blocks 1, 3 .. 7 of every graph agree; the Rips result alone has block 2 - per graph
    V (V - 1) - n1 pairs of type 0_0 between blocks 1 and 3."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    B, V = 3, 7
    pts = K.make_points("normal", 31, B, V, 3)
    n1, n2 = V * (V - 1) // 2, V * (V - 1) * (V - 2) // 6
    cap_r, cap_k = cx.rips_capacity(B, V, B * n1, B * n2), cx.knn_capacity(B, V, V - 1, B * n2)
    assert cap_r.simplices == cap_k.simplices and cap_r.edges == cap_k.edges + B * (V * (V - 1) - n1)
    p = torch.from_numpy(pts).to(dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = ops.rips_lift_workspace(B, V, 2, dev)
    out = {}
    for name, cap, run, param in (("rips", cap_r, ops.rips_lift, float("inf")), ("knn", cap_k, ops.knn_lift, V - 1),
                                  ("knn_above", cap_k, ops.knn_lift, 5 * V)):
        bufs = K.buffers(cap, B, dev)
        v = {key: t[0] for key, t in bufs.items()}
        run(p, B, param, 2, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"], v["ptr"],
            v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws)
        torch.cuda.synchronize()
        assert K.guards_intact(bufs) is None
        out[name] = {key: t.cpu() for key, t in v.items()}
    assert int(status.item()) == 0
    r, k = out["rips"], out["knn"]
    assert K.differences(out["knn_above"], k) == []
    for key in ("x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr"):
        assert torch.equal(r[key], k[key]), key
    assert r["counts"].tolist() == [B * V, B * n1, B * n2, cap_r.edges] and k["counts"].tolist()[:3] == r["counts"].tolist()[:3]
    per_r, per_k, block2 = V * (V - 1) + 5 * n1 + 12 * n2, 6 * n1 + 12 * n2, V * (V - 1) - n1
    assert k["counts"].tolist()[3] == B * per_k
    for g in range(B):
        a, b = g * per_r, g * per_k
        assert torch.equal(r["edge_index"][:, a:a + 2 * n1], k["edge_index"][:, b:b + 2 * n1])                   # block 1
        assert torch.equal(r["edge_index"][:, a + 2 * n1 + block2:a + per_r], k["edge_index"][:, b + 2 * n1:b + per_k])   # 3 .. 7
        assert torch.equal(r["edge_types"][a + 2 * n1 + block2:a + per_r], k["edge_types"][b + 2 * n1:b + per_k])
        assert bool((r["edge_types"][a + 2 * n1:a + 2 * n1 + block2] == 0).all())                                # block 2
        assert bool((k["edge_types"][b + 2 * n1:b + 4 * n1] == torch.tensor([0, 1])).all())                      # block 3 follows
