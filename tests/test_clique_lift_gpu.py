"""The thresholded clique lift on the device (GPU): csmpn_clique_lift against
pad_batch(collate([clique_complex(...)]), capacity) on the float64 copy of the same float32 points, exactly and between guard
regions, on the smallest shapes that reach each part of lift_list_kernel, lift_filter_kernel and the 64-wide table scatter;
infinite thresholds against csmpn_knn_lift bit for bit; batches that do not fit and lists with a bad end;
SimplicialBatch.relift_(points, edges=...) without a host round trip or an allocation; the md17 model on a re-lifted batch
against the host-lifted one, bit for bit; GraphedTrainStep.step(points=..., edges=..., edge_th=..., tri_th=...) against the eager
loop over lists of three lengths in one buffer."""
import copy
import math

import numpy as np
import pytest
import torch

import det_step_helpers as D
import clique_lift_helpers as Q

pytestmark = pytest.mark.gpu
INF = math.inf


def _dev():
    return torch.device("cuda:0")


def _lift(ops, pts, n_graphs, source, edge_th, tri_th, max_dim, cap, bufs, status, ws=None):
    """source: an int k or a numpy list [2, n] of global ids."""
    dev = _dev()
    p = torch.from_numpy(pts).to(dev)
    if ws is None:
        ws = ops.clique_lift_workspace(n_graphs, pts.shape[0] // n_graphs, max_dim, dev)
    if not isinstance(source, int):
        source = torch.from_numpy(np.ascontiguousarray(source)).to(dev)
    v = {key: t[0] for key, t in bufs.items()}
    ops.clique_lift(p, n_graphs, source, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                    v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws, edge_th=edge_th, tri_th=tri_th)
    torch.cuda.synchronize()
    return v


@pytest.mark.parametrize("name", Q.CASES)
def test_structure_matches_host_lift(pkg, name):
    from csmpn_hip import ops
    pts, B, glist, k, edge_th, tri_th, max_dim, cap, _, want = Q.reference(name)
    bufs = Q.buffers(cap, B, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts, B, k if glist is None else glist, edge_th, tri_th, max_dim, cap, bufs, status)
    assert int(status.item()) == 0
    assert Q.differences(got, want) == []
    assert Q.guards_intact(bufs) is None
    if name == "exact_capacity_4x9":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    first = {key: t.clone() for key, t in got.items()}     # a second call: the same bits
    again = _lift(ops, pts, B, k if glist is None else glist, edge_th, tri_th, max_dim, cap, bufs, status)
    assert all(torch.equal(again[key], first[key]) for key in first) and int(status.item()) == 0


@pytest.mark.parametrize("name", ["all_mask_bits_3x64", "aspirin_16x21", "nan_vertex_2x8", "coincident_2x6", "max_dim_1_4x7",
                                  "second_scan_pass_300x4"])
def test_infinite_thresholds_are_the_knn_lift_bit_for_bit(pkg, name):
    """Both thresholds +infinity: the k source gives the bits of csmpn_knn_lift (guard regions included), and the knn_edges list
    as the source gives the bits of the k source - ties, coincident points and a NaN vertex among the cases."""
    import knn_lift_helpers as K
    from csmpn_hip import ops
    dev = _dev()
    pts, k, max_dim, cap, want = K.reference(name)
    B = K.CASES[name][0]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    whole = {}
    bufs = K.buffers(cap, B, dev)
    v = {key: t[0] for key, t in bufs.items()}
    ops.knn_lift(torch.from_numpy(pts).to(dev), B, k, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"],
                 v["x_ind_batch"], v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status,
                 ops.knn_lift_workspace(B, pts.shape[0] // B, max_dim, dev))
    torch.cuda.synchronize()
    whole["knn_lift"] = {key: t[1].clone() for key, t in bufs.items()}
    for how, source in (("k", k), ("list", Q.knn_list(pts, B, k))):
        bufs = K.buffers(cap, B, dev)
        got = _lift(ops, pts, B, source, INF, INF, max_dim, cap, bufs, status)
        assert Q.differences(got, want) == [], how
        whole[how] = {key: t[1].clone() for key, t in bufs.items()}
    assert int(status.item()) == 0
    for key in whole["knn_lift"]:
        assert torch.equal(whole["k"][key], whole["knn_lift"][key]) and torch.equal(whole["list"][key], whole["k"][key]), key


def _short_capacity(kind, rows, edges):
    from csmpn.data.complexes import BatchCapacity
    return {"dimension_1": (BatchCapacity((rows[0], rows[1] - 1, rows[2] + 2), edges + 7), 1 << 1),
            "dimension_2": (BatchCapacity((rows[0], rows[1] + 3, rows[2] - 1), edges + 7), 1 << 2),
            "adjacencies": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges - 1), 1 << 3),
            "no_filler_row": (BatchCapacity(tuple(rows), edges + 7), 1 << 4),
            "end_out_of_range": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges + 7), 1 << 5),
            "end_below_zero": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges + 7), 1 << 5),
            "ends_in_two_graphs": (BatchCapacity((rows[0], rows[1] + 3, rows[2] + 2), edges + 7), 1 << 5)}[kind]


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row", "end_out_of_range", "end_below_zero",
                                  "ends_in_two_graphs"])
def test_refused_batch_changes_nothing(pkg, kind):
    """4 x 6 points over their k = 4 list at a capacity they miss by one (or, for bit 4, at their exact rows with spare
    adjacencies; for bit 5, at a capacity they fit, with ONE bad entry in the list: an end at B V, an end at -3, two ends in
    neighbouring graphs) over buffers that hold other points over a k = 2 list at that capacity: exactly that bit is set,
    every buffer keeps every bit, and the next good call is served."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    big, small = Q.make_points("normal", 21, 4, 6, 3), Q.make_points("normal", 22, 4, 6, 3)
    big_list, small_list = Q.knn_list(big, 4, 4), Q.knn_list(small, 4, 2)
    th = (1.9, 1.1)
    big_counts = Q.counts_of(Q.host_lift(big, 4, Q.local_lists(big_list, 4, 6), *th, 2), 2)
    small_raw = Q.host_lift(small, 4, Q.local_lists(small_list, 4, 6), *th, 2)
    small_counts = Q.counts_of(small_raw, 2)
    assert small_counts[1] < big_counts[1] - 1 and small_counts[2] < big_counts[2] - 1 and small_counts[3] < big_counts[3] - 1
    cap, bit = _short_capacity(kind, big_counts[:3], big_counts[3])
    bad_entry = {"end_out_of_range": (3, 24), "end_below_zero": (-3, 2), "ends_in_two_graphs": (5, 6)}.get(kind)
    if bad_entry is not None:
        big_list = np.concatenate([big_list[:, :7], np.array([bad_entry], dtype=np.int64).T, big_list[:, 7:]], axis=1)
    padded = cx.pad_batch(small_raw, cap)
    want = {key: getattr(padded, key) for key in Q.STRUCTURE}
    want["counts"] = torch.tensor(small_counts, dtype=torch.int64)
    bufs = Q.buffers(cap, 4, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.clique_lift_workspace(4, 6, 2, _dev())
    got = _lift(ops, small, 4, small_list, *th, 2, cap, bufs, status, ws)
    assert int(status.item()) == 0 and Q.differences(got, want) == []
    before = {key: t[1].clone() for key, t in bufs.items()}
    _lift(ops, big, 4, big_list, *th, 2, cap, bufs, status, ws)
    assert int(status.item()) == bit
    for key, t in bufs.items():
        assert torch.equal(t[1], before[key]), key
    got = _lift(ops, small, 4, small_list, *th, 2, cap, bufs, status, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert Q.differences(got, want) == [] and Q.guards_intact(bufs) is None


def _md17_device_batch(cx, case, cap, dev):
    pts, vf, y, _, glist = case
    return cx.clique_batch_device(torch.from_numpy(pts).to(dev), 4, cap, edges=glist, edge_th=Q.MD17_EDGE_TH, tri_th=Q.MD17_TRI_TH,
                                  features={"y": y}, vertex_features=vf)


def test_first_batch_is_refused_over_the_capacity_or_with_a_bad_list(pkg):
    from csmpn.data import complexes as cx
    case = Q.md17_case(1)
    c = Q.counts_of(case[3], 2)
    with pytest.raises(ValueError, match="does not fit"):
        _md17_device_batch(cx, case, cx.BatchCapacity((c[0], c[1] - 1, c[2]), c[3]), _dev())
    bad = case[:4] + (torch.cat([case[4], torch.tensor([[0], [24]])], dim=1),)
    with pytest.raises(ValueError, match="0x20"):
        _md17_device_batch(cx, bad, cx.BatchCapacity((c[0], c[1] + 1, c[2]), c[3]), _dev())


def test_relift_needs_no_host(pkg):
    """The second and third relift_(points, edges=...) - lists of other lengths - run with synchronisation made an error and
    allocate nothing; the batch then holds the third point set: structure, features, and every table of plan() and the CSR as
    a fresh device batch has them. relift_(knn=3, edge_th=...) goes through the same entry: the complex of the kNN list."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    cases = [Q.md17_case(s, extra=x) for s, x in ((1, 0), (2, 3), (3, 7))]
    assert len({int(c[4].shape[1]) for c in cases}) == 3
    cap = cx.capacity_of([c[3] for c in cases])
    b = _md17_device_batch(cx, cases[0], cap, dev)
    b.csr().source_order()
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}, c[4].to(dev)) for c in cases]
    th = dict(edge_th=Q.MD17_EDGE_TH, tri_th=Q.MD17_TRI_TH)
    ptrs = {k: getattr(b, k).data_ptr() for k in b._names}
    b.relift_(on_dev[1][0], vertex_features=on_dev[1][1], edges=on_dev[1][2], **th)      # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0][0], None, on_dev[0][1], edges=on_dev[0][2], **th)
        b.relift_(on_dev[2][0], edges=on_dev[2][2], vertex_features=on_dev[2][1], **th)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {k: getattr(b, k).data_ptr() for k in b._names} == ptrs
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    padded = cx.pad_batch(cases[2][3], cap, Q.MD17_VERTEX_FEATURES)
    for k in padded._names:
        if k != "y":                                       # the target is not part of the lift
            assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k
    assert b._plan["lift_counts"].tolist() == Q.counts_of(cases[2][3], 2)
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
        b.relift_(on_dev[0][0], 1.6, on_dev[0][1], edges=on_dev[0][2])
    b.relift_(on_dev[0][0], vertex_features=on_dev[0][1], knn=3, **th)                 # case 0's list IS its k = 3 list
    torch.cuda.synchronize()
    assert int(b._plan["lift_status"].item()) == 0
    padded = cx.pad_batch(cases[0][3], cap, Q.MD17_VERTEX_FEATURES)
    for k in Q.STRUCTURE:
        assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def test_md17_model_on_relifted_batch_is_bit_identical(pkg):
    """Deterministic mode as the bit-for-bit step tests set it: loss and every parameter gradient of the md17 model on a batch
    that relift_(edges=...) built over another complex, and on the host-lifted, padded batch moved to the device - the same
    bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    first, second = Q.md17_case(3, extra=5), Q.md17_case(1, extra=2)
    cap = cx.capacity_of([first[3], second[3]])
    torch.manual_seed(11)
    model_a = M.MD17SimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = _md17_device_batch(cx, first, cap, dev)
        b.relift_(torch.from_numpy(second[0]).to(dev), vertex_features={k: v.to(dev) for k, v in second[1].items()},
                  edges=second[4].to(dev), edge_th=Q.MD17_EDGE_TH, tri_th=Q.MD17_TRI_TH)
        b.y.copy_(second[2])
        loss_a, grads_a = _loss_and_grads(model_a, b)
        host = cx.pad_batch(second[3], cap, Q.MD17_VERTEX_FEATURES).to(dev)
        loss_b, grads_b = _loss_and_grads(model_b, host)
    assert int(b._plan["lift_status"].item()) == 0
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def test_graphed_step_on_listed_graphs_matches_eager(pkg):
    """Six Adam steps over three point sets whose lists have three different lengths, in deterministic mode (fixed-order
    reductions, as test_knn_lift_gpu compares parameters): the eager loop on the unpadded host-lifted batches against ONE
    captured step fed with step(points=..., edges=..., edge_th=..., tri_th=...) - the thresholds once as the step's defaults and
    once in the call - through one static list buffer: the losses within the 1e-3 of test_graphed_train_step_matches_eager,
    every parameter with its floor of 1e-2, status() == 0; a list longer than the buffer is a ValueError, a bad end shows in
    status()."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep, LIFT_STATUS_SHIFT
    dev = _dev()
    cases = [Q.md17_case(s, extra=x) for s, x in ((1, 0), (2, 3), (3, 7))]
    lengths = [int(c[4].shape[1]) for c in cases]
    assert len(set(lengths)) == 3
    th = dict(edge_th=Q.MD17_EDGE_TH, tri_th=Q.MD17_TRI_TH)
    with D.deterministic(torch_flag=True, request=True):
        torch.manual_seed(7)
        model_e = M.MD17SimplicialMPNN().to(dev)
        model_g = copy.deepcopy(model_e)
        opt_e = torch.optim.Adam(model_e.parameters(), lr=1e-3)
        opt_g = torch.optim.Adam(model_g.parameters(), lr=1e-3, capturable=True)
        eager, graphed = [], []
        for step in range(6):
            loss, _ = model_e(cases[step % 3][3].to(dev))
            opt_e.zero_grad(set_to_none=True)
            loss.backward()
            opt_e.step()
            eager.append(float(loss.detach()))
        cap = cx.capacity_of([c[3] for c in cases])
        gs = GraphedTrainStep(model_g, opt_g, cases[0][3], ["loc", "vel", "charges", "y"], capacity=cap, edges=max(lengths), **th)
        buffer = gs._edge_buffer
        assert tuple(buffer.shape) == (2, max(lengths))
        on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}, c[2].to(dev), c[4].to(dev)) for c in cases]
        for step in range(6):
            pts, vf, y, glist = on_dev[step % 3]
            how = {} if step % 2 else th
            graphed.append(float(gs.step(features={"y": y}, points=pts, vertex_features=vf, edges=glist, **how).detach()))
        assert gs._edge_buffer is buffer and gs.status() == 0
    eager, graphed = np.asarray(eager), np.asarray(graphed)
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
    with pytest.raises(ValueError, match="list buffer"):
        gs.step(points=on_dev[0][0], edges=torch.zeros(2, max(lengths) + 1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="exclude"):
        gs.step(points=on_dev[0][0], edges=on_dev[0][3], knn=3)
    gs.step(points=on_dev[0][0], vertex_features=on_dev[0][1], edges=torch.tensor([[0, 5], [1, 6]], device=dev))
    assert gs.status() == 32 << LIFT_STATUS_SHIFT
