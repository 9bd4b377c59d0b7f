"""The kNN clique lift of point clouds on the device (GPU): csmpn_cloud_knn_lift against pad_batch(collate([knn_clique_complex(
...)]), capacity) on the float64 copy of the same float32 points - every structure tensor and the counts, exactly, between
guard regions, the same bits in two calls - at the word edges (V = 64 .. 200), over several graphs, for k = 1, 3, 8 and
k >= V - 1, on neighbours named in one direction only across a word boundary, outliers, ties, coincident points and NaN
vertices, with decoy points around the slice, at and over the capacity, against csmpn_knn_lift at V = 64 and on one graph of
4096 vertices; SimplicialBatch.relift_ of a kNN cloud batch without a host round trip or an allocation; the md17 model at V = 70
against the host-lifted batch, bit for bit; GraphedTrainStep.step(points=..., knn=...) on a kNN cloud batch against the eager
loop and against the host-fed captured step. The references come from cloud_knn_lift_helpers.fast_structure, which
tests/test_cloud_knn_lift_cpu.py holds against knn_clique_complex."""
import copy

import numpy as np
import pytest
import torch

import cloud_knn_lift_helpers as CK
import det_step_helpers as D
import rips_lift_helpers as R

pytestmark = pytest.mark.gpu
GUARD = CK.GUARD


def _dev():
    return torch.device("cuda:0")


def _lift(ops, points, n_graphs, k, max_dim, cap, bufs, status, ws=None):
    """ops.cloud_knn_lift of device points (a numpy array is moved there) into the guarded buffers."""
    p = torch.from_numpy(points).to(_dev()) if isinstance(points, np.ndarray) else points
    if ws is None:
        ws = ops.cloud_knn_lift_workspace(n_graphs, int(p.shape[0]) // n_graphs, max_dim, _dev())
    v = {key: t[0] for key, t in bufs.items()}
    ops.cloud_knn_lift(p, n_graphs, k, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                       v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws)
    torch.cuda.synchronize()
    return v


def _check_case(name, points=None):
    """One case against its reference: status 0, every tensor, the guards - and, over buffers refilled with the guard value and
    a workspace filled with ones, a second call that leaves the same bits (every position is written, none depends on the call
    or on what the workspace held)."""
    from csmpn_hip import ops
    pts, k, max_dim, cap, want = CK.reference(name)
    B, V = CK.CASES[name]["B"], CK.CASES[name]["V"]
    bufs = CK.buffers(cap, B, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts if points is None else points, B, k, max_dim, cap, bufs, status)
    assert int(status.item()) == 0
    assert CK.differences(got, want) == []
    assert CK.guards_intact(bufs) is None
    first = {key: t[1].clone() for key, t in bufs.items()}
    for t in bufs.values():
        t[1].fill_(GUARD)
    ws = ops.cloud_knn_lift_workspace(B, V, max_dim, _dev()).fill_(0xFF)
    _lift(ops, pts if points is None else points, B, k, max_dim, cap, bufs, status, ws)
    for key, t in bufs.items():
        assert torch.equal(t[1], first[key]), key
    return cap, want


STRUCTURE_CASES = ["v64_k3", "v65_k1", "v66_k8", "v128_k3", "v129_k8", "v129_k1", "v200_k3", "v1000_k8", "b3_65_k3", "b300_65_k3", "boundary_130_k1",
                   "outliers_3x70_k3", "clique_66_k65", "clique_66_k100", "lattice_72_k3", "coincident_70_k3", "one_point_65_k3",
                   "nan_vertex_2x70_k3", "max_dim_1_2x100_k3", "exact_capacity_2x66_k3", "tiny_12_k3", "tiny_12_k11"]


@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_structure_matches_host_lift(pkg, name):
    cap, want = _check_case(name)
    if name == "exact_capacity_2x66_k3":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    if name == "v200_k3":                                   # both ends of the four words are in use
        edges = want["x_ind"][want["node_types"] == 1]
        assert {int(v) // 64 for v in edges[:, :2].flatten()} == {0, 1, 2, 3}
    if name.startswith("clique_66"):
        assert want["counts"].tolist()[1:3] == [2145, 45760]


@pytest.mark.parametrize("name", ["v65_k1", "b3_65_k3"])
def test_no_point_outside_the_slice_is_read(pkg, name):
    """The points are a slice of a larger buffer whose rows in front and behind hold decoys next to real vertices - nearer
    than their nearest neighbours: a lane past V that read a point, counted or set a bit would change the answer (V = 65: 63
    lanes of word 1 lie past the cloud)."""
    pts = CK.points_of(name)
    n = pts.shape[0]
    big = np.concatenate([pts[:64] + np.float32(0.001), pts, pts[-64:] + np.float32(0.001)]).astype(np.float32)
    whole = torch.from_numpy(big).to(_dev())
    view = whole[64:64 + n]
    assert view.is_contiguous() and view.data_ptr() != whole.data_ptr()
    _check_case(name, points=view)


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row"])
def test_batch_that_does_not_fit_changes_nothing(pkg, kind):
    """b3_65 with k = 3 at a capacity it misses by one (or, for bit 4, at its exact rows with spare adjacencies) over buffers
    that hold the complex of k = 2 at that capacity: the bit is set, every buffer keeps every bit, and the next fitting call is
    served."""
    from csmpn.data.complexes import BatchCapacity
    from csmpn_hip import ops
    pts, k, max_dim, _, big_want = CK.reference("b3_65_k3")
    r0, n1, n2, E = big_want["counts"].tolist()
    cap, bit = {"dimension_1": (BatchCapacity((r0, n1 - 1, n2 + 2), E + 7), 1 << 1),
                "dimension_2": (BatchCapacity((r0, n1 + 3, n2 - 1), E + 7), 1 << 2),
                "adjacencies": (BatchCapacity((r0, n1 + 3, n2 + 2), E - 1), 1 << 3),
                "no_filler_row": (BatchCapacity((r0, n1, n2), E + 7), 1 << 4)}[kind]
    assert CK.conditioning_ok(pts, 3, 2)
    want = CK.fast_structure(pts, 3, 2, max_dim, cap)
    assert want["counts"][1] < n1 - 1 and want["counts"][2] < n2 - 1
    bufs = CK.buffers(cap, 3, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.cloud_knn_lift_workspace(3, 65, max_dim, _dev())
    got = _lift(ops, pts, 3, 2, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == 0 and CK.differences(got, want) == []
    before = {key: t[1].clone() for key, t in bufs.items()}
    _lift(ops, pts, 3, k, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == bit
    for key, t in bufs.items():
        assert torch.equal(t[1], before[key]), key
    got = _lift(ops, pts, 3, 2, max_dim, cap, bufs, status, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert CK.differences(got, want) == [] and CK.guards_intact(bufs) is None


@pytest.mark.parametrize("name", ["v64_k3", "tiny_12_k8"])
def test_up_to_64_vertices_are_the_bits_of_knn_lift(pkg, name):
    from csmpn_hip import ops
    pts, k, max_dim, cap, want = CK.reference(name)
    B, V = CK.CASES[name]["B"], CK.CASES[name]["V"]
    dev = _dev()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mine, theirs = CK.buffers(cap, B, dev), CK.buffers(cap, B, dev)
    _lift(ops, pts, B, k, max_dim, cap, mine, status)
    v = {key: t[0] for key, t in theirs.items()}
    ops.knn_lift(torch.from_numpy(pts).to(dev), B, k, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"],
                 v["x_ind_batch"], v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status,
                 ops.knn_lift_workspace(B, V, max_dim, dev))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and CK.differences(v, want) == []
    for key in mine:
        assert torch.equal(mine[key][1], theirs[key][1]), key


def test_one_graph_of_4096_vertices(pkg):
    """The only case above a few hundred vertices: a jittered 64 x 64 grid in sixteenths in a random vertex order, k = 8 - every
    sum is exact and some vertices have equal sums at the k-th place, every vertex has neighbours all over the 64 words, and the
    selection walks 64 words in every one of its passes."""
    cap, want = _check_case("grid_4096_k8")
    counts = want["counts"].tolist()
    assert counts[0] == 4096 and 4 * 4096 <= counts[1] <= 8 * 4096 and counts[2] > 4096
    edges = want["x_ind"][want["node_types"] == 1]
    assert int(((edges[:, 1] // 64) - (edges[:, 0] // 64)).max()) > 32
    s = CK.pair_sums(CK.points_of("grid_4096_k8").astype(np.float64))
    s[np.arange(4096), np.arange(4096)] = np.inf
    near = np.partition(s, (7, 8), axis=1)
    assert int((near[:, 7] == near[:, 8]).sum()) >= 10      # vertices whose 8th and 9th sums are equal: the index decides


def _relift_capacity(names):
    from csmpn.data.complexes import BatchCapacity
    counts = np.array([CK.reference(n)[4]["counts"].tolist() for n in names]).max(axis=0).tolist()
    return BatchCapacity((counts[0], counts[1] + 3, counts[2] + 2), counts[3] + 7)


def test_relift_of_a_knn_cloud_batch_needs_no_host(pkg):
    """A 2 x 96 kNN cloud batch: the second and third relift_ run with synchronisation made an error and allocate nothing; the
    batch then holds the third point set - structure, counts, every table of plan() and the CSR as a fresh device batch has
    them - and refuses every other lift."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    names = ("relift_96_a", "relift_96_b", "relift_96_c")
    cap = _relift_capacity(names)
    on_dev = [torch.from_numpy(CK.points_of(n)).to(dev) for n in names]
    b = cx.knn_cloud_batch_device(on_dev[0], 2, 3, cap)
    assert b._plan["cloud_knn"] == {"k": 3} and "cloud" not in b._plan
    assert b._plan["lift_ws"].numel() == ops.cloud_knn_lift_workspace(2, 96, 2, dev).numel()
    b.csr().source_order()
    ptrs = {key: getattr(b, key).data_ptr() for key in b._names}
    ws = b._plan["lift_ws"].data_ptr()
    b.relift_(on_dev[1], knn=3)                            # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0], knn=3)
        b.relift_(on_dev[2], knn=3)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {key: getattr(b, key).data_ptr() for key in b._names} == ptrs and b._plan["lift_ws"].data_ptr() == ws
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    want = CK.fast_structure(CK.points_of(names[2]), 2, 3, 2, cap)
    got = {key: getattr(b, key) for key in CK.STRUCTURE}
    got["counts"] = b._plan["lift_counts"]
    assert CK.differences(got, want) == []
    fresh = cx.SimplicialBatch(**{key: want[key].to(dev) for key in CK.STRUCTURE})
    plan = fresh.plan(2)
    for d in range(3):
        assert torch.equal(b._plan["rows"][d], plan["rows"][d]) and torch.equal(b._plan["verts"][d], plan["verts"][d]), d
    assert torch.equal(b._plan["graph_of_vertex"], plan["graph_of_vertex"])
    csr = fresh.csr()
    for key in ("perm", "src", "dst", "deg", "row_ptr"):
        assert torch.equal(getattr(b._csr, key), getattr(csr, key)), key
    assert ops.get_csr(b.edge_index, cap.rows) is b._csr
    for kw in (dict(dis=1.0), dict(hull=True), dict(edges=torch.zeros(2, 1, dtype=torch.int64, device=dev)), dict(knn=3, edge_th=1.0)):
        with pytest.raises(ValueError, match="kNN cloud batch"):
            b.relift_(on_dev[0], **kw)
    with pytest.raises(ValueError, match="does not fit the capacity"):
        cx.knn_cloud_batch_device(on_dev[0], 2, 8, cap)


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {key: p.grad.clone() for key, p in model.named_parameters() if p.grad is not None}


def test_md17_model_on_a_knn_cloud_batch_is_bit_identical(pkg):
    """Deterministic mode as test_rips_lift_gpu.py sets it: loss and every parameter gradient of the md17 model on ONE graph of
    70 vertices, on the batch knn_cloud_batch_device lifted and on the host-lifted, padded batch moved to the device - the same
    bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    pts, vf, y, host = CK.md17_cloud_case(1)
    cap = cx.capacity_of([host])
    torch.manual_seed(11)
    model_a = M.MD17SimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = cx.knn_cloud_batch_device(torch.from_numpy(pts).to(dev), 1, CK.MD17_K, cap, features={"y": y}, vertex_features=vf)
        loss_a, grads_a = _loss_and_grads(model_a, b)
        padded = cx.pad_batch(host, cap, CK.MD17_VERTEX_FEATURES)
        for key in CK.STRUCTURE:
            assert torch.equal(getattr(b, key).cpu(), getattr(padded, key)), key
        loss_b, grads_b = _loss_and_grads(model_b, padded.to(dev))
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for key in grads_a:
        assert torch.equal(grads_a[key], grads_b[key]), key


_MD17_CASES = {}


def _md17_cases():
    if not _MD17_CASES:
        _MD17_CASES.update({s: CK.md17_cloud_case(s) for s in (1, 2, 3)})
    return [_MD17_CASES[s] for s in (1, 2, 3)]


def _cloud_step(cx, GraphedTrainStep, model, opt, cases, cap, dev, **defaults):
    """One step captured over the kNN cloud batch of cases[0]: (the step, the device copies of every case)."""
    on_dev = [(torch.from_numpy(c[0]).to(dev), {key: v.to(dev) for key, v in c[1].items()}, c[2].to(dev)) for c in cases]
    first = cx.knn_cloud_batch_device(on_dev[0][0], 1, CK.MD17_K, cap, features={"y": cases[0][2]}, vertex_features=cases[0][1])
    gs = GraphedTrainStep(model, opt, first, ["loc", "vel", "charges", "y"], capacity=cap, **defaults)
    assert gs.batch is first
    return gs, on_dev


def test_graphed_step_on_a_knn_cloud_batch_matches_eager(pkg):
    """Six steps over three clouds of 70 points: the eager loop on the unpadded host-lifted batches against ONE step captured
    over a kNN cloud batch and fed with step(points=...) under the step's knn default, within the 1e-3 of
    test_cloud_lift_gpu.py::test_graphed_step_on_a_cloud_batch_matches_eager, losses and parameters, under its optimiser (SGD at
    lr = 1e-3; that test's docstring says why). Everything but knn is refused there."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    cases = _md17_cases()
    assert len({tuple(R.counts_of(c[3], 2)) for c in cases}) == 3       # three topologies
    torch.manual_seed(7)
    model_e = M.MD17SimplicialMPNN().to(dev)
    model_g = copy.deepcopy(model_e)
    opt_e = torch.optim.SGD(model_e.parameters(), lr=1e-3)
    opt_g = torch.optim.SGD(model_g.parameters(), lr=1e-3)
    eager, graphed = [], []
    for step in range(6):
        loss, _ = model_e(cases[step % 3][3].to(dev))
        opt_e.zero_grad(set_to_none=True)
        loss.backward()
        opt_e.step()
        eager.append(float(loss.detach()))
    cap = cx.capacity_of([c[3] for c in cases])
    gs, on_dev = _cloud_step(cx, GraphedTrainStep, model_g, opt_g, cases, cap, dev, knn=CK.MD17_K)
    for step in range(6):
        pts, vf, y = on_dev[step % 3]
        graphed.append(float(gs.step(features={"y": y}, points=pts, vertex_features=vf).detach()))
    assert gs.status() == 0
    eager, graphed = np.asarray(eager), np.asarray(graphed)
    print("eager", eager, "graphed", graphed)
    assert eager[3] != eager[0]                             # the steps did move the parameters
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
    for kw in (dict(dis=1.0), dict(hull=True), dict(knn=3, edge_th=1.0), dict(edges=torch.zeros(2, 1, dtype=torch.int64, device=dev))):
        with pytest.raises(ValueError, match="kNN cloud batch"):
            gs.step(points=on_dev[0][0], **kw)


def test_graphed_adam_step_on_a_knn_cloud_batch_is_the_host_fed_step(pkg):
    """Deterministic mode: six captured Adam steps over the three clouds fed as device points (step(points=..., knn=k) on a kNN
    cloud batch) and fed as host-lifted batches (step(batch=...)) - the same structure bits go into the same kernels, so every
    loss and every final parameter holds the same bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    cases = _md17_cases()
    cap = cx.capacity_of([c[3] for c in cases])
    torch.manual_seed(7)
    model_c = M.MD17SimplicialMPNN().to(dev)
    model_h = copy.deepcopy(model_c)
    with D.deterministic(torch_flag=True, request=True):
        gs_c, on_dev = _cloud_step(cx, GraphedTrainStep, model_c, torch.optim.Adam(model_c.parameters(), lr=1e-3, capturable=True), cases,
                                   cap, dev)
        gs_h = GraphedTrainStep(model_h, torch.optim.Adam(model_h.parameters(), lr=1e-3, capturable=True), cases[0][3],
                                ["loc", "vel", "charges", "y"], capacity=cap)
        cloud, host = [], []
        for step in range(6):
            pts, vf, y = on_dev[step % 3]
            cloud.append(gs_c.step(features={"y": y}, points=pts, vertex_features=vf, knn=CK.MD17_K).detach().clone())
            host.append(gs_h.step(batch=cases[step % 3][3]).detach().clone())
        torch.cuda.synchronize()
    assert gs_c.status() == 0 and gs_h.status() == 0
    print("cloud", [float(x) for x in cloud], "host", [float(x) for x in host])
    assert all(torch.equal(a, b) for a, b in zip(cloud, host))
    assert not torch.equal(cloud[0], cloud[3])
    for pc, ph in zip(model_c.parameters(), model_h.parameters()):
        assert torch.equal(pc, ph)
