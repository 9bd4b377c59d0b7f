"""The Rips lift of point clouds on the device (GPU): csmpn_cloud_lift against pad_batch(collate([rips_complex(...,
vertex_block)]), capacity) on the float64 copy of the same float32 points - every structure tensor and the counts, exactly,
between guard regions, the same bits in two calls - at the word edges (V = 64 .. 200), over several graphs, on placed and
dense structures, with decoy points around the slice, at the edges of the rule, at and over the capacity, against
csmpn_rips_lift and csmpn_clique_lift at V = 64 and on one graph of 4096 vertices; SimplicialBatch.relift_ of a cloud batch
without a host round trip or an allocation; the md17 model at V = 70 against the host-lifted batch, bit for bit;
GraphedTrainStep.step(points=..., dis=...) on a cloud batch against the eager loop. The references come from
cloud_lift_helpers.fast_structure, which tests/test_cloud_lift_cpu.py holds against lift()."""
import copy
import itertools

import numpy as np
import pytest
import torch

import cloud_lift_helpers as CL
import det_step_helpers as D
import rips_lift_helpers as R

pytestmark = pytest.mark.gpu
GUARD = -77


def _dev():
    return torch.device("cuda:0")


def _guarded(shape, dev, pad=64):
    """An int64 tensor of `shape` inside a larger buffer of guard values: (view, whole buffer, offset)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), GUARD, dtype=torch.int64, device=dev)
    return whole[pad:pad + n].view(shape), whole, pad


def _buffers(cap, n_graphs, dev):
    S, E, nd = cap.rows, cap.edges, cap.max_dim + 1
    shapes = dict(x_ind=(S, nd), node_types=(S,), batch=(S,), x_ind_batch=(S,), ptr=(n_graphs + 1,), x_ind_ptr=(n_graphs + 1,),
                  edge_index=(2, E), edge_types=(E, 2), counts=(nd + 1,))
    return {k: _guarded(s, dev) for k, s in shapes.items()}


def _guards_intact(bufs):
    for k, (view, whole, pad) in bufs.items():
        n = view.numel()
        if not (bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())):
            return k
    return None


def _lift(ops, points, n_graphs, dis, max_dim, cap, bufs, status, vertex_block, ws=None):
    """ops.cloud_lift of device points (a numpy array is moved there) into the guarded buffers."""
    p = torch.from_numpy(points).to(_dev()) if isinstance(points, np.ndarray) else points
    if ws is None:
        ws = ops.cloud_lift_workspace(n_graphs, int(p.shape[0]) // n_graphs, max_dim, _dev())
    v = {k: t[0] for k, t in bufs.items()}
    ops.cloud_lift(p, n_graphs, dis, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"],
                   v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status, ws, vertex_block=vertex_block)
    torch.cuda.synchronize()
    return v


def _check_case(name, vertex_block, points=None):
    """One case against its reference: status 0, every tensor, the guards - and, over buffers refilled with the guard value, a
    second call that leaves the same bits (every position is written, none depends on the call)."""
    from csmpn_hip import ops
    pts, dis, max_dim, cap, want = CL.reference(name, vertex_block)
    B = CL.CASES[name]["B"]
    bufs = _buffers(cap, B, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    got = _lift(ops, pts if points is None else points, B, dis, max_dim, cap, bufs, status, vertex_block)
    assert int(status.item()) == 0
    assert CL.differences(got, want) == []
    assert _guards_intact(bufs) is None
    first = {k: t[1].clone() for k, t in bufs.items()}
    for t in bufs.values():
        t[1].fill_(GUARD)
    _lift(ops, pts if points is None else points, B, dis, max_dim, cap, bufs, status, vertex_block)
    for k, t in bufs.items():
        assert torch.equal(t[1], first[k]), k
    return cap, want


STRUCTURE_CASES = ["sparse_64", "sparse_65", "sparse_66", "sparse_128", "sparse_129", "sparse_200", "b3_65", "b300_65", "placed_200",
                   "clique66_in_130", "complete_65_dim1", "lattice_tie_72", "lattice_ulp_below_72", "dis0_coincident_70",
                   "nan_vertex_70", "max_dim_1_100", "exact_capacity_66"]


@pytest.mark.parametrize("vertex_block", [0, 1], ids=["no_block", "block"])
@pytest.mark.parametrize("name", STRUCTURE_CASES)
def test_structure_matches_host_lift(pkg, name, vertex_block):
    cap, want = _check_case(name, vertex_block)
    if name == "exact_capacity_66":
        assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    if name == "sparse_200":                               # both ends of the four words are in use
        edges = want["x_ind"][want["node_types"] == 1]
        assert {int(v) // 64 for v in edges[:, :2].flatten()} == {0, 1, 2, 3}


@pytest.mark.parametrize("vertex_block", [0, 1], ids=["no_block", "block"])
@pytest.mark.parametrize("name", ["sparse_65", "b3_65"])
def test_no_point_outside_the_slice_is_read(pkg, name, vertex_block):
    """The points are a slice of a larger buffer whose rows in front and behind hold decoys within dis of real vertices: a
    lane past V that read a point or set a bit would change the answer (V = 65: 63 lanes of word 1 lie past the cloud)."""
    pts = CL.points_of(name)
    n = pts.shape[0]
    big = np.concatenate([pts[:64] + np.float32(0.01), pts, pts[-64:] + np.float32(0.01)]).astype(np.float32)
    whole = torch.from_numpy(big).to(_dev())
    view = whole[64:64 + n]
    assert view.is_contiguous() and view.data_ptr() != whole.data_ptr()
    _check_case(name, vertex_block, points=view)


def _smaller_dis(name):
    """A threshold under the case's own that keeps the margin: a strictly smaller complex on the same points."""
    c = CL.CASES[name]
    for dis in (0.8, 0.79, 0.78, 0.77, 0.76, 0.75):
        if CL.conditioning_ok(CL.points_of(name), c["B"], dis):
            return dis
    raise AssertionError("no smaller threshold keeps the margin")


@pytest.mark.parametrize("kind", ["dimension_1", "dimension_2", "adjacencies", "no_filler_row"])
def test_batch_that_does_not_fit_changes_nothing(pkg, kind):
    """b3_65 at a capacity it misses by one (or, for bit 4, at its exact rows with spare adjacencies) over buffers that hold
    the complex of a smaller threshold at that capacity: the bit is set, every buffer keeps every bit, and the next fitting
    call is served."""
    from csmpn.data.complexes import BatchCapacity
    from csmpn_hip import ops
    name, vb = "b3_65", 1
    pts, dis, max_dim, _, big_want = CL.reference(name, vb)
    r0, n1, n2, E = big_want["counts"].tolist()
    cap, bit = {"dimension_1": (BatchCapacity((r0, n1 - 1, n2 + 2), E + 7), 1 << 1),
                "dimension_2": (BatchCapacity((r0, n1 + 3, n2 - 1), E + 7), 1 << 2),
                "adjacencies": (BatchCapacity((r0, n1 + 3, n2 + 2), E - 1), 1 << 3),
                "no_filler_row": (BatchCapacity((r0, n1, n2), E + 7), 1 << 4)}[kind]
    small = _smaller_dis(name)
    want = CL.fast_structure(pts, 3, small, max_dim, vb, cap)
    assert want["counts"][1] < n1 - 1 and want["counts"][2] < n2 - 1
    bufs = _buffers(cap, 3, _dev())
    status = torch.zeros(1, dtype=torch.int32, device=_dev())
    ws = ops.cloud_lift_workspace(3, 65, max_dim, _dev())
    got = _lift(ops, pts, 3, small, max_dim, cap, bufs, status, vb, ws)
    assert int(status.item()) == 0 and CL.differences(got, want) == []
    before = {k: t[1].clone() for k, t in bufs.items()}
    _lift(ops, pts, 3, dis, max_dim, cap, bufs, status, vb, ws)
    assert int(status.item()) == bit
    for k, t in bufs.items():
        assert torch.equal(t[1], before[k]), k
    got = _lift(ops, pts, 3, small, max_dim, cap, bufs, status, vb, ws)
    assert int(status.item()) == bit                       # never cleared by the call
    assert CL.differences(got, want) == [] and _guards_intact(bufs) is None


def test_64_vertices_with_the_block_are_the_bits_of_rips_lift(pkg):
    from csmpn_hip import ops
    pts, dis, max_dim, cap, want = CL.reference("sparse_64", True)
    dev = _dev()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mine, theirs = _buffers(cap, 1, dev), _buffers(cap, 1, dev)
    _lift(ops, pts, 1, dis, max_dim, cap, mine, status, 1)
    v = {k: t[0] for k, t in theirs.items()}
    ops.rips_lift(torch.from_numpy(pts).to(dev), 1, dis, max_dim, cap.simplices, cap.edges, v["x_ind"], v["node_types"], v["batch"],
                  v["x_ind_batch"], v["ptr"], v["x_ind_ptr"], v["edge_index"], v["edge_types"], v["counts"], status,
                  ops.rips_lift_workspace(1, 64, max_dim, dev))
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and CL.differences(v, want) == []
    for k in mine:
        assert torch.equal(mine[k][1], theirs[k][1]), k


@pytest.mark.parametrize("form", ["close_pairs_max_dim_2", "complete_tri_th_0_max_dim_1"])
def test_64_vertices_without_the_block_are_the_bits_of_clique_lift(pkg, form):
    """csmpn_clique_lift with edge_th = dis, in the two forms in which the thresholded clique lift IS the Rips complex
    (tests/test_cloud_lift_cpu.py::test_rips_without_vertex_block_is_the_clique_complex says why the complete list with an
    infinite tri_th is not one: it keeps every triple): the list of the close pairs at max_dim = 2, and the complete graph's
    list with tri_th = 0 at max_dim = 1."""
    from csmpn_hip import ops
    c = CL.CASES["sparse_64"]
    pts, dis, dev = CL.points_of("sparse_64"), c["dis"], _dev()
    max_dim = 2 if form == "close_pairs_max_dim_2" else 1
    counts = CL.fast_structure(pts, 1, dis, max_dim, False)["counts"].tolist()
    cap = CL.capacity_for(counts, max_dim, "spare")
    pairs = np.array(list(itertools.combinations(range(64), 2)), dtype=np.int64).T
    if max_dim == 2:
        p64 = pts.astype(np.float64)
        pairs = pairs[:, np.linalg.norm(p64[pairs[0]] - p64[pairs[1]], axis=-1) <= dis]
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mine, theirs = _buffers(cap, 1, dev), _buffers(cap, 1, dev)
    _lift(ops, pts, 1, dis, max_dim, cap, mine, status, 0)
    v = {k: t[0] for k, t in theirs.items()}
    ops.clique_lift(torch.from_numpy(pts).to(dev), 1, torch.from_numpy(np.ascontiguousarray(pairs)).to(dev), max_dim, cap.simplices,
                    cap.edges, v["x_ind"], v["node_types"], v["batch"], v["x_ind_batch"], v["ptr"], v["x_ind_ptr"], v["edge_index"],
                    v["edge_types"], v["counts"], status, ops.clique_lift_workspace(1, 64, max_dim, dev), edge_th=dis,
                    tri_th=float("inf") if max_dim == 2 else 0.0)
    torch.cuda.synchronize()
    assert int(status.item()) == 0 and counts[1] > 0
    for k in mine:
        assert torch.equal(mine[k][1], theirs[k][1]), k


def test_one_graph_of_4096_vertices(pkg):
    """The only case above a few hundred vertices: a jittered 64 x 64 grid in a random vertex order, degree 4 to 8 - every
    vertex has neighbours all over the 64 words, and V (V - 1) = 16.7 M passes through the index arithmetic."""
    cap, want = _check_case("grid_4096", 0)
    counts = want["counts"].tolist()
    assert counts[0] == 4096 and 8192 <= counts[1] <= 16384 and counts[2] > 4096
    edges = want["x_ind"][want["node_types"] == 1]
    assert int(((edges[:, 1] // 64) - (edges[:, 0] // 64)).max()) > 32


def _relift_capacity(names, vertex_block):
    from csmpn.data.complexes import BatchCapacity
    counts = np.array([CL.reference(n, vertex_block)[4]["counts"].tolist() for n in names]).max(axis=0).tolist()
    return BatchCapacity((counts[0], counts[1] + 3, counts[2] + 2), counts[3] + 7)


@pytest.mark.parametrize("vertex_block", [False, True], ids=["no_block", "block"])
def test_relift_of_a_cloud_batch_needs_no_host(pkg, vertex_block):
    """A V = 96 cloud batch: the second and third relift_ run with synchronisation made an error and allocate nothing; the
    batch then holds the third point set - structure, counts, every table of plan() and the CSR as a fresh device batch has
    them - and refuses the lifts that stop at 64 vertices."""
    from csmpn.data import complexes as cx
    from csmpn_hip import ops
    dev = _dev()
    names = ("relift_96_a", "relift_96_b", "relift_96_c")
    cap = _relift_capacity(names, vertex_block)
    on_dev = [torch.from_numpy(CL.points_of(n)).to(dev) for n in names]
    b = cx.cloud_batch_device(on_dev[0], 2, 1.0, cap, vertex_block=vertex_block)
    assert b._plan["cloud"] == {"vertex_block": vertex_block}
    b.csr().source_order()
    ptrs = {k: getattr(b, k).data_ptr() for k in b._names}
    ws = b._plan["lift_ws"].data_ptr()
    b.relift_(on_dev[1], dis=1.0)                          # the first call allocates the workspaces of the rebuild
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        b.relift_(on_dev[0], dis=1.0)
        b.relift_(on_dev[2], dis=1.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocated
    assert {k: getattr(b, k).data_ptr() for k in b._names} == ptrs and b._plan["lift_ws"].data_ptr() == ws
    assert int(b._plan["lift_status"].item()) == 0 and int(b._plan["status"].item()) == 0
    c = CL.CASES[names[2]]
    want = CL.fast_structure(CL.points_of(names[2]), 2, 1.0, c["max_dim"], vertex_block, cap)
    got = {k: getattr(b, k) for k in CL.STRUCTURE}
    got["counts"] = b._plan["lift_counts"]
    assert CL.differences(got, want) == []
    fresh = cx.SimplicialBatch(**{k: want[k].to(dev) for k in CL.STRUCTURE})
    plan = fresh.plan(2)
    for d in range(3):
        assert torch.equal(b._plan["rows"][d], plan["rows"][d]) and torch.equal(b._plan["verts"][d], plan["verts"][d]), d
    assert torch.equal(b._plan["graph_of_vertex"], plan["graph_of_vertex"])
    csr = fresh.csr()
    for k in ("perm", "src", "dst", "deg", "row_ptr"):
        assert torch.equal(getattr(b._csr, k), getattr(csr, k)), k
    assert ops.get_csr(b.edge_index, cap.rows) is b._csr
    for kw in (dict(knn=3), dict(hull=True), dict(edges=torch.zeros(2, 1, dtype=torch.int64, device=dev)), dict(dis=1.0, edge_th=1.0)):
        with pytest.raises(ValueError, match="64 vertices"):
            b.relift_(on_dev[0], **kw)


def _loss_and_grads(model, batch):
    loss, _ = model(batch)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("vertex_block", [False, True], ids=["no_block", "block"])
def test_md17_model_on_a_cloud_batch_is_bit_identical(pkg, vertex_block):
    """Deterministic mode as test_rips_lift_gpu.py sets it: loss and every parameter gradient of the md17 model on ONE graph of
    70 vertices, on the batch cloud_batch_device lifted and on the host-lifted, padded batch moved to the device - the same
    bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    dev = _dev()
    pts, vf, y, host = CL.md17_cloud_case(1, vertex_block)
    cap = cx.capacity_of([host])
    torch.manual_seed(11)
    model_a = M.MD17SimplicialMPNN().to(dev)
    model_b = copy.deepcopy(model_a)
    with D.deterministic(torch_flag=True, request=True):
        b = cx.cloud_batch_device(torch.from_numpy(pts).to(dev), 1, CL.MD17_DIS, cap, vertex_block=vertex_block, features={"y": y},
                                  vertex_features=vf)
        loss_a, grads_a = _loss_and_grads(model_a, b)
        padded = cx.pad_batch(host, cap, R.MD17_VERTEX_FEATURES)
        for k in CL.STRUCTURE:
            assert torch.equal(getattr(b, k).cpu(), getattr(padded, k)), k
        loss_b, grads_b = _loss_and_grads(model_b, padded.to(dev))
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert sorted(grads_a) == sorted(grads_b) and len(grads_a) > 20
    for k in grads_a:
        assert torch.equal(grads_a[k], grads_b[k]), k


def _cloud_step(cx, GraphedTrainStep, model, opt, cases, cap, dev):
    """One step captured over the cloud batch of cases[0]: (the step, the device copies of every case)."""
    on_dev = [(torch.from_numpy(c[0]).to(dev), {k: v.to(dev) for k, v in c[1].items()}, c[2].to(dev)) for c in cases]
    first = cx.cloud_batch_device(on_dev[0][0], 1, CL.MD17_DIS, cap, vertex_block=True, features={"y": cases[0][2]},
                                  vertex_features=cases[0][1])
    gs = GraphedTrainStep(model, opt, first, ["loc", "vel", "charges", "y"], capacity=cap)
    assert gs.batch is first
    return gs, on_dev


def test_graphed_step_on_a_cloud_batch_matches_eager(pkg):
    """Six steps over three clouds of 70 points: the eager loop on the unpadded host-lifted batches against ONE step captured
    over a cloud batch and fed with step(points=..., dis=...), within the 1e-3 of
    test_graphed_step_on_device_lifted_points_matches_eager, losses and parameters. The optimiser is SGD at lr = 1e-3, because
    at this size the training dynamics amplify ANY difference between two runs from step to step: a padded and an unpadded
    batch round differently (2e-7 of the first loss), and the relative loss differences of the two loops were, on one MI355X,
    1e-7, 7e-5, 3e-4, 3e-4, 1.5e-3, 1.1e-2 under Adam (lr = 1e-3) and 4e-7, 2e-6, 7e-5, 1.4e-3, 2.0e-2, 4.1e-2 under SGD at
    lr = 1e-2 - a factor of 10 per step in the mean (up to 30), i.e. 1 + lr |H| with |H| about 1e3. At lr = 1e-3 that factor is
    about 2 (at most 4), and a rounding difference stays at 1e-5 (at most 4e-4) over six steps, so that the bound tests the step
    and not the conditioning of the trajectory. The device-fed step is not what drifts: under Adam it holds the bits of the host-fed captured step (the test
    below)."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    cases = [CL.md17_cloud_case(s, True) for s in (1, 2, 3)]
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
    gs, on_dev = _cloud_step(cx, GraphedTrainStep, model_g, opt_g, cases, cap, dev)
    for step in range(6):
        pts, vf, y = on_dev[step % 3]
        graphed.append(float(gs.step(features={"y": y}, points=pts, vertex_features=vf, dis=CL.MD17_DIS).detach()))
    assert gs.status() == 0
    eager, graphed = np.asarray(eager), np.asarray(graphed)
    print("eager", eager, "graphed", graphed)
    assert eager[3] != eager[0]                             # the steps did move the parameters
    assert np.all(np.abs(eager - graphed) <= 1e-3 * np.maximum(np.abs(eager), 1e-3)), (eager, graphed)
    for pe, pg in zip(model_e.parameters(), model_g.parameters()):
        assert float((pe - pg).detach().abs().max()) <= 1e-3 * max(float(pe.detach().abs().max()), 1e-2)
    with pytest.raises(ValueError, match="64 vertices"):
        gs.step(points=on_dev[0][0], knn=3)


def test_graphed_adam_step_on_a_cloud_batch_is_the_host_fed_step(pkg):
    """Deterministic mode: six captured Adam steps over the three clouds fed as device points (step(points=..., dis=...) on a
    cloud batch) and fed as host-lifted batches (step(batch=...), the path that existed before) - the same structure bits go
    into the same kernels, so every loss and every final parameter holds the same bits."""
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    dev = _dev()
    cases = [CL.md17_cloud_case(s, True) for s in (1, 2, 3)]
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
            cloud.append(gs_c.step(features={"y": y}, points=pts, vertex_features=vf, dis=CL.MD17_DIS).detach().clone())
            host.append(gs_h.step(batch=cases[step % 3][3]).detach().clone())
        torch.cuda.synchronize()
    assert gs_c.status() == 0 and gs_h.status() == 0
    print("cloud", [float(x) for x in cloud], "host", [float(x) for x in host])
    assert all(torch.equal(a, b) for a, b in zip(cloud, host))
    assert not torch.equal(cloud[0], cloud[3])
    for pc, ph in zip(model_c.parameters(), model_h.parameters()):
        assert torch.equal(pc, ph)
