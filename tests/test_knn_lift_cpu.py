"""The k-nearest-neighbour clique lift, the parts that need no GPU: knn_clique_complex against the reference's simplicial_lift
(complexes_knn_ref.npz, tests/golden/make_knn_complex_golden.py), knn_edges against a brute-force double loop (distinct
distances, ties, coincident points, a NaN vertex, k >= V - 1), lift(vertex_block=...) against the parent's lift,
clique_adjacencies / knn_capacity against collated host batches, the workspace query and every rejected argument combination
of csmpn_knn_lift (checked before the first HIP call), the dis / knn exclusion of relift_ and GraphedTrainStep, the closed
forms of csrc/lift.hip without the vertex block restated on the host against lift(..., vertex_block=False), and a mutation
guard for the comparison the GPU tests use."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import knn_lift_helpers as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_CASES = ["aspirin_21_k3", "nine_k3", "twelve_k2", "complete_6_k5"]
cols = lambda a: sorted(map(tuple, np.asarray(a).T.tolist()))


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_knn_clique_complex_matches_reference_lift(pkg, name):
    """x_d and node_types exactly; every adjacency type as a sorted multiset of columns (the order inside a type is the
    stand-in's enumeration); the big graph's type blocks in the reference's order; no 0_0 pair that no edge joins."""
    from csmpn.data import complexes as cx
    g = np.load(os.path.join(GOLD, "complexes_knn_ref.npz"))
    pts, k = g[f"{name}/points"], int(g[f"{name}/k"])
    c = cx.knn_clique_complex(pts, k, max_dim=2)
    nt = c.node_types.numpy()
    assert np.array_equal(nt, g[f"{name}/node_types"])
    offs = np.concatenate([[0], np.cumsum(np.bincount(nt, minlength=3))])
    for d in range(3):
        assert np.array_equal(c.x_ind.numpy()[nt == d][:, :d + 1], g[f"{name}/x_{d}"]), d
    assert np.array_equal(c.edge_types.numpy(), g[f"{name}/edge_attr"])       # same type blocks in the same order
    ei, ref, et = c.edge_index.numpy(), g[f"{name}/edge_index"], g[f"{name}/edge_attr"]
    assert ei.shape == ref.shape
    ref_types = sorted(key.split("/")[1][4:] for key in g.files if key.startswith(f"{name}/adj_"))
    assert ref_types == sorted({f"{s}_{t}" for s, t in et.tolist()})
    for key in ref_types:
        s_, t_ = int(key[0]), int(key[2])
        m = (et[:, 0] == s_) & (et[:, 1] == t_)
        local = ei[:, m] - np.array([[offs[s_]], [offs[t_]]])
        assert cols(local) == cols(g[f"{name}/adj_{key}"]) == cols(ref[:, m] - np.array([[offs[s_]], [offs[t_]]])), key
    edges = {tuple(e) for e in g[f"{name}/x_1"].tolist()}
    m00 = (et[:, 0] == 0) & (et[:, 1] == 0)
    assert m00.any() and all((min(a, b), max(a, b)) in edges for a, b in ei[:, m00].T.tolist())
    assert ei.shape[1] == cx.clique_adjacencies(len(edges), int((nt == 2).sum()))


def _brute_force_edges(p, k):
    nb = K.brute_force_neighbours(p, k)
    return [(b, a) for a in range(len(nb)) for b in sorted(nb[a])]


KNN_POINTS = {
    "distinct": (lambda: np.random.default_rng(0).standard_normal((13, 3)), 3),
    "lattice": (lambda: np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.float64), 2),
    "coincident": (lambda: np.tile(np.array([[0.5, -1.25, 2.0]]), (6, 1)), 2),
    "nan_vertex": (lambda: K.make_points("nan", 5, 2, 8, 5)[8:].astype(np.float64), 3),
    "k_is_V_minus_1": (lambda: np.random.default_rng(1).standard_normal((5, 3)), 4),
    "k_above_V": (lambda: np.random.default_rng(1).standard_normal((5, 3)), 10),
}


@pytest.mark.parametrize("name", list(KNN_POINTS))
def test_knn_edges_match_brute_force(pkg, name):
    from csmpn.data import complexes as cx
    make, k = KNN_POINTS[name]
    p = make()
    got = cx.knn_edges(p, k)
    assert got.dtype == torch.int64 and got.shape[0] == 2
    want = _brute_force_edges(p, k)
    assert list(map(tuple, got.t().tolist())) == want
    V = len(p)
    assert got.shape[1] == V * min(k, V - 1)                   # every vertex names exactly min(k, V - 1) neighbours
    if name == "coincident":                                   # all ties: the k smallest other indices
        assert [b for b, a in want if a == 4] == [0, 1]
    if name == "nan_vertex":                                   # nobody names the NaN vertex; it names the smallest indices
        assert np.isnan(p[2]).any() and all(b != 2 for b, a in want) and [b for b, a in want if a == 2] == [0, 1, 3]
    if name == "lattice":                                      # corner (0, 0) = vertex 0: (0, 1) = vertex 1 and (1, 0) = vertex 4
        assert [b for b, a in want if a == 0] == [1, 4]
        assert [b for b, a in want if a == 5] == [1, 4]        # interior (1, 1): four neighbours at distance 1, the two smallest
    with pytest.raises(ValueError):
        cx.knn_edges(p, 0)


@pytest.mark.parametrize("name", ["tetra_surface", "strip_with_tail", "octahedron"])
def test_lift_with_vertex_block_is_the_parents_lift(pkg, name):
    """vertex_block=True is the default and the lift pinned by complexes_ref.npz; vertex_block=False differs from it by the
    non-edge pairs of 0_0 alone."""
    from csmpn.data import complexes as cx
    g = np.load(os.path.join(GOLD, "complexes_ref.npz"))
    nv = int(g[f"{name}/n_vertices"])
    tops = [[int(v) for v in row if v >= 0] for row in g[f"{name}/tops"]]
    x_def, a_def = cx.lift(nv, tops, 2)
    x_on, a_on = cx.lift(nv, tops, max_dim=2, vertex_block=True)
    assert sorted(a_def) == sorted(a_on) and all(torch.equal(a_def[k], a_on[k]) for k in a_def)
    assert all(torch.equal(x_def[d], x_on[d]) for d in range(3))
    for k, a in a_on.items():
        assert cols(a.numpy()) == cols(g[f"{name}/adj_{k}"]), k
    x_off, a_off = cx.lift(nv, tops, max_dim=2, vertex_block=False)
    assert all(torch.equal(x_off[d], x_on[d]) for d in range(3)) and sorted(a_off) == sorted(a_on)
    for k in a_on:
        if k != "0_0":
            assert torch.equal(a_off[k], a_on[k]), k
    n1 = int(x_on[1].shape[0])
    assert a_off["0_0"].shape[1] == 2 * n1 and a_on["0_0"].shape[1] == nv * (nv - 1) + n1
    assert torch.equal(a_on["0_0"][:, :2 * n1], a_off["0_0"])  # the shared-edge pairs come first


def test_capacity_counts_adjacencies(pkg):
    """clique_adjacencies is edge_index.shape[1] of the collated host batches of every device case; knn_capacity holds them,
    its default edge bound included."""
    from csmpn.data import complexes as cx
    for name, (B, verts, _, k, max_dim, _, _, _) in K.CASES.items():
        pts, _, _, _, want = K.reference(name)
        c = want["counts"].tolist()
        n1, n2 = c[1], c[2] if max_dim == 2 else 0
        assert cx.clique_adjacencies(n1, n2) == c[-1] == 6 * n1 + 12 * n2, name
        assert n1 <= B * min(k * verts, verts * (verts - 1) // 2), name
        cap = cx.knn_capacity(B, verts, k, n2, max_edges=n1, max_dim=max_dim)
        assert cap.simplices == (B * verts, n1 + 1) + ((n2,) if max_dim == 2 else ()) and cap.edges == c[-1], name
        cx.pad_batch(K.host_lift(pts, B, k, max_dim), cap)     # the spare 1-simplex is there, so this never refuses
        bound = cx.knn_capacity(B, verts, k, n2, max_dim=max_dim)
        assert bound.simplices[0] == B * verts and bound.max_dim == max_dim
        assert bound.simplices[1] == B * min(k * verts, verts * (verts - 1) // 2) + 1
        assert bound.edges == cx.clique_adjacencies(bound.simplices[1] - 1, n2)
        cx.pad_batch(K.host_lift(pts, B, k, max_dim), bound)
    assert cx.knn_capacity(16, 21, 3, 500).simplices == (336, 16 * 63 + 1, 500)
    for bad in (dict(max_dim=3), dict(verts_per_graph=2), dict(k=0), dict(max_triangles=-1), dict(n_graphs=0)):
        a = dict(n_graphs=4, verts_per_graph=6, k=3, max_triangles=5)
        a.update(bad)
        with pytest.raises(ValueError):
            cx.knn_capacity(**a)


def test_workspace_query(pkg):
    from csmpn_hip import native
    q = native.lib().csmpn_knn_lift_workspace_bytes
    sizes = [int(q(b, 13, 2)) for b in (1, 16, 300, 5000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert int(q(16, 64, 2)) > 0 and int(q(16, 2, 1)) > 0
    assert int(q(16, 65, 2)) == 0 and int(q(16, 13, 0)) == 0 and int(q(16, 13, 3)) == 0
    assert int(q(0, 13, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q(1 << 31, 13, 2)) == 0
    assert int(q(16, 21, 2)) == int(native.lib().csmpn_rips_lift_workspace_bytes(16, 21, 2))


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call


def _call(lib, **over):
    """csmpn_knn_lift for 4 graphs of 6 vertices in R^3, k = 3, max_dim 2, with the named arguments replaced."""
    a = dict(points=FAKE, point_dim=3, n_graphs=4, verts=6, k=3, max_dim=2, cap=(24, 28, 13), cap_edges=384, x_ind=FAKE,
             x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE, x_ind_ptr=FAKE, edge_index=FAKE,
             edge_types=FAKE, counts=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_knn_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["k"], a["max_dim"],
                              None if cap is None else C.addressof(cap), a["cap_edges"], a["x_ind"], a["x_ind_cols"],
                              a["node_types"], a["batch"], a["x_ind_batch"], a["ptr"], a["x_ind_ptr"], a["edge_index"],
                              a["edge_types"], a["counts"], a["status"], a["workspace"], a["workspace_bytes"], None)


REJECTED = [
    ("k_0", dict(k=0), "invalid"),
    ("k_negative", dict(k=-2), "invalid"),
    ("max_dim_negative", dict(max_dim=-1), "invalid"),
    ("max_dim_0", dict(max_dim=0, cap=(24,), x_ind_cols=1), "unsupported"),
    ("max_dim_3", dict(max_dim=3, cap=(24, 28, 13, 1), x_ind_cols=4), "unsupported"),
    ("65_vertices", dict(verts=65, cap=(260, 28, 13)), "unsupported"),
    ("too_few_vertices", dict(verts=2, cap=(8, 28, 13)), "invalid"),
    ("too_few_vertices_max_dim_1", dict(verts=1, max_dim=1, cap=(4, 28)), "invalid"),
    ("no_graph", dict(n_graphs=0), "invalid"),
    ("negative_graphs", dict(n_graphs=-3), "invalid"),
    ("vertices_past_int32", dict(n_graphs=(1 << 31) // 6 + 1), "invalid"),
    ("point_dim_0", dict(point_dim=0), "invalid"),
    ("x_ind_too_narrow", dict(x_ind_cols=2), "invalid"),
    ("vertex_capacity_differs", dict(cap=(25, 28, 13)), "invalid"),
    ("negative_row_capacity", dict(cap=(24, -1, 13)), "invalid"),
    ("rows_past_int32", dict(cap=(24, (1 << 31) - 30, 13)), "invalid"),
    ("negative_edge_capacity", dict(cap_edges=-1), "invalid"),
    ("edges_past_int32", dict(cap_edges=1 << 31), "invalid"),
    ("no_workspace", dict(workspace=None), "invalid"),
    ("workspace_too_small", dict(workspace_bytes=64), "invalid"),
    ("no_capacity", dict(cap=None), "invalid"),
] + [(f"null_{name}", {name: None}, "invalid") for name in
     ("points", "x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr", "edge_index")]


@pytest.mark.parametrize("name,over,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments(pkg, name, over, code):
    from csmpn_hip import native
    lib = native.lib()
    want = {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[code]
    assert _call(lib, **over) == want
    assert lib.csmpn_last_error()                       # a message says why


def test_threshold_and_k_are_checked_where_dis_always_was(pkg):
    """A bad k (a bad dis in the Rips entry) together with an unsupported shape reports the shape, as csmpn_rips_lift did
    before the two entries shared their checks; together with a later finding it is reported itself."""
    import test_rips_lift_cpu as R
    from csmpn_hip import native
    lib = native.lib()
    assert _call(lib, k=0, max_dim=3, cap=(24, 28, 13, 1), x_ind_cols=4) == native.ERR_UNSUPPORTED
    assert _call(lib, k=0, verts=65, cap=(260, 28, 13)) == native.ERR_UNSUPPORTED
    assert _call(lib, k=0, x_ind_cols=2) == native.ERR_INVALID and b"k = 0" in lib.csmpn_last_error()
    assert R._call(lib, dis=-1.0, max_dim=3, cap=(24, 28, 13, 1), x_ind_cols=4) == native.ERR_UNSUPPORTED
    assert R._call(lib, dis=float("nan"), verts=65, cap=(260, 28, 13)) == native.ERR_UNSUPPORTED
    assert R._call(lib, dis=-1.0, x_ind_cols=2) == native.ERR_INVALID and b"dis" in lib.csmpn_last_error()


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.knn_lift(torch.zeros(24, 3), 4, 3, 2, (24, 28, 13), 384, i64(65, 3), i64(65), i64(65), i64(65), i64(5), i64(5),
                     i64(2, 384), None, None, None, torch.zeros(4096, dtype=torch.uint8))


def test_dis_and_knn_exclude_each_other(pkg):
    """relift_, load_points and step refuse both and neither before they touch the device; so does a step built with both
    defaults. (The step object is made without its constructor: capturing needs a GPU, the argument rule does not.)"""
    from csmpn.data import complexes as cx
    from csmpn_hip.graphed import GraphedTrainStep
    b = K.host_lift(K.make_points("normal", 0, 2, 5, 3), 2, 2, 2)
    pts = torch.zeros(10, 3)
    with pytest.raises(ValueError, match="exactly one"):
        b.relift_(pts, 1.0, knn=3)
    with pytest.raises(ValueError, match="exactly one"):
        b.relift_(pts)
    with pytest.raises(ValueError, match="exactly one"):
        b.relift_(pts, None, None, None)
    with pytest.raises(RuntimeError):                          # one of the two: accepted, and the missing plan is the next finding
        b.relift_(pts, 1.0, None)
    with pytest.raises(RuntimeError):
        b.relift_(pts, knn=3)
    with pytest.raises(ValueError, match="exclude"):
        GraphedTrainStep(None, None, None, [], rips_dis=1.0, knn=3)
    for defaults in (dict(rips_dis=None, knn=None), dict(rips_dis=1.6, knn=None), dict(rips_dis=None, knn=3)):
        gs = object.__new__(GraphedTrainStep)
        gs.capacity = cx.BatchCapacity((10, 5, 2), 40)
        gs.__dict__.update(defaults)
        with pytest.raises(ValueError, match="exclude"):
            gs.load_points(pts, dis=1.0, knn=3)
        with pytest.raises(ValueError, match="exclude"):
            gs.step(points=pts, dis=1.0, knn=3)
    gs = object.__new__(GraphedTrainStep)
    gs.capacity, gs.rips_dis, gs.knn = cx.BatchCapacity((10, 5, 2), 40), None, None
    with pytest.raises(ValueError, match="pass dis"):
        gs.load_points(pts)
    with pytest.raises(ValueError, match="pass dis"):
        gs.step(points=pts)


@pytest.mark.parametrize("name", list(K.CASES))
def test_closed_forms_match_host_lift(pkg, name):
    """Every position the kernels compute from popcounts and scans, block 3 directly behind block 1
    (knn_lift_helpers.closed_form_structure), is the position lift(..., vertex_block=False) + to_complex() + collate() +
    pad_batch() give - with the masks of the double-loop neighbour rule, not of knn_edges."""
    pts, k, max_dim, cap, want = K.reference(name)
    got = K.closed_form_structure(pts, K.CASES[name][0], k, max_dim, cap)
    assert K.differences(got, want) == []


def test_cases_reach_what_they_are_for(pkg):
    """The outliers of the 3 x 64 case are named by nobody, so their mask bits come from the transposed step alone; k = 1
    leaves no triangle; the complete cases are complete; the exact capacity leaves no filler."""
    pts, k, _, _, want = K.reference("all_mask_bits_3x64")
    p = pts.astype(np.float64).reshape(3, 64, 3)
    for g in range(3):
        nb = K.brute_force_neighbours(p[g], k)
        assert all(0 not in nb[a] and 63 not in nb[a] for a in range(64))
        masks = K.knn_masks(p[g], k)
        assert bin(masks[0]).count("1") == 3 and bin(masks[63]).count("1") == 3
        assert all((masks[b] >> 0) & 1 for b in nb[0]) and all((masks[b] >> 63) & 1 for b in nb[63])
    edges = want["x_ind"][want["node_types"] == 1]
    assert int(edges[:, 0].min()) == 0 and int(edges[:, 1].max()) == 63
    assert K.reference("mask_halves_2x33_k1")[4]["counts"][2] == 0
    assert K.reference("second_scan_pass_300x4")[4]["counts"][2] == 0
    for name in ("complete_2x5_k4", "complete_2x5_k10"):
        assert K.reference(name)[4]["counts"].tolist() == [10, 20, 20, 6 * 20 + 12 * 20]
    assert K.differences(K.reference("complete_2x5_k4")[4], K.reference("complete_2x5_k10")[4]) == []
    _, _, _, cap, want = K.reference("exact_capacity_16x21")
    assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on."""
    _, _, _, cap, want = K.reference("aspirin_16x21")
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert K.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert K.differences(swapped, want) == ["edge_index"]
    wrong_ptr = clone()                                    # one wrong ptr entry
    wrong_ptr["ptr"][2] += 1
    assert K.differences(wrong_ptr, want) == ["ptr"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert K.differences(filler, want) == ["node_types"]
    missing_edge = clone()                                 # one directed neighbour dropped: another x_ind row
    row = int((want["node_types"] == 1).nonzero()[0])
    missing_edge["x_ind"][row, 1] += 1
    assert K.differences(missing_edge, want) == ["x_ind"]
    narrower = clone()                                     # ... and shapes and dtypes count
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert K.differences(narrower, want) == ["batch"]
    bufs = K.buffers(cap, 16, torch.device("cpu"))         # the guard check sees one written guard word
    assert K.guards_intact(bufs) is None
    bufs["ptr"][1][-1] = 0
    assert K.guards_intact(bufs) == "ptr"
