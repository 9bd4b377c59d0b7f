"""The convex-hull lift, the parts that need no GPU: hull_facets against scipy's qhull (hull_facets_ref.npz,
tests/golden/make_hull_facets_golden.py; live as well where scipy imports) and against the rule restated with plain Python
floats, bit for bit; degenerate inputs with their answers by hand; hull_complex's two methods; the closed forms of
csrc/lift.hip with the facet table T restated on the host against lift(); hull_capacity against collated host batches; the
workspace query and every rejected argument combination of csmpn_hull_lift (checked before the first HIP call) with their
place among the shared checks; the three-way exclusion of relift_ and GraphedTrainStep; and a mutation guard for the
comparison the GPU tests use."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest
import torch

import hull_lift_helpers as H

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHAPES = [(8, 5), (8, 4), (8, 3), (7, 2), (6, 5), (16, 5), (12, 3), (9, 4)]
FIXTURE_CASES = [f"v{V}_n{n}_s{seed}" for V, n in SHAPES for seed in range(4)]


def _smallest_side(p):
    """min over the candidates F and the vertices q outside F of |det [p_f1 - p_f0; ...; q - p_f0]| (numpy's determinant: an
    independent route to |side(F, q)|, good to ~1e-15 of its size - the condition asks for 1e-9)."""
    V, n = p.shape
    cand = np.array(list(itertools.combinations(range(V), n)))
    rows = p[cand[:, 1:]] - p[cand[:, :1]]                                   # [C, n - 1, n]
    smallest = math.inf
    for q in range(V):
        last = (p[q][None, :] - p[cand[:, 0]])[:, None, :]
        d = np.abs(np.linalg.det(np.concatenate([rows, last], axis=1)))
        smallest = min(smallest, float(d[~(cand == q).any(axis=1)].min()))
    return smallest


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_hull_facets_match_scipy(pkg, name):
    """On Gaussian points (every |side| of every candidate above 1e-9: general position) the facet set is scipy's and the
    volume agrees to 1e-9 relative (1.5e-14 measured) - from the committed fixture, and live where scipy imports."""
    from csmpn.data import complexes as cx
    g = np.load(os.path.join(GOLD, "hull_facets_ref.npz"))
    pts = g[f"{name}/points"]
    assert _smallest_side(pts) > 1e-9
    facets, volume = cx.hull_facets(pts)
    assert facets.dtype == np.int64 and np.array_equal(facets, g[f"{name}/facets"])
    want = float(g[f"{name}/volume"])
    assert abs(volume - want) <= 1e-9 * want
    try:
        from scipy.spatial import ConvexHull
    except ImportError:
        return
    hull = ConvexHull(pts)
    assert sorted(map(tuple, np.sort(hull.simplices, axis=1).tolist())) == list(map(tuple, facets.tolist()))
    assert abs(volume - hull.volume) <= 1e-9 * hull.volume


def test_fixture_covers_the_shapes(pkg):
    g = np.load(os.path.join(GOLD, "hull_facets_ref.npz"))
    shapes = {tuple(g[k].shape) for k in g.files if k.endswith("/points")}
    assert shapes >= {(8, 5), (8, 4), (8, 3), (7, 2), (6, 5), (16, 5), (12, 3)}
    assert sorted({k.split("/")[0] for k in g.files}) == sorted(FIXTURE_CASES)


@pytest.mark.parametrize("shape", [(8, 5), (6, 5), (7, 2), (12, 3), (9, 4), (16, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hull_facets_is_the_rule_in_plain_floats(pkg, shape):
    """hull_facets (numpy, all candidates at once) against the rule candidate by candidate in Python floats: the same facets
    and the same volume to the bit - the order of operations is the stated one, not numpy's choice."""
    from csmpn.data import complexes as cx
    V, n = shape
    p = np.random.default_rng(7 * V + n).standard_normal((V, n)).astype(np.float32).astype(np.float64)
    facets, volume = cx.hull_facets(p)
    want, smallest = H.brute_force_facets(p)
    assert list(map(tuple, facets.tolist())) == want and smallest > 1e-9
    assert volume == H.brute_force_volume(p) and volume > 0


def test_degenerate_inputs(pkg):
    """Answers by hand. A zero or a NaN side value makes a candidate no facet; what qhull makes of such input is not restated."""
    from csmpn.data import complexes as cx
    facets = lambda p: list(map(tuple, cx.hull_facets(np.asarray(p, dtype=np.float64))[0].tolist()))
    # unit-cube corners: every plane through three corners holds a fourth one or cuts the cube
    assert facets(H.CUBE) == [] and cx.hull_facets(H.CUBE)[1] == 0.0
    # square pyramid: the base (0, 1, 2, 3) is coplanar, so none of its four triples is a facet; the four sides are
    assert facets(H.PYRAMID) == [(0, 1, 4), (0, 3, 4), (1, 2, 4), (2, 3, 4)]
    assert cx.hull_facets(H.PYRAMID)[1] == pytest.approx(1.0 / 3.0, rel=1e-15)     # apex p_0 lies in the missing base
    assert facets(np.tile([[0.5, -1.25, 2.0]], (6, 1))) == []
    nan = H.make_points("nan", 10, 2, 8, 5)[8:]
    assert np.isnan(nan).sum() == 1 and facets(nan) == [] and cx.hull_facets(nan)[1] == 0.0
    for V, n in ((3, 2), (4, 3), (5, 4), (6, 5)):                                  # V = n + 1: a simplex, every subset a facet
        p = np.random.default_rng(V).standard_normal((V, n))
        assert facets(p) == list(itertools.combinations(range(V), n))
    inner = H.split(H.make_points("interior", 11, 2, 6, 3), 2)[0]
    got = facets(inner)
    assert got and all(4 not in F for F in got)
    c = cx.hull_complex(inner, 2, method="exact")                                  # ... an isolated vertex of the complex
    assert int((c.node_types == 0).sum()) == 6 and not bool((c.x_ind[c.node_types >= 1] == 4).any())
    for bad in (np.zeros((5, 5)), np.zeros((4, 1)), np.zeros(7)):
        with pytest.raises(ValueError):
            cx.hull_facets(bad)


def test_hull_complex_methods(pkg):
    """The default is qhull, as before; on points in general position "exact" gives the same complex; another name is refused."""
    pytest.importorskip("scipy")
    from csmpn.data import complexes as cx
    p = np.random.default_rng(3).standard_normal((8, 5)).astype(np.float32)
    a, b, c = cx.hull_complex(p), cx.hull_complex(p, 2, method="qhull"), cx.hull_complex(p, 2, method="exact")
    for other in (b, c):
        for k in ("x_ind", "node_types", "edge_index", "edge_types"):
            assert torch.equal(getattr(a, k), getattr(other, k)), k
    with pytest.raises(ValueError):
        cx.hull_complex(p, 2, method="joggled")


@pytest.mark.parametrize("name", list(H.CASES))
def test_closed_forms_match_host_lift(pkg, name):
    """Every position the kernels compute from popcounts and scans, with an edge's triangles and cofaces read from the facet
    table T (hull_lift_helpers.closed_form_structure), is the position lift() + to_complex() + collate() + pad_batch() give -
    with the facets of the candidate-by-candidate rule, not of hull_facets."""
    pts, max_dim, cap, want, _ = H.reference(name)
    got = H.closed_form_structure(pts, H.CASES[name][0], max_dim, cap)
    assert H.differences(got, want) == []


def _cliques_and_triangles(name):
    want = H.reference(name)[3]
    B, V = H.CASES[name][:2]
    out = []
    for g in range(B):
        rows = slice(int(want["ptr"][g]), int(want["ptr"][g + 1]))
        x, t = want["x_ind"][rows], want["node_types"][rows]
        edges = {tuple(e) for e in x[t == 1][:, :2].tolist()}
        cliques = sum(1 for s in itertools.combinations(range(V), 3) if all(p in edges for p in itertools.combinations(s, 2)))
        out.append((len(edges), cliques, int((t == 2).sum())))
    return out


def test_cases_reach_what_they_are_for(pkg):
    """The task's shape has triples whose three pairs are edges and which are no 2-simplex (the one place where this is not a
    clique complex); V = n + 1 is complete; the plane has no triangle and interior vertices; the degenerate graphs have
    nothing but vertices; the exact capacity leaves no filler."""
    counts = _cliques_and_triangles("task_3x8_r5") + _cliques_and_triangles("strides_1x16_r5")
    assert any(cliques > triangles for _, cliques, triangles in counts), counts
    assert all(cliques >= triangles for _, cliques, triangles in counts)
    assert _cliques_and_triangles("all_subsets_2x6_r5") == [(15, 20, 20)] * 2
    plane = H.reference("plane_2x7_r2")[3]
    assert int(plane["counts"][2]) == 0 and int(plane["counts"][1]) < 2 * 7
    assert _cliques_and_triangles("cube_2x8_r3")[0] == (0, 0, 0) and _cliques_and_triangles("cube_2x8_r3")[1][0] > 0
    assert _cliques_and_triangles("pyramid_2x5_r3")[0] == (8, 4, 4)
    assert H.reference("coincident_2x6_r3")[3]["counts"].tolist() == [12, 0, 0, 2 * 6 * 5]
    assert _cliques_and_triangles("nan_2x8_r5")[1] == (0, 0, 0) and _cliques_and_triangles("nan_2x8_r5")[0][0] > 0
    assert H.reference("second_scan_pass_300x5_r4")[3]["counts"].tolist()[:3] == [1500, 3000, 3000]
    _, _, cap, want, vols = H.reference("exact_capacity_3x8_r5")
    assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    assert np.all(vols > 0) and H.reference("cube_2x8_r3")[4][0] == 0.0


def test_capacity_counts_adjacencies(pkg):
    """rips_adjacencies is edge_index.shape[1] of the collated host batches of every device case; hull_capacity holds them,
    its default bounds included, with the spare 1-simplex."""
    from csmpn.data import complexes as cx
    for name, (B, V, _, max_dim, _, _, _) in H.CASES.items():
        pts, _, _, want, _ = H.reference(name)
        c = want["counts"].tolist()
        n1, n2 = c[1], c[2] if max_dim == 2 else 0
        assert cx.rips_adjacencies(B, V, n1, n2) == c[-1], name
        cap = cx.hull_capacity(B, V, max_dim, max_edges=n1, max_triangles=n2)
        assert cap.simplices == (B * V, n1 + 1) + ((n2,) if max_dim == 2 else ()) and cap.edges == c[-1], name
        cx.pad_batch(H.host_lift(pts, B, max_dim), cap)
        bound = cx.hull_capacity(B, V, max_dim)
        assert bound.simplices == (B * V, B * math.comb(V, 2) + 1) + ((B * math.comb(V, 3),) if max_dim == 2 else ())
        assert bound.edges == cx.rips_adjacencies(B, V, B * math.comb(V, 2), B * math.comb(V, 3) if max_dim == 2 else 0)
        cx.pad_batch(H.host_lift(pts, B, max_dim), bound)
    assert cx.hull_capacity(16, 8).simplices == (128, 16 * 28 + 1, 16 * 56)
    for bad in (dict(max_dim=3), dict(verts_per_graph=2), dict(max_edges=-1), dict(max_triangles=-1), dict(n_graphs=0)):
        a = dict(n_graphs=4, verts_per_graph=6)
        a.update(bad)
        with pytest.raises(ValueError):
            cx.hull_capacity(**a)


def test_workspace_query(pkg):
    from csmpn_hip import native
    q = native.lib().csmpn_hull_lift_workspace_bytes
    sizes = [int(q(b, 8, 2)) for b in (1, 16, 300, 5000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert int(q(16, 16, 2)) > 0 and int(q(16, 3, 1)) > 0
    assert int(q(16, 17, 2)) == 0 and int(q(16, 8, 0)) == 0 and int(q(16, 8, 3)) == 0
    assert int(q(0, 8, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q(1 << 31, 8, 2)) == 0
    # the facet tables and the volumes come on top of what the other two lifts need
    assert int(q(16, 8, 2)) > int(native.lib().csmpn_rips_lift_workspace_bytes(16, 8, 2)) + 16 * 8 * 8 * 8


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call


def _call(lib, **over):
    """csmpn_hull_lift for 4 graphs of 8 vertices in R^5, max_dim 2, with the named arguments replaced."""
    a = dict(points=FAKE, point_dim=5, n_graphs=4, verts=8, max_dim=2, cap=(32, 113, 224), cap_edges=3500, x_ind=FAKE,
             x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE, x_ind_ptr=FAKE, edge_index=FAKE,
             edge_types=FAKE, counts=FAKE, status=FAKE, volume=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_hull_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["max_dim"],
                               None if cap is None else C.addressof(cap), a["cap_edges"], a["x_ind"], a["x_ind_cols"],
                               a["node_types"], a["batch"], a["x_ind_batch"], a["ptr"], a["x_ind_ptr"], a["edge_index"],
                               a["edge_types"], a["counts"], a["status"], a["volume"], a["workspace"], a["workspace_bytes"], None)


REJECTED = [
    ("point_dim_1", dict(point_dim=1), "unsupported"),
    ("point_dim_6", dict(point_dim=6), "unsupported"),
    ("point_dim_0", dict(point_dim=0), "invalid"),
    ("point_dim_negative", dict(point_dim=-2), "invalid"),
    ("vertices_equal_point_dim", dict(verts=5, cap=(20, 113, 224)), "invalid"),
    ("vertices_below_point_dim", dict(verts=4, cap=(16, 113, 224)), "invalid"),
    ("17_vertices", dict(verts=17, cap=(68, 113, 224)), "unsupported"),
    ("65_vertices", dict(verts=65, cap=(260, 113, 224)), "unsupported"),
    ("max_dim_negative", dict(max_dim=-1), "invalid"),
    ("max_dim_0", dict(max_dim=0, cap=(32,), x_ind_cols=1), "unsupported"),
    ("max_dim_3", dict(max_dim=3, cap=(32, 113, 224, 1), x_ind_cols=4), "unsupported"),
    ("too_few_vertices", dict(verts=2, point_dim=2, cap=(8, 113, 224)), "invalid"),
    ("no_graph", dict(n_graphs=0), "invalid"),
    ("negative_graphs", dict(n_graphs=-3), "invalid"),
    ("vertices_past_int32", dict(n_graphs=(1 << 31) // 8 + 1), "invalid"),
    ("x_ind_too_narrow", dict(x_ind_cols=2), "invalid"),
    ("vertex_capacity_differs", dict(cap=(33, 113, 224)), "invalid"),
    ("negative_row_capacity", dict(cap=(32, -1, 224)), "invalid"),
    ("rows_past_int32", dict(cap=(32, (1 << 31) - 40, 224)), "invalid"),
    ("negative_edge_capacity", dict(cap_edges=-1), "invalid"),
    ("edges_past_int32", dict(cap_edges=1 << 31), "invalid"),
    ("no_workspace", dict(workspace=None), "invalid"),
    ("workspace_too_small", dict(workspace_bytes=64), "invalid"),
    ("workspace_of_the_rips_lift", dict(workspace_bytes=None), "invalid"),
    ("no_capacity", dict(cap=None), "invalid"),
] + [(f"null_{name}", {name: None}, "invalid") for name in
     ("points", "x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr", "edge_index")]


@pytest.mark.parametrize("name,over,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments(pkg, name, over, code):
    from csmpn_hip import native
    lib = native.lib()
    if name == "workspace_of_the_rips_lift":               # enough for the other two lifts, not for this one
        over = dict(workspace_bytes=int(lib.csmpn_rips_lift_workspace_bytes(4, 8, 2)))
    want = {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[code]
    assert _call(lib, **over) == want
    assert lib.csmpn_last_error()                       # a message says why


def test_checks_stand_where_the_shared_ones_do(pkg):
    """The 16-vertex limit is reported where the other entries report their 64; the point dimension where csmpn_rips_lift has
    always checked dis - behind the shapes, in front of x_ind_cols, the pointers, the capacity and the workspace; NULL for the
    volume, the edge types, the counts and the status is accepted as far as the checks go."""
    from csmpn_hip import native
    lib = native.lib()
    assert _call(lib, verts=17, max_dim=3, cap=(68, 113, 224, 1), x_ind_cols=4) == native.ERR_UNSUPPORTED
    assert b"max_dim" in lib.csmpn_last_error()
    assert _call(lib, verts=17, max_dim=-1) == native.ERR_INVALID
    assert _call(lib, verts=17, n_graphs=0) == native.ERR_UNSUPPORTED and b"17 vertices" in lib.csmpn_last_error()
    assert _call(lib, point_dim=6, verts=65, cap=(260, 113, 224)) == native.ERR_UNSUPPORTED and b"65 vertices" in lib.csmpn_last_error()
    assert _call(lib, point_dim=6, n_graphs=0) == native.ERR_INVALID and b"n_graphs" in lib.csmpn_last_error()
    assert _call(lib, point_dim=6, x_ind_cols=2) == native.ERR_UNSUPPORTED and b"R^6" in lib.csmpn_last_error()
    assert _call(lib, verts=5, cap=(20, 113, 224), points=None) == native.ERR_INVALID and b"R^5" in lib.csmpn_last_error()
    assert _call(lib, point_dim=1, workspace=None) == native.ERR_UNSUPPORTED
    # everything in order up to the workspace: the last check is the one that answers
    assert _call(lib, volume=None, edge_types=None, counts=None, status=None, workspace_bytes=64) == native.ERR_INVALID
    assert b"workspace" in lib.csmpn_last_error()


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.hull_lift(torch.zeros(32, 5), 4, 2, (32, 113, 224), 3500, i64(369, 3), i64(369), i64(369), i64(369), i64(5), i64(5),
                      i64(2, 3500), None, None, None, torch.zeros(4096, dtype=torch.uint8), volume=torch.zeros(4))


def test_dis_knn_and_hull_exclude_each_other(pkg):
    """relift_, load_points and step refuse two or three of the choices, and none, before they touch the device; so does a step
    built with two defaults. (The step object is made without its constructor: capturing needs a GPU, the rule does not.)"""
    from csmpn.data import complexes as cx
    from csmpn_hip.graphed import GraphedTrainStep
    b = H.host_lift(H.make_points("normal", 0, 2, 6, 3), 2, 2)
    pts = torch.zeros(12, 3)
    for bad in (dict(dis=1.0, hull=True), dict(knn=3, hull=True), dict(dis=1.0, knn=3, hull=True), dict(dis=1.0, knn=3), dict(),
                dict(hull=False)):
        with pytest.raises(ValueError, match="exactly one"):
            b.relift_(pts, **bad)
    for one in (dict(dis=1.0), dict(knn=3), dict(hull=True)):      # one of the three: accepted, the missing plan is the next finding
        with pytest.raises(RuntimeError):
            b.relift_(pts, **one)
    for bad in (dict(rips_dis=1.0, hull=True), dict(knn=3, hull=True), dict(rips_dis=1.0, knn=3, hull=True)):
        with pytest.raises(ValueError, match="exclude"):
            GraphedTrainStep(None, None, None, [], **bad)
    for defaults in (dict(rips_dis=None, knn=None, hull=False), dict(rips_dis=1.6, knn=None, hull=False),
                     dict(rips_dis=None, knn=3, hull=False), dict(rips_dis=None, knn=None, hull=True)):
        gs = object.__new__(GraphedTrainStep)
        gs.capacity = cx.BatchCapacity((12, 5, 2), 40)
        gs.__dict__.update(defaults)
        for bad in (dict(dis=1.0, hull=True), dict(knn=3, hull=True), dict(dis=1.0, knn=3, hull=True)):
            with pytest.raises(ValueError, match="exclude"):
                gs.load_points(pts, **bad)
            with pytest.raises(ValueError, match="exclude"):
                gs.step(points=pts, **bad)
    gs = object.__new__(GraphedTrainStep)
    gs.capacity, gs.rips_dis, gs.knn = cx.BatchCapacity((12, 5, 2), 40), None, None      # a step from before `hull` existed
    assert gs.hull is False
    with pytest.raises(ValueError, match="pass dis"):
        gs.load_points(pts)
    with pytest.raises(ValueError, match="pass dis"):
        gs.step(points=pts, hull=False)


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on."""
    _, _, cap, want, _ = H.reference("task_3x8_r5")
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert H.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert H.differences(swapped, want) == ["edge_index"]
    wrong_ptr = clone()                                    # one wrong ptr entry
    wrong_ptr["ptr"][2] += 1
    assert H.differences(wrong_ptr, want) == ["ptr"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert H.differences(filler, want) == ["node_types"]
    clique = clone()                                       # a triangle that is a clique but lies in no facet: another x_ind row
    row = int((want["node_types"] == 2).nonzero()[0])
    clique["x_ind"][row, 2] += 1
    assert H.differences(clique, want) == ["x_ind"]
    one_more = clone()                                     # ... and one more coface of an edge: another count
    one_more["counts"][2] += 1
    assert H.differences(one_more, want) == ["counts"]
    narrower = clone()                                     # shapes and dtypes count
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert H.differences(narrower, want) == ["batch"]
    bufs = H.buffers(cap, 3, torch.device("cpu"))          # the guard check sees one written guard word
    assert H.guards_intact(bufs) is None
    bufs["ptr"][1][-1] = 0
    assert H.guards_intact(bufs) == "ptr"
    # the volume comparison of the GPU tests: one float32 spacing of the host's double value, no more
    v = H.reference("task_3x8_r5")[4]
    near = v.astype(np.float32)
    assert np.all(np.abs(near.astype(np.float64) - v) <= np.spacing(np.abs(near)))
    far = np.nextafter(np.nextafter(near, np.float32(np.inf)), np.float32(np.inf))
    assert not np.all(np.abs(far.astype(np.float64) - v) <= np.spacing(np.abs(far)))
