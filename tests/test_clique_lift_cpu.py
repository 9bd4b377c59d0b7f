"""The thresholded clique lift, the parts that need no GPU: clique_complex against the reference's simplicial_lift with finite
edge_th / tri_th (complexes_th_ref.npz, tests/golden/make_thresholded_complex_golden.py), the fixture's conditioning and its
coverage recomputed, clique_complex on a kNN list against knn_clique_complex, ties on an integer lattice, a NaN vertex, the rule
restated as loops over masks and the closed forms of csrc/lift.hip with the table T against lift(), clique_capacity, the
workspace query, every rejected argument combination of csmpn_clique_lift and its place among the shared checks, the exclusion
rules of relift_ and GraphedTrainStep, and a mutation guard for the comparison the GPU tests use."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import clique_lift_helpers as Q

INF = math.inf
cols = lambda a: sorted(map(tuple, np.asarray(a).T.tolist()))
FIXTURE_CASES = Q.fixture_cases() if os.path.exists(os.path.join(Q.GOLD, "complexes_th_ref.npz")) else []


def test_fixture_holds_the_cases_of_the_issue():
    assert len(FIXTURE_CASES) == 22 and sum(c.startswith("knn_") for c in FIXTURE_CASES) == 20
    assert sum(c.startswith("ring_13_chords") for c in FIXTURE_CASES) == 2


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_clique_complex_matches_reference_lift(pkg, name):
    """x_d and node_types exactly; every adjacency type as a sorted multiset of columns (the order inside a type is the
    stand-in's enumeration); the big graph's type blocks in the reference's order; 6 n1 + 12 n2 adjacencies."""
    from csmpn.data import complexes as cx
    g = Q.fixture()
    pts, edges = g[f"{name}/points"], g[f"{name}/edges"]
    c = cx.clique_complex(pts, edges, float(g[f"{name}/edge_th"]), float(g[f"{name}/tri_th"]), max_dim=2)
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
    n1, n2 = len(g[f"{name}/x_1"]), len(g[f"{name}/x_2"])
    sizes = {"0_0": 2 * n1, "1_1": 6 * n2, "0_1": 2 * n1, "1_0": 2 * n1, "1_2": 3 * n2, "2_1": 3 * n2}
    for key in ref_types:
        s_, t_ = int(key[0]), int(key[2])
        m = (et[:, 0] == s_) & (et[:, 1] == t_)
        local = ei[:, m] - np.array([[offs[s_]], [offs[t_]]])
        assert cols(local) == cols(g[f"{name}/adj_{key}"]) == cols(ref[:, m] - np.array([[offs[s_]], [offs[t_]]])), key
        assert local.shape[1] == sizes[key], key
    assert ei.shape[1] == cx.clique_adjacencies(n1, n2) == 6 * n1 + 12 * n2


def test_fixture_is_well_conditioned_and_not_blind():
    """Every threshold keeps a relative 1e-4 from every edge length and triangle area of its G (float32 in the reference and
    float64 here cannot disagree); at least 10 cases have a triple of 1-simplices that bounds no 2-simplex and at least 10 an
    edge that a triangle brought back (the generator printed 14 and 17)."""
    g = Q.fixture()
    hollow_cases = back_cases = 0
    for name in FIXTURE_CASES:
        pts, edges = g[f"{name}/points"], g[f"{name}/edges"]
        edge_th, tri_th = float(g[f"{name}/edge_th"]), float(g[f"{name}/tri_th"])
        pairs, lengths, _, areas = Q.graph_values(pts, edges)
        assert Q.relative_gap(edge_th, lengths) >= Q.MIN_GAP and Q.relative_gap(tri_th, areas) >= Q.MIN_GAP, name
        hollow, back = Q.hollow_and_brought_back(g[f"{name}/x_1"], g[f"{name}/x_2"], len(pts), pairs, lengths, edge_th)
        hollow_cases += hollow > 0
        back_cases += back > 0
        if "_e0_" in name:                                     # half the shortest edge: every 1-simplex was brought back
            assert edge_th < lengths.min() and back == len(g[f"{name}/x_1"]) > 0, name
    assert hollow_cases >= 10 and back_cases >= 10, (hollow_cases, back_cases)
    ring = g["ring_13_chords_e5_t5/edges"]
    assert ring.shape == (2, 17) and len({(min(a, b), max(a, b)) for a, b in ring.T.tolist()}) == 17    # one direction each


@pytest.mark.parametrize("name", ["aspirin_21_k3", "nine_k3", "twelve_k2", "complete_6_k5"])
def test_infinite_thresholds_give_the_knn_clique_complex(pkg, name):
    from csmpn.data import complexes as cx
    g = np.load(os.path.join(Q.GOLD, "complexes_knn_ref.npz"))
    pts, k = g[f"{name}/points"], int(g[f"{name}/k"])
    for max_dim in (1, 2):
        a, b = cx.clique_complex(pts, cx.knn_edges(pts, k), max_dim=max_dim), cx.knn_clique_complex(pts, k, max_dim)
        for f in ("x_ind", "node_types", "edge_index", "edge_types"):
            assert torch.equal(getattr(a, f), getattr(b, f)), (f, max_dim)
    both = torch.cat([cx.knn_edges(pts, k), cx.knn_edges(pts, k)[[1, 0]], torch.tensor([[2, 2], [2, 2]])], dim=1)
    assert torch.equal(cx.clique_complex(pts, both, INF, INF).edge_index, cx.knn_clique_complex(pts, k).edge_index)


def _simplices(c):
    nt = c.node_types.numpy()
    return ({tuple(r[:2]) for r in c.x_ind.numpy()[nt == 1].tolist()}, {tuple(r[:3]) for r in c.x_ind.numpy()[nt == 2].tolist()})


def test_ties_on_the_lattice(pkg):
    """4 x 4 integer lattice, every sum exact. At (1, 1): the unit edge (0, 1) is in E_keep (s = 1 <= 1), (0, 2) of length 2 is
    not, yet the flat triple (0, 1, 2) of area 0 brings it back; the triangle (0, 1, 8) of area exactly 1 (g = 4 <= 4) is kept;
    (0, 2, 9) of area 2 is not. One ulp below both: (0, 1, 8) is dropped, and with edge_th alone one ulp below 1 and no
    triangle kept (tri_th = 0 keeps the flat ones - so G without them) no unit edge survives."""
    from csmpn.data import complexes as cx
    pts, edges = Q.lattice_case()
    e, t = _simplices(cx.clique_complex(pts, edges, 1.0, 1.0))
    assert (0, 1) in e and (0, 4) in e and (0, 1, 8) in t and (0, 1, 2) in t and (0, 2) in e and (0, 2, 9) not in t
    assert (0, 5, 6) in t and (0, 6) in e                                    # sqrt 5 comes back with its triangle
    below = float(np.nextafter(1.0, 0.0))
    e, t = _simplices(cx.clique_complex(pts, edges, below, below))
    assert (0, 1, 8) not in t and (0, 1, 5) in t and (0, 1) in e            # area 1 dropped; area 1/2 kept and brings (0, 1) back
    only = np.array([[0, 1, 0], [1, 5, 5]])                                  # one triangle of area 1/2: legs 1, 1, sqrt 2
    assert _simplices(cx.clique_complex(pts, only, 1.0, 0.25)) == ({(0, 1), (1, 5)}, set())
    assert _simplices(cx.clique_complex(pts, only, below, 0.25)) == (set(), set())
    assert _simplices(cx.clique_complex(pts, only, 0.0, 0.5)) == ({(0, 1), (0, 5), (1, 5)}, {(0, 1, 5)})
    assert _simplices(cx.clique_complex(pts, only, 0.0, float(np.nextafter(0.5, 0.0)))) == (set(), set())
    for bad in ((-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("nan"))):
        with pytest.raises(ValueError):
            cx.clique_complex(pts, only, *bad)
    with pytest.raises(ValueError):
        cx.clique_complex(pts, np.array([[0], [16]]))


def test_nan_vertex_is_dropped_by_a_finite_threshold_and_kept_by_infinity(pkg):
    from csmpn.data import complexes as cx
    pts = Q.make_points("nan", 5, 2, 8, 5)[8:].astype(np.float64)
    assert np.isnan(pts[2]).any()
    edges = cx.knn_edges(pts, 3)
    e, t = _simplices(cx.clique_complex(pts, edges, 1e6, 1e6))
    assert e and all(2 not in s for s in e | t)
    e_inf, t_inf = _simplices(cx.clique_complex(pts, edges, INF, INF))
    assert any(2 in s for s in e_inf) and e < e_inf and t <= t_inf
    assert _simplices(cx.clique_complex(pts, edges, INF, INF)) == _simplices(cx.knn_clique_complex(pts, 3))
    half = _simplices(cx.clique_complex(pts, edges, INF, 1e6))               # the NaN edges stay, their triangles go
    assert half[0] == e_inf and all(2 not in s for s in half[1])


CLOSED_FORM_CASES = [c for c in Q.CASES if c not in ("complete_2x64", "second_scan_pass_300x5")]    # (slow as Python loops)


@pytest.mark.parametrize("name", CLOSED_FORM_CASES)
def test_closed_forms_with_the_table_match_host_lift(pkg, name):
    """Every position the kernels compute from popcounts of the final masks and of T and from the scans
    (clique_lift_helpers.closed_form_structure, over the rule restated as scalar loops) is the position clique_complex +
    collate() + pad_batch() give."""
    pts, B, _, _, edge_th, tri_th, max_dim, cap, lists, want = Q.reference(name)
    got = Q.closed_form_structure(pts, B, lists, edge_th, tri_th, max_dim, cap)
    assert Q.differences(got, want) == []


def test_cases_reach_what_they_are_for(pkg):
    c = lambda name: Q.reference(name)[9]["counts"].tolist()
    assert c("triangle_kept_1x3") == [3, 3, 1, 30] and c("triangle_dropped_1x3") == [3, 3, 0, 18]
    n = c("complete_2x64")
    assert n[1] == 2 * 2016 and 0 < n[2] < 1000                              # every edge, few triangles: all else is hollow
    edges = Q.reference("complete_2x64")[9]["x_ind"][Q.reference("complete_2x64")[9]["node_types"] == 1]
    assert [0, 63] in edges[:, :2].tolist() and [62, 63] in edges[:, :2].tolist()
    n = c("edge_th_0_2x9")
    assert n[1] > 0 and n[2] > 0
    n = c("tri_th_0_2x8")
    assert n[1] > 0 and n[2] == 0
    _, B, glist, _, _, _, _, _, lists, want = Q.reference("empty_graph_3x6")
    assert lists[1].shape[1] == 0 and int(want["ptr"][2] - want["ptr"][1]) == 6 and int(want["ptr"][1]) > 6
    assert c("second_scan_pass_300x5")[0] == 1500
    _, _, dirty, _, _, _, _, _, lists, _ = Q.reference("dirty_list_2x7")
    assert (dirty == -1).all(0).sum() == 9 and (dirty[0] == dirty[1]).sum() >= 14 and dirty.shape[1] > 2 * sum(l.shape[1] for l in lists) // 2
    n1 = c("max_dim_1_4x7")
    assert len(n1) == 3 and n1[2] == 6 * n1[1]
    _, _, _, _, _, _, _, cap, _, want = Q.reference("exact_capacity_4x9")
    assert want["counts"].tolist() == list(cap.simplices) + [cap.edges]
    assert c("lattice_ties_1x16") != c("lattice_below_1x16")
    assert c("nan_vertex_2x8")[1] < c("nan_vertex_inf_2x8")[1]
    g = Q.fixture()
    want = Q.reference("aspirin_from_k3")[9]
    rows = want["x_ind"][: int(want["ptr"][1])]
    types = want["node_types"][: int(want["ptr"][1])]
    for d in (1, 2):
        assert np.array_equal(rows[types == d][:, :d + 1].numpy(), g[f"knn_21_k3_s0_e5_t5/x_{d}"])


def test_capacity(pkg):
    from csmpn.data import complexes as cx
    for name in ("edge_th_0_2x9", "max_dim_1_4x7", "empty_graph_3x6"):
        pts, B, _, _, edge_th, tri_th, max_dim, _, lists, want = Q.reference(name)
        c = want["counts"].tolist()
        n1, n2 = c[1], c[2] if max_dim == 2 else 0
        V = pts.shape[0] // B
        cap = cx.clique_capacity(B, V, n1, n2, max_dim=max_dim)
        assert cap.simplices == (B * V, n1 + 1) + ((n2,) if max_dim == 2 else ()) and cap.edges == cx.clique_adjacencies(n1, n2) == c[-1]
        cx.pad_batch(Q.host_lift(pts, B, lists, edge_th, tri_th, max_dim), cap)
        full = cx.clique_capacity(B, V, max_dim=max_dim)
        assert full.simplices[1] == B * math.comb(V, 2) + 1 and full.max_dim == max_dim
        assert full.edges == cx.clique_adjacencies(B * math.comb(V, 2), B * math.comb(V, 3) if max_dim == 2 else 0)
        cx.pad_batch(Q.host_lift(pts, B, lists, edge_th, tri_th, max_dim), full)
    assert cx.clique_capacity(2, 64).simplices == (128, 2 * 2016 + 1, 2 * 41664)
    for bad in (dict(max_dim=3), dict(verts_per_graph=2), dict(max_edges=-1), dict(max_triangles=-1), dict(n_graphs=0)):
        a = dict(n_graphs=4, verts_per_graph=6)
        a.update(bad)
        with pytest.raises(ValueError):
            cx.clique_capacity(**a)


def test_workspace_query(pkg):
    from csmpn_hip import native
    lib = native.lib()
    q = lib.csmpn_clique_lift_workspace_bytes
    sizes = [int(q(b, 13, 2)) for b in (1, 16, 300, 5000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert int(q(16, 64, 2)) > 0 and int(q(16, 2, 1)) > 0
    assert int(q(16, 65, 2)) == 0 and int(q(16, 13, 0)) == 0 and int(q(16, 13, 3)) == 0
    assert int(q(0, 13, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q(1 << 31, 13, 2)) == 0
    for B, V in ((16, 21), (3, 64), (300, 5)):                 # the table [V, V] and G's masks [V] of every graph on top of the kNN lift's
        assert int(q(B, V, 2)) >= int(lib.csmpn_knn_lift_workspace_bytes(B, V, 2)) + 8 * B * V * (V + 1)
    assert int(q(16, 16, 2)) >= int(lib.csmpn_hull_lift_workspace_bytes(16, 16, 2))


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call
DEFAULT = object()


def _call(lib, **over):
    """csmpn_clique_lift for 4 graphs of 6 vertices in R^3, a list of 9 entries, thresholds (1.5, 0.5), max_dim 2, with the
    named arguments replaced."""
    a = dict(points=FAKE, point_dim=3, n_graphs=4, verts=6, k=0, edge_list=FAKE, n_list=9, edge_th=1.5, tri_th=0.5, max_dim=2,
             cap=(24, 28, 13), cap_edges=384, x_ind=FAKE, x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE,
             x_ind_ptr=FAKE, edge_index=FAKE, edge_types=FAKE, counts=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_clique_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["k"], a["edge_list"], a["n_list"],
                                 a["edge_th"], a["tri_th"], a["max_dim"], None if cap is None else C.addressof(cap),
                                 a["cap_edges"], a["x_ind"], a["x_ind_cols"], a["node_types"], a["batch"], a["x_ind_batch"],
                                 a["ptr"], a["x_ind_ptr"], a["edge_index"], a["edge_types"], a["counts"], a["status"],
                                 a["workspace"], a["workspace_bytes"], None)


REJECTED = [
    ("list_and_k", dict(k=3), "invalid"),
    ("neither_list_nor_k", dict(edge_list=None), "invalid"),
    ("neither_list_nor_k_negative", dict(edge_list=None, k=-2), "invalid"),
    ("n_list_negative", dict(n_list=-1), "invalid"),
    ("n_list_past_int32", dict(n_list=1 << 31), "invalid"),
    ("edge_th_negative", dict(edge_th=-1.0), "invalid"),
    ("edge_th_nan", dict(edge_th=float("nan")), "invalid"),
    ("tri_th_negative", dict(tri_th=-0.5), "invalid"),
    ("tri_th_nan", dict(tri_th=float("nan")), "invalid"),
    ("tri_th_nan_with_k", dict(edge_list=None, k=3, tri_th=float("nan")), "invalid"),
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
    ("workspace_of_the_knn_lift", dict(workspace_bytes=DEFAULT), "invalid"),
    ("no_capacity", dict(cap=None), "invalid"),
] + [(f"null_{name}", {name: None}, "invalid") for name in
     ("points", "x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr", "edge_index")]


@pytest.mark.parametrize("name,over,code", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments(pkg, name, over, code):
    from csmpn_hip import native
    lib = native.lib()
    if over.get("workspace_bytes") is DEFAULT:                 # enough for csmpn_knn_lift, not for the table
        over = dict(over, workspace_bytes=int(lib.csmpn_knn_lift_workspace_bytes(4, 6, 2)))
    want = {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[code]
    assert _call(lib, **over) == want
    assert lib.csmpn_last_error()                       # a message says why


def test_source_and_thresholds_are_checked_where_dis_and_k_are(pkg):
    """A bad source or threshold together with an unsupported shape reports the shape; together with a later finding (x_ind
    too narrow) it is reported itself; infinite thresholds and k <= 0 beside a list pass these checks (the next finding - the
    narrow x_ind - is reported)."""
    from csmpn_hip import native
    lib = native.lib()
    for bad in (dict(k=3), dict(edge_list=None), dict(edge_th=-1.0), dict(tri_th=float("nan")), dict(n_list=-1)):
        assert _call(lib, max_dim=3, cap=(24, 28, 13, 1), x_ind_cols=4, **bad) == native.ERR_UNSUPPORTED
        assert _call(lib, verts=65, cap=(260, 28, 13), **bad) == native.ERR_UNSUPPORTED
        assert _call(lib, point_dim=0, **bad) == native.ERR_INVALID and b"point_dim" in lib.csmpn_last_error()
    for bad, word in ((dict(k=3), b"exactly one"), (dict(edge_list=None), b"exactly one"), (dict(edge_th=-1.0), b"edge_th"),
                      (dict(tri_th=float("nan")), b"tri_th"), (dict(n_list=-1), b"n_list")):
        assert _call(lib, x_ind_cols=2, **bad) == native.ERR_INVALID and word in lib.csmpn_last_error()
    for fine in (dict(edge_th=INF, tri_th=INF), dict(edge_th=0.0, tri_th=0.0), dict(k=-5), dict(edge_list=None, k=2), dict(n_list=0)):
        assert _call(lib, x_ind_cols=2, **fine) == native.ERR_INVALID and b"x_ind has 2 columns" in lib.csmpn_last_error()


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clique_lift(torch.zeros(24, 3), 4, i64(2, 5), 2, (24, 28, 13), 384, i64(65, 3), i64(65), i64(65), i64(65), i64(5), i64(5),
                        i64(2, 384), None, None, None, torch.zeros(4096, dtype=torch.uint8), edge_th=1.0)
    from csmpn.data import complexes as cx
    with pytest.raises(ValueError, match="exactly one"):
        cx.clique_batch_device(torch.zeros(24, 3), 4, cx.BatchCapacity((24, 28, 13), 384))
    with pytest.raises(ValueError, match="exactly one"):
        cx.clique_batch_device(torch.zeros(24, 3), 4, cx.BatchCapacity((24, 28, 13), 384), edges=i64(2, 5), knn=3)
    with pytest.raises(ValueError, match="edge_th"):
        cx.clique_batch_device(torch.zeros(24, 3), 4, cx.BatchCapacity((24, 28, 13), 384), knn=3, edge_th=-1.0)


def test_exclusion_rules(pkg):
    """relift_, load_points and step refuse two sources, none, and a threshold beside dis or hull before they touch the device;
    one source with thresholds is accepted and the missing plan is the next finding. (The step object is made without its
    constructor: capturing needs a GPU, the argument rule does not.)"""
    from csmpn.data import complexes as cx
    from csmpn_hip.graphed import GraphedTrainStep
    pts32 = Q.make_points("normal", 0, 2, 5, 3)
    b = Q.host_lift(pts32, 2, Q.local_lists(Q.knn_list(pts32, 2, 2), 2, 5), INF, INF, 2)
    pts, edges = torch.zeros(10, 3), torch.zeros(2, 4, dtype=torch.int64)
    for both in (dict(dis=1.0, edges=edges), dict(knn=3, edges=edges), dict(hull=True, edges=edges), dict(dis=1.0, knn=3), dict()):
        with pytest.raises(ValueError, match="exactly one"):
            b.relift_(pts, **both)
    for bad in (dict(dis=1.0, edge_th=1.0), dict(hull=True, tri_th=1.0), dict(dis=1.0, edge_th=INF)):
        with pytest.raises(ValueError, match="edge_th / tri_th"):
            b.relift_(pts, **bad)
    for fine in (dict(edges=edges), dict(edges=edges, edge_th=1.0, tri_th=0.5), dict(knn=3, edge_th=1.0), dict(knn=3, tri_th=0.5), dict(knn=3)):
        with pytest.raises(RuntimeError, match="plan"):
            b.relift_(pts, **fine)
    for bad in (dict(rips_dis=1.0, edges=True), dict(knn=3, edges=True), dict(hull=True, edges=64), dict(rips_dis=1.0, knn=3)):
        with pytest.raises(ValueError, match="exclude"):
            GraphedTrainStep(None, None, None, [], **bad)
    for bad in (dict(rips_dis=1.0, edge_th=1.0), dict(hull=True, tri_th=1.0)):
        with pytest.raises(ValueError, match="edge_th / tri_th"):
            GraphedTrainStep(None, None, None, [], **bad)
    for defaults in (dict(), dict(rips_dis=1.6), dict(knn=3), dict(edges=True)):
        gs = object.__new__(GraphedTrainStep)
        gs.capacity, gs.rips_dis, gs.knn = cx.BatchCapacity((10, 5, 2), 40), None, None
        gs.__dict__.update(defaults)
        for both in (dict(dis=1.0, edges=edges), dict(knn=3, edges=edges), dict(hull=True, edges=edges)):
            with pytest.raises(ValueError, match="exclude"):
                gs.load_points(pts, **both)
            with pytest.raises(ValueError, match="exclude"):
                gs.step(points=pts, **both)
    gs = object.__new__(GraphedTrainStep)
    gs.capacity, gs.rips_dis, gs.knn = cx.BatchCapacity((10, 5, 2), 40), None, None
    with pytest.raises(ValueError, match="pass dis"):
        gs.load_points(pts)
    gs.edges = True
    with pytest.raises(ValueError, match="pass edges"):
        gs.step(points=pts)
    gs.edges, gs.batch = False, b
    with pytest.raises(ValueError, match="edge_th / tri_th"):
        gs.step(points=pts, dis=1.0, edge_th=2.0)


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on, on a case with hollow triples and brought-back edges."""
    _, B, _, _, _, _, _, cap, _, want = Q.reference("edge_th_0_2x9")
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert Q.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert Q.differences(swapped, want) == ["edge_index"]
    wrong_ptr = clone()
    wrong_ptr["ptr"][1] += 1
    assert Q.differences(wrong_ptr, want) == ["ptr"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert Q.differences(filler, want) == ["node_types"]
    triangle = clone()                                     # one triangle more: a hollow triple filled in
    row = int((want["node_types"] == 2).nonzero()[0])
    triangle["x_ind"][row, 2] += 1
    assert Q.differences(triangle, want) == ["x_ind"]
    count = clone()
    count["counts"][2] += 1
    assert Q.differences(count, want) == ["counts"]
    narrower = clone()
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert Q.differences(narrower, want) == ["batch"]
    bufs = Q.buffers(cap, B, torch.device("cpu"))
    assert Q.guards_intact(bufs) is None
    bufs["edge_types"][1][0] = 0
    assert Q.guards_intact(bufs) == "edge_types"
