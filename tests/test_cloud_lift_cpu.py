"""The Rips lift of point clouds on the device (csmpn_cloud_lift), the parts that need no GPU: the fast restatement of the host
lift against lift() itself, rips_complex(vertex_block=False) against clique_complex, cloud_capacity, the workspace query, every
rejected argument combination with its code, message and place among the shared checks (the arguments are checked before the
first HIP call), the relift_ exclusions of a cloud batch, the kernels' closed forms restated word by word on the host against
the host lift, and a mutation guard for the comparison the GPU tests use."""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import cloud_lift_helpers as CL

HOST_CASES = [n for n, c in CL.CASES.items() if c["host"]]


def test_case_table_is_conditioned(pkg):
    """Every case keeps the margin or is exact (points_of asserts it); the placed and dense cases hold what they are for."""
    for name in CL.CASES:
        if name != "grid_4096":                            # the GPU test of the large case checks it
            CL.points_of(name)
    x = CL.reference("placed_200", False)[4]
    rows = {tuple(r) for r in x["x_ind"][: int(x["ptr"][-1])].tolist()}
    for simplex in ((63, 64, 0), (64, 65, 0), (127, 128, 0), (0, 199, 0), (5, 70, 140), (62, 63, 64), (66, 195, 0), (10, 66, 195),
                    (66, 130, 195), (66, 195, 197)):
        assert simplex in rows, simplex
    assert (63, 65, 0) not in rows and not any(100 in r[:2] and r[1] for r in rows)      # vertex 100 is isolated
    assert CL.reference("clique66_in_130", False)[4]["counts"].tolist()[1:3] == [66 * 65 // 2, 45760]
    assert CL.reference("complete_65_dim1", True)[4]["counts"].tolist()[1] == 65 * 64 // 2
    edges = CL.reference("sparse_65", False)[4]["x_ind"]
    assert int((edges[:, 1] == 64).sum()) > 0               # the vertex alone in word 1 has a neighbour
    assert len(CL.reference("lattice_tie_72", False)[4]["x_ind"]) > len(CL.reference("lattice_ulp_below_72", False)[4]["x_ind"])
    assert CL.reference("dis0_coincident_70", False)[4]["counts"].tolist()[1:3] == [7, 4]    # a 4-clique and a pair


@pytest.mark.parametrize("vertex_block", [False, True], ids=["no_block", "block"])
@pytest.mark.parametrize("name", HOST_CASES)
def test_fast_restatement_matches_host_lift(pkg, name, vertex_block):
    pts, dis, max_dim, cap, want = CL.reference(name, vertex_block)
    assert CL.differences(want, CL.host_structure(name, vertex_block, cap)) == []


def test_fast_restatement_is_fast(pkg):
    c = CL.CASES["clique66_in_130"]
    pts = CL.points_of("clique66_in_130")
    t0 = time.perf_counter()
    CL.fast_structure(pts, c["B"], c["dis"], c["max_dim"], True)
    assert time.perf_counter() - t0 < 2.0


@pytest.mark.parametrize("name", list(CL.SMALL))
def test_rips_without_vertex_block_is_the_clique_complex(pkg, name):
    """rips_complex(vertex_block=False) is the thresholded clique lift with edge_th = dis. clique_complex takes its triples
    from the pairs of the GRAPH, not from the pairs that edge_th keeps, and a kept triple brings its pairs back: over the
    complete graph with tri_th = +infinity it keeps all C(V, 3) triples and every pair (on tiny_12, graph 0: 220 triangles and
    66 edges where the Rips complex has 17 and 23), so that form is no identity. The two forms that are one: the complete
    graph's list with tri_th = 0, which keeps no triple of points in general position, at max_dim = 1; and the list of the
    close pairs - the complete list with the pairs beyond dis struck out - at max_dim = 2."""
    from csmpn.data import complexes as cx
    c = CL.CASES[name]
    p = CL.points_of(name).astype(np.float64).reshape(c["B"], c["V"], c["n"])
    complete = torch.tensor(list(itertools.combinations(range(c["V"]), 2)), dtype=torch.int64).t().contiguous()
    same = lambda x, y: all(torch.equal(getattr(x, k), getattr(y, k)) for k in ("x_ind", "node_types", "edge_index", "edge_types"))
    for g in range(c["B"]):
        a = cx.rips_complex(p[g], c["dis"], c["max_dim"], vertex_block=False)
        assert same(cx.rips_complex(p[g], c["dis"], 1, vertex_block=False), cx.clique_complex(p[g], complete, edge_th=c["dis"], tri_th=0.0, max_dim=1)), g
        close = complete[:, torch.from_numpy(np.linalg.norm(p[g][complete[0]] - p[g][complete[1]], axis=-1) <= c["dis"])]
        assert same(a, cx.clique_complex(p[g], close, edge_th=c["dis"], max_dim=c["max_dim"])), g
        assert not same(a, cx.clique_complex(p[g], complete, edge_th=c["dis"], max_dim=c["max_dim"]))
        assert int(a.node_types.eq(1).sum()) > 0 and int(a.node_types.eq(2).sum()) > 0
        d = cx.rips_complex(p[g], c["dis"], c["max_dim"])            # the default keeps the block
        assert int(d.edge_index.shape[1]) == int(a.edge_index.shape[1]) + c["V"] * (c["V"] - 1) - int(a.node_types.eq(1).sum())


def test_cloud_capacity_counts_adjacencies(pkg):
    from csmpn.data import complexes as cx
    for name in HOST_CASES:
        c = CL.CASES[name]
        for vb in (False, True):
            raw = cx.collate(CL.host_complexes(name, vb))
            n = torch.bincount(raw.node_types, minlength=3).tolist()
            cap = cx.cloud_capacity(c["B"], c["V"], n[1], n[2], c["max_dim"], vertex_block=vb)
            assert cap.edges == int(raw.edge_index.shape[1]), (name, vb)
            assert cap.simplices == (c["B"] * c["V"], n[1] + 1) + ((n[2],) if c["max_dim"] == 2 else ())
            assert cap.simplices == cx.rips_capacity(c["B"], c["V"], n[1], n[2], c["max_dim"]).simplices
            cx.pad_batch(raw, cap)
        if name == "b3_65":
            break                                                     # lift() of the rest is checked above
    assert cx.cloud_capacity(1, 4096, 10, 2).edges == cx.clique_adjacencies(10, 2)
    assert cx.cloud_capacity(2, 100, 10, 2, vertex_block=True).edges == cx.rips_adjacencies(2, 100, 10, 2)
    with pytest.raises(ValueError):
        cx.cloud_capacity(4, 6, 10, 2, max_dim=3)


def test_workspace_query(pkg):
    from csmpn_hip import native
    q = native.lib().csmpn_cloud_lift_workspace_bytes
    assert int(q(1, 4097, 2)) == 0 and int(q(16, 100, 0)) == 0 and int(q(16, 100, 3)) == 0
    assert int(q(0, 100, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q((1 << 31) // 100 + 1, 100, 2)) == 0
    for V in (64, 65, 4096):
        sizes = [int(q(b, V, 2)) for b in (1, 3, 16, 300)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0], V
    assert int(q(1, 2, 1)) > 0
    # masks V^2 / 8 and ranks V^2 / 16 bytes per graph, 16 V of per-vertex counts
    assert int(q(1, 4096, 2)) >= 4096 * 4096 // 8 + 4096 * 4096 // 16 + 16 * 4096
    assert int(q(1, 4096, 2)) <= 4096 * 4096 // 8 + 4096 * 4096 // 16 + 16 * 4096 + 4096


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call


def _call(lib, **over):
    """csmpn_cloud_lift for 2 graphs of 100 vertices in R^3, max_dim 2, with the named arguments replaced."""
    a = dict(points=FAKE, point_dim=3, n_graphs=2, verts=100, dis=1.0, vertex_block=0, max_dim=2, cap=(200, 28, 13), cap_edges=384,
             x_ind=FAKE, x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE, x_ind_ptr=FAKE, edge_index=FAKE,
             edge_types=FAKE, counts=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 24)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_cloud_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["dis"], a["vertex_block"], a["max_dim"],
                                None if cap is None else C.addressof(cap), a["cap_edges"], a["x_ind"], a["x_ind_cols"],
                                a["node_types"], a["batch"], a["x_ind_batch"], a["ptr"], a["x_ind_ptr"], a["edge_index"],
                                a["edge_types"], a["counts"], a["status"], a["workspace"], a["workspace_bytes"], None)


# name, replaced arguments, code, a piece of the message; in the order of the checks
REJECTED = [
    ("max_dim_negative", dict(max_dim=-1), "invalid", "max_dim -1 is negative"),
    ("max_dim_0", dict(max_dim=0, cap=(200,), x_ind_cols=1), "unsupported", "max_dim 0"),
    ("max_dim_3", dict(max_dim=3, cap=(200, 28, 13, 1), x_ind_cols=4), "unsupported", "max_dim 3"),
    ("4097_vertices", dict(verts=4097, n_graphs=1, cap=(4097, 28, 13)), "unsupported", "kCloudMaxVerts = 4096"),
    ("too_few_vertices", dict(verts=2, cap=(4, 28, 13)), "invalid", "2 vertices per graph"),
    ("too_few_vertices_max_dim_1", dict(verts=1, max_dim=1, cap=(2, 28)), "invalid", "1 vertices per graph"),
    ("no_graph", dict(n_graphs=0), "invalid", "bad sizes"),
    ("negative_graphs", dict(n_graphs=-3), "invalid", "bad sizes"),
    ("vertices_past_int32", dict(n_graphs=(1 << 31) // 100 + 1), "invalid", "bad sizes"),
    ("point_dim_0", dict(point_dim=0), "invalid", "point_dim 0"),
    ("negative_dis", dict(dis=-1.0), "invalid", "dis -1"),
    ("nan_dis", dict(dis=float("nan")), "invalid", "not a number"),
    ("vertex_block_2", dict(vertex_block=2), "invalid", "vertex_block 2"),
    ("vertex_block_negative", dict(vertex_block=-1), "invalid", "vertex_block -1"),
    ("x_ind_too_narrow", dict(x_ind_cols=2), "invalid", "x_ind has 2 columns"),
    ("no_capacity", dict(cap=None), "invalid", "null pointer"),
    ("vertex_capacity_differs", dict(cap=(201, 28, 13)), "invalid", "vertex rows are never padded"),
    ("negative_row_capacity", dict(cap=(200, -1, 13)), "invalid", "capacity -1 of dimension 1"),
    ("rows_past_int32", dict(cap=(200, (1 << 31) - 210, 13)), "invalid", "bad capacity"),
    ("negative_edge_capacity", dict(cap_edges=-1), "invalid", "bad capacity"),
    ("edges_past_int32", dict(cap_edges=1 << 31), "invalid", "bad capacity"),
    ("no_workspace", dict(workspace=None), "invalid", "workspace too small"),
    ("workspace_too_small", dict(workspace_bytes=64), "invalid", "workspace too small"),
] + [(f"null_{name}", {name: None}, "invalid", "null pointer") for name in
     ("points", "x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr", "edge_index")]


@pytest.mark.parametrize("name,over,code,message", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_arguments(pkg, name, over, code, message):
    from csmpn_hip import native
    lib = native.lib()
    want = {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[code]
    assert _call(lib, **over) == want
    assert message in lib.csmpn_last_error().decode()


def test_rejections_come_in_the_order_of_the_shared_checks(pkg):
    """Two faults in one call: the one that check_lift_args reaches first is reported - max_dim, the vertex limit, the sizes,
    point_dim, dis, vertex_block, the x_ind columns, the pointers, the capacity, the workspace."""
    from csmpn_hip import native
    lib = native.lib()
    order = [("max_dim_3", "4097_vertices"), ("4097_vertices", "no_graph"), ("no_graph", "point_dim_0"), ("point_dim_0", "negative_dis"),
             ("negative_dis", "vertex_block_2"), ("vertex_block_2", "x_ind_too_narrow"), ("x_ind_too_narrow", "null_points"),
             ("null_points", "negative_edge_capacity"), ("negative_edge_capacity", "workspace_too_small")]
    table = {r[0]: r for r in REJECTED}
    for first, second in order:
        over = dict(table[second][1])
        over.update(table[first][1])
        if first == "max_dim_3":
            over["cap"] = (4097, 28, 13, 1)
        assert _call(lib, **over) == {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[table[first][2]], (first, second)
        assert table[first][3] in lib.csmpn_last_error().decode(), (first, second)
    # V <= 64 is served as well: the same call with 64 vertices passes every check up to the workspace
    assert _call(lib, verts=64, cap=(128, 28, 13), workspace_bytes=64) == native.ERR_INVALID
    assert "workspace too small" in lib.csmpn_last_error().decode()


def test_the_four_small_lifts_still_refuse_65_vertices(pkg):
    from csmpn_hip import native
    lib = native.lib()
    for q in (lib.csmpn_rips_lift_workspace_bytes, lib.csmpn_knn_lift_workspace_bytes, lib.csmpn_hull_lift_workspace_bytes,
              lib.csmpn_clique_lift_workspace_bytes):
        assert int(q(16, 65, 2)) == 0


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cloud_lift(torch.zeros(200, 3), 2, 1.0, 2, (200, 28, 13), 384, i64(241, 3), i64(241), i64(241), i64(241), i64(3), i64(3),
                       i64(2, 384), None, None, None, torch.zeros(4096, dtype=torch.uint8))


def test_relift_exclusions_of_a_cloud_batch(pkg):
    """On a batch whose plan says `cloud`, everything but dis=... alone is a ValueError that names the 64-vertex limit - before
    anything needs a device; a plain batch gets the errors it always got."""
    from csmpn.data import complexes as cx
    raw = cx.collate(CL.host_complexes("tiny_12", False))
    raw.plan(2)
    pts = torch.from_numpy(CL.points_of("tiny_12"))
    with pytest.raises(RuntimeError, match="plan\\(\\) and csr\\(\\)"):       # not a cloud batch: as before
        raw.relift_(pts, knn=3)
    raw._plan["cloud"] = {"vertex_block": False}
    for kw in (dict(knn=3), dict(hull=True), dict(edges=torch.zeros(2, 1, dtype=torch.int64)), dict(knn=3, edge_th=1.0),
               dict(dis=1.0, edge_th=1.0), dict(dis=1.0, tri_th=1.0)):
        with pytest.raises(ValueError, match="64 vertices"):
            raw.relift_(pts, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        raw.relift_(pts, dis=1.0, knn=3)
    with pytest.raises(RuntimeError, match="plan\\(\\) and csr\\(\\)"):       # dis alone passes the exclusions
        raw.relift_(pts, dis=1.0)


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on."""
    _, _, _, cap, want = CL.reference("sparse_129", False)
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert CL.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert CL.differences(swapped, want) == ["edge_index"]
    wrong = clone()                                        # one vertex of one edge in another word
    row = int(want["node_types"].eq(1).nonzero()[0])
    wrong["x_ind"][row, 1] += 64
    assert CL.differences(wrong, want) == ["x_ind"]
    count = clone()
    count["counts"][2] += 1
    assert CL.differences(count, want) == ["counts"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert CL.differences(filler, want) == ["node_types"]
    narrower = clone()                                     # ... and shapes and dtypes count
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert CL.differences(narrower, want) == ["batch"]


CLOSED_FORM_CASES = ["sparse_65", "sparse_129", "b3_65", "placed_200", "lattice_tie_72", "nan_vertex_70", "max_dim_1_100", "exact_capacity_66"]


@pytest.mark.parametrize("vertex_block", [False, True], ids=["no_block", "block"])
@pytest.mark.parametrize("name", CLOSED_FORM_CASES)
def test_closed_forms_match_host_lift(pkg, name, vertex_block):
    """Every position the kernels compute from mask words, ranks and scans (restated word by word in
    cloud_lift_helpers.closed_form_structure, each position written exactly once) is the position the host lift gives."""
    pts, dis, max_dim, cap, want = CL.reference(name, vertex_block)
    got = CL.closed_form_structure(pts, CL.CASES[name]["B"], dis, max_dim, vertex_block, cap)
    assert CL.differences(got, want) == []
