"""The kNN clique lift of point clouds on the device (csmpn_cloud_knn_lift), the parts that need no GPU: the fast restatement of
the host lift against knn_clique_complex + collate + pad_batch, the case table's conditioning, the exports and the header, the
workspace query, every rejected argument combination with its code, message and place among the shared checks (the arguments
are checked before the first HIP call), knn_capacity above 64 vertices, the relift_ and GraphedTrainStep exclusions in both
directions, the selection restated as threshold + tie prefix and the symmetrisation, word by word, against the rank rule, and a
mutation guard for the comparison the GPU tests use."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import cloud_knn_lift_helpers as CK
import knn_lift_helpers as KH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [n for n, c in CK.CASES.items() if c["host"]]


def test_case_table_is_conditioned(pkg):
    """Every case that is no deliberate tie keeps the margin (recomputed here, not read from a cache); the placed cases hold
    what they are for."""
    for name, c in CK.CASES.items():
        if name == "grid_4096_k8":
            continue                                        # a tie case; its GPU test checks what it holds
        pts = CK.points_of(name)
        assert pts.dtype == np.float32 and pts.shape == (c["B"] * c["V"], c["n"])
        if c.get("tie"):
            continue
        p = pts.astype(np.float64).reshape(c["B"], c["V"], c["n"])
        for g in range(c["B"]):
            if c["k"] < c["V"] - 1:
                so = np.sort(np.where(np.eye(c["V"], dtype=bool), np.inf, CK.pair_sums(p[g])), axis=1)
                assert np.all(so[:, c["k"]] - so[:, c["k"] - 1] >= CK.MARGIN * so[:, c["k"]]), (name, g)
    named = CK.directed_neighbours(CK.points_of("boundary_130_k1").astype(np.float64), 1)
    assert named[64, 63] and not named[63, 64] and named[63, 10] and named[10, 63]       # one direction, across words 0 | 1
    assert named[127, 128] and not named[128, 127] and named[128, 20] and named[20, 128]  # the other direction, across 1 | 2
    rows = {tuple(r) for r in CK.reference("boundary_130_k1")[4]["x_ind"].tolist()}
    assert (63, 64, 0) in rows and (127, 128, 0) in rows and (10, 63, 0) in rows and (10, 63, 64) not in rows
    c = CK.CASES["outliers_3x70_k3"]
    p = CK.points_of("outliers_3x70_k3").astype(np.float64).reshape(3, 70, 3)
    for g in range(3):
        named = CK.directed_neighbours(p[g], 3)
        assert not named[:, 0].any() and not named[:, 69].any() and named[0].sum() == 3 and named[69].sum() == 3
    assert CK.reference("clique_66_k65")[4]["counts"].tolist()[1:3] == [66 * 65 // 2, 45760]
    assert CK.differences(CK.reference("clique_66_k100")[4], CK.reference("clique_66_k65")[4]) == []
    named = CK.directed_neighbours(CK.points_of("one_point_65_k3").astype(np.float64), 3)
    assert named[0].nonzero()[0].tolist() == [1, 2, 3] and named[2].nonzero()[0].tolist() == [0, 1, 3] and named[64].nonzero()[0].tolist() == [0, 1, 2]
    p = CK.points_of("nan_vertex_2x70_k3").astype(np.float64).reshape(2, 70, 3)
    named = CK.directed_neighbours(p[0], 3)
    assert named[65].nonzero()[0].tolist() == [0, 1, 2] and not named[:, 65].any()         # a NaN vertex: every sum +infinity
    lattice = CK.pair_sums(CK.points_of("lattice_72_k3").astype(np.float64))
    assert sum(len(np.unique(np.sort(row)[1:5])) < 4 for row in lattice) == 72              # equal sums among every vertex's four nearest


@pytest.mark.parametrize("name", HOST_CASES)
def test_fast_restatement_matches_host_lift(pkg, name):
    pts, k, max_dim, cap, want = CK.reference(name)
    assert CK.differences(want, CK.host_structure(name, cap)) == []
    assert int(want["counts"][1]) > 0 and (max_dim == 1 or k == 1 or int(want["counts"][2]) > 0)     # k = 1: a forest and 2-cycles


def test_host_cases_span_the_sizes_and_k(pkg):
    sizes = {(CK.CASES[n]["V"], CK.CASES[n]["k"]) for n in HOST_CASES}
    assert {v for v, _ in sizes} >= {12, 33, 64, 65, 66, 70, 72, 100, 129}
    assert {k for _, k in sizes} >= {1, 3, 8} and (12, 11) in sizes and (33, 32) in sizes


def test_exports_and_header(pkg):
    from csmpn_hip import native
    lib = native.lib()
    for name in ("csmpn_cloud_knn_lift_workspace_bytes", "csmpn_cloud_knn_lift"):
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.csmpn_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "csmpn_hip.h")).read()
    assert re.search(r"size_t csmpn_cloud_knn_lift_workspace_bytes\(int64_t n_graphs, int32_t verts_per_graph, int32_t max_dim\);", header)
    decl = re.search(r"int csmpn_cloud_knn_lift\(([^;]*)\);", header).group(1)
    knn = re.search(r"int csmpn_knn_lift\(([^;]*)\);", header).group(1)
    assert re.sub(r"\s+", " ", decl) == re.sub(r"\s+", " ", knn)       # the argument list of csmpn_knn_lift


def test_workspace_query(pkg):
    """That of csmpn_cloud_lift plus 8 B V W bytes for the directed masks, rounded up to 256; 0 for sizes the entry rejects."""
    from csmpn_hip import native
    q, cloud = native.lib().csmpn_cloud_knn_lift_workspace_bytes, native.lib().csmpn_cloud_lift_workspace_bytes
    assert int(q(1, 4097, 2)) == 0 and int(q(16, 100, 0)) == 0 and int(q(16, 100, 3)) == 0
    assert int(q(0, 100, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q((1 << 31) // 100 + 1, 100, 2)) == 0
    for B, V, max_dim in ((1, 2, 1), (1, 3, 2), (1, 64, 2), (1, 65, 2), (3, 65, 2), (300, 65, 2), (2, 96, 1), (1, 200, 2), (1, 4096, 2)):
        extra = 8 * B * V * ((V + 63) // 64)
        assert int(cloud(B, V, max_dim)) > 0
        assert int(q(B, V, max_dim)) == int(cloud(B, V, max_dim)) + (extra + 255) // 256 * 256, (B, V, max_dim)


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call


def _call(lib, **over):
    """csmpn_cloud_knn_lift for 2 graphs of 100 vertices in R^3, k = 3, max_dim 2, with the named arguments replaced."""
    a = dict(points=FAKE, point_dim=3, n_graphs=2, verts=100, k=3, max_dim=2, cap=(200, 28, 13), cap_edges=384,
             x_ind=FAKE, x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE, x_ind_ptr=FAKE, edge_index=FAKE,
             edge_types=FAKE, counts=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 24)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_cloud_knn_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["k"], a["max_dim"],
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
    ("k_0", dict(k=0), "invalid", "k = 0 (at least 1)"),
    ("k_negative", dict(k=-2), "invalid", "k = -2 (at least 1)"),
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
    point_dim, k (where csmpn_knn_lift checks it: behind point_dim, in front of the x_ind columns), the pointers, the
    capacity, the workspace."""
    from csmpn_hip import native
    lib = native.lib()
    order = [("max_dim_3", "4097_vertices"), ("4097_vertices", "no_graph"), ("no_graph", "point_dim_0"), ("point_dim_0", "k_0"),
             ("k_0", "x_ind_too_narrow"), ("x_ind_too_narrow", "null_points"), ("null_points", "negative_edge_capacity"),
             ("negative_edge_capacity", "workspace_too_small")]
    table = {r[0]: r for r in REJECTED}
    for first, second in order:
        over = dict(table[second][1])
        over.update(table[first][1])
        if first == "max_dim_3":
            over["cap"] = (4097, 28, 13, 1)
        assert _call(lib, **over) == {"invalid": native.ERR_INVALID, "unsupported": native.ERR_UNSUPPORTED}[table[first][2]], (first, second)
        assert table[first][3] in lib.csmpn_last_error().decode(), (first, second)
    # V <= 64 is served as well, and a k far above V is no fault: both calls pass every check up to the workspace
    for over in (dict(verts=64, cap=(128, 28, 13)), dict(k=1 << 30)):
        assert _call(lib, workspace_bytes=64, **over) == native.ERR_INVALID
        assert "workspace too small" in lib.csmpn_last_error().decode()
    # the workspace of csmpn_cloud_lift is too small for this entry: the directed masks are missing
    short = int(lib.csmpn_cloud_lift_workspace_bytes(2, 100, 2))
    assert _call(lib, workspace_bytes=short) == native.ERR_INVALID and "workspace too small" in lib.csmpn_last_error().decode()


def test_the_small_knn_lift_still_refuses_65_vertices(pkg):
    from csmpn_hip import native
    assert int(native.lib().csmpn_knn_lift_workspace_bytes(16, 65, 2)) == 0


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="cloud_knn_lift needs device tensors \\(no CPU fallback\\)"):
        ops.cloud_knn_lift(torch.zeros(200, 3), 2, 3, 2, (200, 28, 13), 384, i64(241, 3), i64(241), i64(241), i64(241), i64(3), i64(3),
                           i64(2, 384), None, None, None, torch.zeros(4096, dtype=torch.uint8))
    from csmpn.data import complexes as cx
    with pytest.raises(RuntimeError, match="knn_cloud_batch_device needs device points"):
        cx.knn_cloud_batch_device(torch.zeros(200, 3), 2, 3, cx.knn_capacity(2, 100, 3, 50))


def test_knn_capacity_above_64_vertices(pkg):
    """knn_capacity's formula holds for any V: its default edge bound admits every case, and the capacity of a case's own
    counts is the shape of its collated batch."""
    from csmpn.data import complexes as cx
    for name in ("v129_k8", "v200_k3", "v1000_k8", "b3_65_k3", "clique_66_k65", "clique_66_k100", "boundary_130_k1", "max_dim_1_2x100_k3"):
        c = CK.CASES[name]
        counts = CK.fast_structure(CK.points_of(name), c["B"], c["k"], c["max_dim"])["counts"].tolist()
        n1, n2, E = counts[1], counts[2] if c["max_dim"] == 2 else 0, counts[-1]
        bound = cx.knn_capacity(c["B"], c["V"], c["k"], n2, max_dim=c["max_dim"])
        assert bound.simplices[0] == c["B"] * c["V"] and bound.simplices[1] - 1 == c["B"] * min(c["k"] * c["V"], c["V"] * (c["V"] - 1) // 2)
        assert n1 <= bound.simplices[1] - 1, name
        own = cx.knn_capacity(c["B"], c["V"], c["k"], n2, max_edges=n1, max_dim=c["max_dim"])
        assert own.edges == E == cx.clique_adjacencies(n1, n2) and own.simplices[1] == n1 + 1, name
        CK.fast_structure(CK.points_of(name), c["B"], c["k"], c["max_dim"], own)       # fits: no ValueError
    assert cx.knn_capacity(1, 4096, 8, 10).simplices == (4096, 8 * 4096 + 1, 10)


def _host_batch(name):
    from csmpn.data import complexes as cx
    raw = cx.collate(CK.host_complexes(name))
    raw.plan(2)
    return raw, torch.from_numpy(CK.points_of(name))


def test_relift_exclusions_in_both_directions(pkg):
    """On a batch whose plan says `cloud_knn`, everything but knn=... alone is a ValueError that names the batch - before
    anything needs a device; a batch of cloud_batch_device keeps refusing knn with the message it always had; a plain batch
    gets the errors it always got."""
    raw, pts = _host_batch("tiny_12_k3")
    with pytest.raises(RuntimeError, match="plan\\(\\) and csr\\(\\)"):       # a plain batch: as before
        raw.relift_(pts, knn=3)
    raw._plan["cloud_knn"] = {"k": 3}
    for kw in (dict(dis=1.0), dict(hull=True), dict(edges=torch.zeros(2, 1, dtype=torch.int64)), dict(knn=3, edge_th=1.0),
               dict(knn=3, tri_th=1.0), dict(dis=1.0, edge_th=1.0)):
        with pytest.raises(ValueError, match="kNN cloud batch \\(knn_cloud_batch_device\\)"):
            raw.relift_(pts, **kw)
    with pytest.raises(ValueError, match="exactly one"):
        raw.relift_(pts, dis=1.0, knn=3)
    with pytest.raises(RuntimeError, match="plan\\(\\) and csr\\(\\)"):       # knn alone passes the exclusions
        raw.relift_(pts, knn=3)
    del raw._plan["cloud_knn"]
    raw._plan["cloud"] = {"vertex_block": False}
    for kw in (dict(knn=3), dict(knn=3, edge_th=1.0)):
        with pytest.raises(ValueError, match="cloud_batch_device.*64 vertices"):
            raw.relift_(pts, **kw)
    with pytest.raises(RuntimeError, match="plan\\(\\) and csr\\(\\)"):
        raw.relift_(pts, dis=1.0)


def test_graphed_step_takes_a_knn_cloud_batch_as_it_is(pkg):
    """GraphedTrainStep pads and moves every batch but a cloud batch, which must have been built at the step's capacity; a
    kNN cloud batch is one."""
    from csmpn.data import complexes as cx
    from csmpn_hip.graphed import GraphedTrainStep
    raw, _ = _host_batch("tiny_12_k3")
    wrong = cx.BatchCapacity((24, int(raw.node_types.eq(1).sum()) + 5, int(raw.node_types.eq(2).sum()) + 5), int(raw.edge_index.shape[1]) + 9)
    for key, value in (("cloud_knn", {"k": 3}), ("cloud", {"vertex_block": False})):
        raw._plan[key] = value
        with pytest.raises(ValueError, match="the cloud batch was not built at `capacity`"):
            GraphedTrainStep(None, None, raw, [], capacity=wrong, device=torch.device("cpu"))
        del raw._plan[key]


SELECTION_CASES = [("v65_k1", None), ("v129_k8", None), ("b3_65_k3", None), ("boundary_130_k1", None), ("lattice_72_k3", None),
                   ("coincident_70_k3", None), ("one_point_65_k3", None), ("nan_vertex_2x70_k3", None), ("clique_66_k65", None),
                   ("lattice_72_k3", 1), ("lattice_72_k3", 8), ("one_point_65_k3", 63), ("v65_k1", 64), ("v65_k1", 63)]


@pytest.mark.parametrize("name,k", SELECTION_CASES, ids=[f"{n}{'' if k is None else '_as_k%d' % k}" for n, k in SELECTION_CASES])
def test_selection_and_symmetrisation_match_the_rank_rule(pkg, name, k):
    """cloud_knn_select_kernel (the k-th smallest sum by bisection on its bits, two bits a pass; every smaller sum and the first
    ties in ascending index) and cloud_knn_mask_kernel (the ballot over the one word of every other vertex), restated word by
    word in cloud_knn_lift_helpers, against the rank rule as knn_lift_helpers.brute_force_neighbours loops it."""
    c = CK.CASES[name]
    k = c["k"] if k is None else k
    p = CK.points_of(name).astype(np.float64).reshape(c["B"], c["V"], c["n"])
    for g in range(c["B"]):
        dirs, masks = CK.kernel_masks(p[g], k)
        brute = KH.brute_force_neighbours(p[g], k)
        named = np.zeros((c["V"], c["V"]), dtype=bool)
        for a, nb in enumerate(brute):
            named[a, sorted(nb)] = True
        assert np.array_equal(named, CK.directed_neighbours(p[g], k))
        for a in range(c["V"]):
            assert dirs[a] == CK.words_of(named[a]), (g, a)
            assert masks[a] == CK.words_of(named[a] | named[:, a]), (g, a)


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on."""
    _, _, _, cap, want = CK.reference("v129_k8")
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert CK.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert CK.differences(swapped, want) == ["edge_index"]
    wrong = clone()                                        # one vertex of one edge in another word
    row = int(want["node_types"].eq(1).nonzero()[0])
    wrong["x_ind"][row, 1] += 64
    assert CK.differences(wrong, want) == ["x_ind"]
    count = clone()
    count["counts"][2] += 1
    assert CK.differences(count, want) == ["counts"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert CK.differences(filler, want) == ["node_types"]
    narrower = clone()                                     # ... and shapes and dtypes count
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert CK.differences(narrower, want) == ["batch"]
    # one neighbour more for one vertex is another complex
    other = CK.fast_structure(CK.points_of("v129_k8"), 1, 9, 2)
    assert other["counts"][1] > CK.fast_structure(CK.points_of("v129_k8"), 1, 8, 2)["counts"][1]
