"""The Rips lift on the device, the parts that need no GPU: the workspace query, every rejected argument combination of
csmpn_rips_lift (the arguments are checked before the first HIP call), rips_capacity against host-lifted batches, the closed
forms of csrc/lift.hip restated on the host against lift(), and a mutation guard for the comparison the GPU tests use."""
import ctypes as C

import pytest
import torch

import rips_lift_helpers as R
import varying_helpers as V


def test_workspace_query(pkg):
    from csmpn_hip import native
    q = native.lib().csmpn_rips_lift_workspace_bytes
    sizes = [int(q(b, 13, 2)) for b in (1, 16, 300, 5000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert int(q(16, 64, 2)) > 0 and int(q(16, 2, 1)) > 0
    assert int(q(16, 65, 2)) == 0 and int(q(16, 13, 0)) == 0 and int(q(16, 13, 3)) == 0
    assert int(q(0, 13, 2)) == 0 and int(q(16, 2, 2)) == 0 and int(q(1 << 31, 13, 2)) == 0


FAKE = 0x1000          # never dereferenced: every call below is refused before the first HIP call


def _call(lib, **over):
    """csmpn_rips_lift for 4 graphs of 6 vertices in R^3, max_dim 2, with the named arguments replaced."""
    a = dict(points=FAKE, point_dim=3, n_graphs=4, verts=6, dis=1.6, max_dim=2, cap=(24, 28, 13), cap_edges=384, x_ind=FAKE,
             x_ind_cols=3, node_types=FAKE, batch=FAKE, x_ind_batch=FAKE, ptr=FAKE, x_ind_ptr=FAKE, edge_index=FAKE,
             edge_types=FAKE, counts=FAKE, status=FAKE, workspace=FAKE, workspace_bytes=1 << 20)
    a.update(over)
    cap = None if a["cap"] is None else (C.c_int64 * len(a["cap"]))(*a["cap"])
    return lib.csmpn_rips_lift(a["points"], a["point_dim"], a["n_graphs"], a["verts"], a["dis"], a["max_dim"],
                               None if cap is None else C.addressof(cap), a["cap_edges"], a["x_ind"], a["x_ind_cols"],
                               a["node_types"], a["batch"], a["x_ind_batch"], a["ptr"], a["x_ind_ptr"], a["edge_index"],
                               a["edge_types"], a["counts"], a["status"], a["workspace"], a["workspace_bytes"], None)


REJECTED = [
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
    ("negative_dis", dict(dis=-1.0), "invalid"),
    ("nan_dis", dict(dis=float("nan")), "invalid"),
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


def test_ops_wrapper_refuses_host_tensors(pkg):
    from csmpn_hip import ops
    i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rips_lift(torch.zeros(24, 3), 4, 1.6, 2, (24, 28, 13), 384, i64(65, 3), i64(65), i64(65), i64(65), i64(5), i64(5),
                      i64(2, 384), None, None, None, torch.zeros(4096, dtype=torch.uint8))


def test_rips_capacity_counts_adjacencies(pkg):
    """rips_capacity's adjacency count is edge_index.shape[1] of host-lifted batches: the Rips batches of the varying-topology
    tests with their recorded counts, and every case of the device tests."""
    from csmpn.data import complexes as cx
    for seed, (rows, edges) in V.RIPS_COUNTS.items():
        b = V.rips_batch(seed)
        cap = cx.rips_capacity(4, 6, rows[1], rows[2])
        assert cap.edges == edges == int(b.edge_index.shape[1])
        assert cap.simplices == (24, rows[1] + 1, rows[2])
        cx.pad_batch(b, cap)                               # the spare 1-simplex is there, so this never refuses
    for name, (B, verts, _, _, max_dim, _, _) in R.CASES.items():
        want = R.reference(name)[4]["counts"].tolist()
        cap = cx.rips_capacity(B, verts, want[1], want[2] if max_dim == 2 else 0, max_dim)
        assert cap.edges == want[-1], name
        assert cap.max_dim == max_dim and cap.simplices[0] == B * verts
    with pytest.raises(ValueError):
        cx.rips_capacity(4, 6, 10, 2, max_dim=3)
    with pytest.raises(ValueError):
        cx.rips_capacity(4, 2, 10, 2, max_dim=2)


@pytest.mark.parametrize("name", list(R.CASES))
def test_closed_forms_match_host_lift(pkg, name):
    """Every position the kernels compute from popcounts and scans (restated in rips_lift_helpers.closed_form_structure) is
    the position lift() + to_complex() + collate() + pad_batch() give."""
    pts, dis, max_dim, cap, want = R.reference(name)
    got = R.closed_form_structure(pts, R.CASES[name][0], dis, max_dim, cap)
    assert R.differences(got, want) == []


def test_closed_forms_on_more_seeds(pkg):
    """Ten more seeds of 3 x 9 points, with the recorded per-graph count V (V - 1) + 5 n1 + 12 n2."""
    from csmpn.data import complexes as cx
    for seed in range(20, 30):
        pts, _ = R.seeded_points(seed, 3, 9, 3, 1.3)
        raw = R.host_lift(pts, 3, 1.3, 2)
        c = R.counts_of(raw, 2)
        assert c[3] == 3 * 9 * 8 + 5 * c[1] + 12 * c[2]
        cap = cx.rips_capacity(3, 9, c[1], c[2])
        padded = cx.pad_batch(raw, cap)
        want = {k: getattr(padded, k) for k in R.STRUCTURE}
        assert R.differences(R.closed_form_structure(pts, 3, 1.3, 2, cap), want) == []


def test_comparison_sees_single_changes(pkg):
    """Mutation guard of the comparison the GPU tests rely on."""
    _, _, _, cap, want = R.reference("rips_seed1")
    clone = lambda: {k: v.clone() for k, v in want.items()}
    assert R.differences(clone(), want) == []
    swapped = clone()                                      # one swapped adjacency pair
    swapped["edge_index"][:, [40, 41]] = swapped["edge_index"][:, [41, 40]]
    assert not torch.equal(swapped["edge_index"], want["edge_index"])
    assert R.differences(swapped, want) == ["edge_index"]
    wrong_ptr = clone()                                    # one wrong ptr entry
    wrong_ptr["ptr"][2] += 1
    assert R.differences(wrong_ptr, want) == ["ptr"]
    filler = clone()                                       # a filler 2-simplex typed 1
    last = cap.rows - 1
    assert int(want["node_types"][last]) == 2 and last >= int(want["ptr"][-1])
    filler["node_types"][last] = 1
    assert R.differences(filler, want) == ["node_types"]
    narrower = clone()                                     # ... and shapes and dtypes count
    narrower["batch"] = narrower["batch"].to(torch.int32)
    assert R.differences(narrower, want) == ["batch"]
