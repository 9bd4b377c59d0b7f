"""Shared by tests/test_clique_lift_cpu.py and tests/test_clique_lift_gpu.py: the graphs, points and thresholds of the
thresholded clique lift, its host reference (pad_batch(collate([clique_complex(...)]), capacity) on the float64 copy of the very
float32 points the device gets - host and device take the same float64 sums, so ties are part of the cases), the rule restated
as plain loops over masks (what lift_filter_kernel forms), the closed-form positions of csrc/lift.hip WITH the table T restated
on the host, and md17-shaped data over edge lists of changing length. Guarded buffers and the comparison come from
knn_lift_helpers."""
import itertools
import math
import os

import numpy as np
import torch

from knn_lift_helpers import (STRUCTURE, counts_of, differences, make_points, capacity_for, guarded, buffers, guards_intact,  # noqa: F401
                              pair_sums, knn_masks, MD17_FRAMES, MD17_VERTEX_FEATURES, GUARD, _popc, _below, _above)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INF = math.inf
MIN_GAP = 1e-4                                             # the fixture's conditioning (relative)


# ----------------------------------------------------------------------------------------------- the fixture

def fixture():
    return np.load(os.path.join(GOLD, "complexes_th_ref.npz"))


def fixture_cases(g=None):
    g = fixture() if g is None else g
    return sorted({key.split("/")[0] for key in g.files})


def graph_values(points, edges):
    """(the pairs a < b of G, their lengths, the triples of G, their areas) in float64, by plain loops."""
    p = np.asarray(points, dtype=np.float64)
    pairs = sorted({(min(a, b), max(a, b)) for a, b in np.asarray(edges).T.tolist() if a != b})
    present = set(pairs)
    triples = [t for t in itertools.combinations(range(len(p)), 3) if all(q in present for q in itertools.combinations(t, 2))]
    lengths = np.array([math.sqrt(sum((p[a, j] - p[b, j]) ** 2 for j in range(p.shape[1]))) for a, b in pairs])
    areas = []
    for a, b, c in triples:
        u, v = p[b] - p[a], p[c] - p[a]
        areas.append(0.5 * math.sqrt(max(float(u @ u) * float(v @ v) - float(u @ v) ** 2, 0.0)))
    return pairs, lengths, triples, np.array(areas)


def relative_gap(th, values):
    return float(np.min(np.abs(values - th) / np.maximum(np.abs(values), th))) if len(values) else INF


def hollow_and_brought_back(x1, x2, n_vertices, pairs, lengths, edge_th):
    """(triples of 1-simplices that bound no 2-simplex, 1-simplices longer than edge_th)."""
    e, t = {tuple(r) for r in np.asarray(x1).tolist()}, {tuple(r) for r in np.asarray(x2).tolist()}
    hollow = sum(1 for s in itertools.combinations(range(n_vertices), 3)
                 if s not in t and all(q in e for q in itertools.combinations(s, 2)))
    back = sum(1 for q, length in zip(pairs, lengths) if length > edge_th and q in e)
    return hollow, back


# ----------------------------------------------------------------------------------------------- graphs and thresholds

def local_lists(global_list, n_graphs, verts):
    """The cleaned per-graph lists [2, n_g] of local ids of a global list: padding and self-loops dropped."""
    ei = np.asarray(global_list, dtype=np.int64).reshape(2, -1)
    keep = (ei[0] >= 0) & (ei[0] != ei[1])
    ei = ei[:, keep]
    return [ei[:, ei[0] // verts == g] - g * verts for g in range(n_graphs)]


def knn_list(points32, n_graphs, k):
    """The global list of the k-nearest-neighbour graphs (knn_edges on the float64 copy), graph after graph."""
    from csmpn.data import complexes as cx
    p = np.asarray(points32).astype(np.float64).reshape(n_graphs, -1, points32.shape[-1])
    V = p.shape[1]
    return np.concatenate([cx.knn_edges(p[g], k).numpy() + g * V for g in range(n_graphs)], axis=1)


def complete_list(n_graphs, verts):
    one = np.array([(a, b) for a in range(verts) for b in range(a + 1, verts)], dtype=np.int64).T
    return np.concatenate([one + g * verts for g in range(n_graphs)], axis=1)


def gap_midpoint(values, q):
    """(the threshold, its relative distance to the nearest value): midway in the WIDEST gap between neighbouring sorted values
    among the five around the q quantile."""
    v = np.unique(values[np.isfinite(values)])
    if len(v) < 2:
        return (float(v[0]) * 2 + 1.0 if len(v) else 1.0), INF
    i = max(0, min(int(q * len(v)) - 1, len(v) - 2))
    lo, hi = max(0, i - 2), min(len(v) - 2, i + 2)
    j = max(range(lo, hi + 1), key=lambda t: v[t + 1] - v[t])
    th = float(0.5 * (v[j] + v[j + 1]))
    return th, relative_gap(th, v)


def batch_values(points32, lists):
    """(edge lengths, triangle areas) of the graphs G of a batch as the rule measures them: sqrt(s) and sqrt(g) / 2."""
    from csmpn.data import complexes as cx
    B = len(lists)
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    lengths, areas = [], []
    for g in range(B):
        pairs, _, triples, _ = graph_values(p[g], lists[g])
        s = cx._pair_sums(p[g])
        lengths += [math.sqrt(s[a, b]) for a, b in pairs]
        if triples:
            areas += (0.5 * np.sqrt(np.maximum(cx._gram_dets(p[g], np.asarray(triples)), 0.0))).tolist()
    return np.asarray(lengths), np.asarray(areas)


def midpoint_thresholds(points32, lists, qe, qt):
    """Thresholds at gap midpoints of the batch's own values; the squared thresholds keep a relative 1e-9 from every s and g."""
    lengths, areas = batch_values(points32, lists)
    edge_th, ge = (INF, INF) if qe is None else gap_midpoint(lengths, qe)
    tri_th, gt = (INF, INF) if qt is None else gap_midpoint(areas, qt)
    assert min(ge, gt) >= 1e-9, (ge, gt)
    return edge_th, tri_th


def lattice_case():
    """16 points of the 4 x 4 integer lattice in R^2, G = every pair with s <= 5 (lengths 1, sqrt 2, 2, sqrt 5): every
    intermediate of s and g is an exact small integer."""
    pts = np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.float32)
    pairs = [(a, b) for a in range(16) for b in range(a + 1, 16) if float(((pts[a] - pts[b]) ** 2).sum()) <= 5.0]
    return pts, np.array(pairs, dtype=np.int64).T.copy()


def _dirty(clean, n_graphs, verts, seed):
    """`clean` with duplicates, reversed copies, self-loops and padding mixed in, shuffled."""
    rng = np.random.default_rng(seed)
    loops = np.tile(rng.integers(0, n_graphs * verts, size=5), (2, 1))
    cols = np.concatenate([clean, clean[::-1, ::2], clean[:, ::3], loops, np.full((2, 9), -1, dtype=np.int64)], axis=1)
    return np.ascontiguousarray(cols[:, rng.permutation(cols.shape[1])])


def _build(name):
    """(points float32 [B V, n], B, the global list or None, k or None, edge_th, tri_th, max_dim, capacity mode, the cleaned
    per-graph lists of G)."""
    from csmpn.data import complexes as cx
    if name in ("triangle_kept_1x3", "triangle_dropped_1x3"):
        pts = np.array([[0, 0, 0], [2, 0, 0], [0, 2, 0]], dtype=np.float32)              # area 2
        glist = np.array([[0, 1, 2], [1, 2, 0]], dtype=np.int64)
        return pts, 1, glist, None, INF, 2.5 if "kept" in name else 1.5, 2, "spare"
    if name == "complete_2x64":                            # bit 63 and every row of the 64-wide table; few triangles survive
        pts = make_points("normal", 41, 2, 64, 3)
        glist = complete_list(2, 64)
        _, tri_th = midpoint_thresholds(pts, local_lists(glist, 2, 64), None, 0.004)
        return pts, 2, glist, None, INF, tri_th, 2, "spare"
    if name == "edge_th_0_2x9":                            # every 1-simplex comes from a kept triangle
        pts = make_points("normal", 42, 2, 9, 3)
        glist = knn_list(pts, 2, 4)
        _, tri_th = midpoint_thresholds(pts, local_lists(glist, 2, 9), None, 0.5)
        return pts, 2, glist, None, 0.0, tri_th, 2, "spare"
    if name == "tri_th_0_2x8":                             # every edge kept, no triangle: all hollow
        pts = make_points("normal", 43, 2, 8, 3)
        return pts, 2, knn_list(pts, 2, 4), None, INF, 0.0, 2, "spare"
    if name == "empty_graph_3x6":                          # graph 1 has no entry in the list
        pts = make_points("normal", 44, 3, 6, 3)
        glist = knn_list(pts, 3, 3)
        glist = glist[:, glist[0] // 6 != 1]
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(glist, 3, 6), 0.7, 0.5)
        return pts, 3, glist, None, edge_th, tri_th, 2, "spare"
    if name == "second_scan_pass_300x5":
        pts = make_points("normal", 45, 300, 5, 2)
        glist = knn_list(pts, 300, 3)
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(glist, 300, 5), 0.5, 0.5)
        return pts, 300, glist, None, edge_th, tri_th, 2, "spare"
    if name == "dirty_list_2x7":
        pts = make_points("normal", 46, 2, 7, 3)
        clean = knn_list(pts, 2, 3)
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(clean, 2, 7), 0.6, 0.6)
        return pts, 2, _dirty(clean, 2, 7, 46), None, edge_th, tri_th, 2, "spare"
    if name == "max_dim_1_4x7":                            # a kept triangle brings its pairs back for max_dim = 1 as well
        pts = make_points("normal", 47, 4, 7, 3)
        glist = knn_list(pts, 4, 3)
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(glist, 4, 7), 0.4, 0.6)
        return pts, 4, glist, None, edge_th, tri_th, 1, "spare"
    if name == "exact_capacity_4x9":
        pts = make_points("normal", 48, 4, 9, 3)
        glist = knn_list(pts, 4, 4)
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(glist, 4, 9), 0.5, 0.5)
        return pts, 4, glist, None, edge_th, tri_th, 2, "exact"
    if name in ("lattice_ties_1x16", "lattice_below_1x16"):
        pts, glist = lattice_case()
        below = "below" in name
        return pts, 1, glist, None, float(np.nextafter(1.0, 0.0)) if below else 1.0, float(np.nextafter(1.0, 0.0)) if below else 1.0, 2, "spare"
    if name in ("nan_vertex_2x8", "nan_vertex_inf_2x8"):   # vertex 2 of graph 1; point_dim 5
        pts = make_points("nan", 5, 2, 8, 5)
        glist = knn_list(pts, 2, 3)
        if "inf" in name:
            return pts, 2, glist, None, INF, INF, 2, "spare"
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(glist, 2, 8), 0.8, 0.8)
        return pts, 2, glist, None, edge_th, tri_th, 2, "spare"
    if name == "aspirin_from_k3":                          # the fixture's aspirin case, G from the device's own kNN kernel
        g = fixture()
        c = "knn_21_k3_s0_e5_t5"
        return g[f"{c}/points"], 1, None, 3, float(g[f"{c}/edge_th"]), float(g[f"{c}/tri_th"]), 2, "spare"
    if name == "knn_source_3x33_k4":                       # both mask halves from the k source, finite thresholds
        pts = make_points("normal", 49, 3, 33, 2)
        edge_th, tri_th = midpoint_thresholds(pts, local_lists(knn_list(pts, 3, 4), 3, 33), 0.6, 0.5)
        return pts, 3, None, 4, edge_th, tri_th, 2, "spare"
    raise KeyError(name)


CASES = ["triangle_kept_1x3", "triangle_dropped_1x3", "complete_2x64", "edge_th_0_2x9", "tri_th_0_2x8", "empty_graph_3x6",
         "second_scan_pass_300x5", "dirty_list_2x7", "max_dim_1_4x7", "exact_capacity_4x9", "lattice_ties_1x16",
         "lattice_below_1x16", "nan_vertex_2x8", "nan_vertex_inf_2x8", "aspirin_from_k3", "knn_source_3x33_k4"]


def host_lift(points32, n_graphs, lists, edge_th, tri_th, max_dim):
    """The collated, unpadded host batch of the float64 copy of the points over the per-graph local lists."""
    from csmpn.data import complexes as cx
    p = np.asarray(points32).astype(np.float64).reshape(n_graphs, -1, points32.shape[-1])
    return cx.collate([cx.clique_complex(p[g], lists[g], edge_th, tri_th, max_dim) for g in range(n_graphs)])


_REFERENCES = {}


def reference(name):
    """(points float32, B, global list or None, k or None, edge_th, tri_th, max_dim, capacity, the cleaned per-graph lists,
    {structure tensor name: CPU tensor} + counts) of a case; computed once and shared - callers must not change it."""
    if name not in _REFERENCES:
        from csmpn.data import complexes as cx
        pts, B, glist, k, edge_th, tri_th, max_dim, mode = _build(name)
        V = pts.shape[0] // B
        lists = local_lists(knn_list(pts, B, k) if glist is None else glist, B, V)
        raw = host_lift(pts, B, lists, edge_th, tri_th, max_dim)
        cap = capacity_for(raw, max_dim, mode)
        padded = cx.pad_batch(raw, cap)
        want = {key: getattr(padded, key) for key in STRUCTURE}
        want["counts"] = torch.tensor(counts_of(raw, max_dim), dtype=torch.int64)
        _REFERENCES[name] = (pts, B, glist, k, edge_th, tri_th, max_dim, cap, lists, want)
    return _REFERENCES[name]


# ----------------------------------------------------------------------------------------------- the rule as loops over masks

def list_masks(local_list, verts):
    m = [0] * verts
    for a, b in np.asarray(local_list).T.tolist():
        if a != b:
            m[a] |= 1 << b
            m[b] |= 1 << a
    return m


def filter_masks(p, gm, edge_th, tri_th):
    """(final masks, T[a][b]) of one graph as lift_filter_kernel forms them, by scalar loops in Python floats (IEEE double,
    one rounding per operation)."""
    V, n = p.shape
    e2, t4 = edge_th * edge_th, 4.0 * tri_th * tri_th
    nn = lambda x: INF if x != x else x
    fm = [0] * V
    T = [[0] * V for _ in range(V)]
    for a in range(V):
        for b in range(V):
            if a != b and (gm[a] >> b) & 1:
                s = 0.0
                for j in range(n):
                    d = float(p[a, j]) - float(p[b, j])
                    s = s + d * d
                if nn(s) <= e2:
                    fm[a] |= 1 << b
    for a, b, c in itertools.combinations(range(V), 3):
        if not ((gm[a] >> b) & 1 and (gm[a] >> c) & 1 and (gm[b] >> c) & 1):
            continue
        uu = vv = uv = 0.0
        for j in range(n):
            u, v = float(p[b, j]) - float(p[a, j]), float(p[c, j]) - float(p[a, j])
            uu, vv, uv = uu + u * u, vv + v * v, uv + u * v
        if nn(uu * vv - uv * uv) <= t4:
            for x, y, z in ((a, b, c), (a, c, b), (b, c, a)):
                T[x][y] |= 1 << z
                T[y][x] |= 1 << z
                fm[x] |= 1 << y
                fm[y] |= 1 << x
    return fm, T


def closed_form_structure(points32, n_graphs, lists, edge_th, tri_th, max_dim, capacity):
    """The structure tensors as csrc/lift.hip places them for the thresholded clique lift: every position from popcounts of the
    FINAL masks and of the table T and the scans over vertices and edges, block 3 directly behind block 1. None if the batch
    does not fit."""
    B = n_graphs
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    V = p.shape[1]
    per_graph, n1, n2 = [], [], []
    for g in range(B):
        m, T = filter_masks(p[g], list_masks(lists[g], V), edge_th, tri_th)
        up = [m[a] & _above(a) for a in range(V)]
        per_graph.append((m, T, up))
        n1.append(sum(_popc(u) for u in up))
        n2.append(sum(_popc(T[a][b] & _above(b)) for a in range(V) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0)
    N1, N2 = sum(n1), sum(n2)
    E = 6 * N1 + 12 * N2
    cap = list(capacity.simplices) + [0] * (3 - len(capacity.simplices))
    if N1 > cap[1] or (max_dim >= 2 and N2 > cap[2]) or E > capacity.edges:
        return None
    S_cap = capacity.rows
    x_ind = np.zeros((S_cap, max_dim + 1), np.int64)
    types, graph = np.zeros(S_cap, np.int64), np.zeros(S_cap, np.int64)
    ei, et = np.zeros((2, capacity.edges), np.int64), np.zeros((capacity.edges, 2), np.int64)
    ptr = np.zeros(B + 1, np.int64)

    def put_row(r, d, g, vs):
        x_ind[r, :len(vs)] = vs
        types[r], graph[r] = d, g

    def put(pos, s, t, ts, tt):
        ei[0, pos], ei[1, pos], et[pos] = s, t, (ts, tt)

    row0 = adj0 = 0
    for g in range(B):
        m, T, up = per_graph[g]
        on = max_dim >= 2
        tri = [sum(_popc(T[a][b] & _above(b)) for b in range(V) if (up[a] >> b) & 1) if on else 0 for a in range(V)]
        cof = [sum(_popc(T[a][b]) for b in range(V) if (up[a] >> b) & 1) if on else 0 for a in range(V)]
        scan = lambda xs: [sum(xs[:i]) for i in range(V)]
        deg_s, up_s, tri_s, cof_s = scan([_popc(x) for x in m]), scan([_popc(x) for x in up]), scan(tri), scan(cof)
        o1 = adj0
        o3 = o1 + 2 * n1[g]
        o4 = o3 + 2 * n1[g]
        o5 = o4 + 2 * n1[g]
        o6 = o5 + 6 * n2[g]
        o7 = o6 + 3 * n2[g]
        e0 = row0 + V
        t0 = e0 + n1[g]
        ptr[g] = row0
        eidx = lambda lo, hi: up_s[lo] + _popc(up[lo] & _below(hi))
        for a in range(V):
            put_row(row0 + a, 0, g, [a])
            tb, cb = tri_s[a], cof_s[a]
            for b in range(V):
                if (m[a] >> b) & 1:
                    put(o1 + deg_s[a] + _popc(m[a] & _below(b)), row0 + b, row0 + a, 0, 0)
                if not (up[a] >> b) & 1:
                    continue
                e = eidx(a, b)
                erow = e0 + e
                put_row(erow, 1, g, [a, b])
                put(o3 + 2 * e, row0 + a, erow, 0, 1)
                put(o3 + 2 * e + 1, row0 + b, erow, 0, 1)
                put(o4 + 2 * e, erow, row0 + a, 1, 0)
                put(o4 + 2 * e + 1, erow, row0 + b, 1, 0)
                if max_dim < 2:
                    continue
                for c in range(b + 1, V):
                    if (T[a][b] >> c) & 1:
                        trow = t0 + tb
                        put_row(trow, 2, g, [a, b, c])
                        for j, f in enumerate((erow, e0 + eidx(a, c), e0 + eidx(b, c))):
                            put(o6 + 3 * tb + j, f, trow, 1, 2)
                            put(o7 + 3 * tb + j, trow, f, 2, 1)
                        tb += 1
                for w in range(V):
                    if (T[a][b] >> w) & 1:
                        put(o5 + 2 * cb, e0 + eidx(min(a, w), max(a, w)), erow, 1, 1)
                        put(o5 + 2 * cb + 1, e0 + eidx(min(b, w), max(b, w)), erow, 1, 1)
                        cb += 1
        row0 += V + n1[g] + n2[g]
        adj0 += 6 * n1[g] + 12 * n2[g]
    ptr[B] = row0
    fill1 = cap[1] - N1
    n_fill = S_cap - row0
    for i in range(n_fill):
        d = 1 if i < fill1 else 2
        put_row(row0 + i, d, B - 1, list(range(d + 1)))
    for j in range(capacity.edges - E):
        i = j % n_fill
        d = 1 if i < fill1 else 2
        put(E + j, row0 + i, row0 + i, d, d)
    t = torch.from_numpy
    return {"x_ind": t(x_ind), "node_types": t(types), "batch": t(graph), "x_ind_batch": t(graph.copy()), "ptr": t(ptr),
            "x_ind_ptr": t(ptr.copy()), "edge_index": t(ei), "edge_types": t(et),
            "counts": torch.tensor([B * V, N1] + ([N2] if max_dim >= 2 else []) + [E], dtype=torch.int64)}


# ----------------------------------------------------------------------------------------------- md17-shaped data

MD17_EDGE_TH, MD17_TRI_TH = 1.7, 0.8


def md17_case(seed, n_graphs=4, verts=6, extra=0):
    """knn_lift_helpers.md17_case over an edge list: the k = 3 nearest-neighbour list of every graph plus `extra` random pairs
    per graph (lists of different lengths), lifted by clique_complex at (MD17_EDGE_TH, MD17_TRI_TH): (points float32 [B V, 3],
    per-vertex features {loc, vel, charges: [B V, 10, .]}, the per-vertex target y, the collated host batch with those
    features in its vertex rows, the global list int64 [2, n])."""
    from csmpn.data import complexes as cx
    pts = np.random.default_rng(seed).standard_normal((n_graphs * verts, 3)).astype(np.float32)
    rng = np.random.default_rng(1000 + seed)
    N, F = n_graphs * verts, MD17_FRAMES
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    vf = {"loc": f32(pts)[:, None, :] + 0.05 * f32(rng.standard_normal((N, F, 3))),
          "vel": 0.1 * f32(rng.standard_normal((N, F, 3))),
          "charges": f32(rng.integers(1, 9, size=(N, 1, 1))).expand(N, F, 1).contiguous()}
    y = vf["loc"] + 0.1 * f32(rng.standard_normal((N, F, 3)))
    glist = knn_list(pts, n_graphs, 3)
    if extra:
        more = rng.integers(0, verts, size=(2, n_graphs, extra)) + (np.arange(n_graphs) * verts)[None, :, None]
        glist = np.concatenate([glist, more.reshape(2, -1)], axis=1)
    lists = local_lists(glist, n_graphs, verts)
    p64 = pts.astype(np.float64).reshape(n_graphs, verts, 3)
    graphs = []
    for g in range(n_graphs):
        c = cx.clique_complex(p64[g], lists[g], MD17_EDGE_TH, MD17_TRI_TH, 2)
        for k, v in vf.items():
            t = torch.zeros((c.n_simplices,) + tuple(v.shape[1:]))
            t[:verts] = v[g * verts:(g + 1) * verts]
            c.features[k] = t
        graphs.append(c)
    b = cx.collate(graphs)
    b.y = y
    b._names.append("y")
    return pts, vf, y, b, torch.from_numpy(np.ascontiguousarray(glist))
