"""Shared by tests/test_hull_lift_cpu.py and tests/test_hull_lift_gpu.py: the point sets of the convex-hull lift, its host
reference (pad_batch(collate([hull_complex(..., method="exact")]), capacity) on the float64 copy of the very float32 points
the device gets, and hull_facets' volumes - host and device state the same expression in the same order, so no margin is
needed and the degenerate sets are part of the cases), the facet rule restated with plain Python floats, the closed-form
positions of csrc/lift.hip WITH the facet table T restated on the host (next to rips_lift_helpers.closed_form_structure,
which takes triangles and cofaces from the neighbour masks), hulls-shaped data for the model tests."""
import itertools
import math

import numpy as np
import torch

from rips_lift_helpers import STRUCTURE, counts_of, differences, _popc, _below, _above  # noqa: F401
from knn_lift_helpers import GUARD, buffers, capacity_for, guarded, guards_intact  # noqa: F401

# name: (graphs, vertices per graph, point dimension, max_dim, seed, capacity mode, kind of points)
CASES = {
    "task_3x8_r5": (3, 8, 5, 2, 1, "spare", "normal"),                   # the hulls task's shape
    "all_subsets_2x6_r5": (2, 6, 5, 2, 2, "spare", "normal"),            # V = n + 1: every subset is a facet
    "plane_2x7_r2": (2, 7, 2, 2, 3, "spare", "normal"),                  # facets are edges: no triangle, interior vertices
    "space_2x12_r3": (2, 12, 3, 2, 4, "spare", "normal"),
    "r4_2x9": (2, 9, 4, 2, 5, "spare", "normal"),
    "strides_1x16_r5": (1, 16, 5, 2, 6, "spare", "normal"),              # 4368 candidates: 18 strides of 256 threads
    "second_scan_pass_300x5_r4": (300, 5, 4, 2, 7, "spare", "normal"),
    "cube_2x8_r3": (2, 8, 3, 2, 8, "spare", "cube"),                     # graph 0: the unit cube's corners, no facet
    "pyramid_2x5_r3": (2, 5, 3, 2, 9, "spare", "pyramid"),               # graph 0: a square pyramid, the four sides only
    "coincident_2x6_r3": (2, 6, 3, 2, 0, "spare", "coincident"),         # every point the same: no facet anywhere
    "nan_2x8_r5": (2, 8, 5, 2, 10, "spare", "nan"),                      # graph 1 has one NaN coordinate: no facet there
    "interior_2x6_r3": (2, 6, 3, 2, 11, "spare", "interior"),            # vertex 4 of every graph strictly inside
    "max_dim_1_3x8_r5": (3, 8, 5, 1, 1, "spare", "normal"),
    "exact_capacity_3x8_r5": (3, 8, 5, 2, 1, "exact", "normal"),
}

CUBE = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float32)
PYRAMID = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1]], dtype=np.float32)


def make_points(kind, seed, n_graphs, verts, dim):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n_graphs * verts, dim)).astype(np.float32)
    if kind == "cube":
        pts[:8] = CUBE
    elif kind == "pyramid":
        pts[:5] = PYRAMID
    elif kind == "coincident":
        pts = np.tile(np.array([[0.5, -1.25, 2.0]], dtype=np.float32)[:, :dim], (n_graphs * verts, 1))
    elif kind == "nan":
        pts[verts + 2, 1] = np.nan                            # vertex 2 of graph 1
    elif kind == "interior":
        p = pts.reshape(n_graphs, verts, dim)
        p[:, 4] = (p[:, :4].mean(axis=1) * 0.999).astype(np.float32)     # inside the simplex of the vertices 0..3
    else:
        assert kind == "normal"
    return np.ascontiguousarray(pts)


def split(points32, n_graphs):
    return np.asarray(points32).astype(np.float64).reshape(n_graphs, -1, points32.shape[-1])


def host_lift(points32, n_graphs, max_dim):
    """The collated, unpadded host batch of the float64 copy of the points, by the exact rule."""
    from csmpn.data import complexes as cx
    return cx.collate([cx.hull_complex(p, max_dim, method="exact") for p in split(points32, n_graphs)])


def host_volumes(points32, n_graphs):
    """hull_facets' volumes, float64 [n_graphs]."""
    from csmpn.data import complexes as cx
    return np.array([cx.hull_facets(p)[1] for p in split(points32, n_graphs)])


_REFERENCES = {}


def reference(name):
    """(points float32, max_dim, capacity, {structure tensor name: CPU tensor} + counts, volumes float64) of a case; computed
    once and shared - callers must not change it."""
    if name not in _REFERENCES:
        from csmpn.data import complexes as cx
        B, V, n, max_dim, seed, mode, kind = CASES[name]
        pts = make_points(kind, seed, B, V, n)
        raw = host_lift(pts, B, max_dim)
        cap = capacity_for(raw, max_dim, mode)
        padded = cx.pad_batch(raw, cap)
        want = {key: getattr(padded, key) for key in STRUCTURE}
        want["counts"] = torch.tensor(counts_of(raw, max_dim), dtype=torch.int64)
        _REFERENCES[name] = (pts, max_dim, cap, want, host_volumes(pts, B))
    return _REFERENCES[name]


# ----------------------------------------------------------------------------------------------- the rule in plain floats

def _det(rows, cols):
    """Laplace expansion along the first row over `cols` ascending, ((a0 d0 - a1 d1) + a2 d2) - ..., Python floats."""
    if len(cols) == 1:
        return rows[0][cols[0]]
    acc = 0.0
    for k, c in enumerate(cols):
        term = rows[0][c] * _det(rows[1:], [x for x in cols if x != c])
        acc = term if k == 0 else (acc - term if k & 1 else acc + term)
    return acc


def sides_of(p, F):
    """[side(F, q) for every vertex q of the graph] by the rule of the issue, one candidate, Python floats."""
    n = len(F)
    origin = [float(x) for x in p[F[0]]]
    rows = [[float(p[f][j]) - origin[j] for j in range(n)] for f in F[1:]]
    normal = []
    for j in range(n):
        d = _det(rows, [c for c in range(n) if c != j])
        normal.append(-d if (n - 1 + j) & 1 else d)
    out = []
    for q in range(len(p)):
        s = normal[0] * (float(p[q][0]) - origin[0])
        for j in range(1, n):
            s = s + normal[j] * (float(p[q][j]) - origin[j])
        out.append(s)
    return out


def brute_force_facets(p):
    """(facets, smallest |side| over every candidate and every vertex outside it) of one graph, candidate by candidate."""
    V, n = p.shape
    facets, smallest = [], math.inf
    for F in itertools.combinations(range(V), n):
        s = [x for q, x in enumerate(sides_of(p, F)) if q not in F]
        if all(x > 0 for x in s) or all(x < 0 for x in s):
            facets.append(F)
        smallest = min([smallest] + [abs(x) if x == x else 0.0 for x in s])
    return facets, smallest


def brute_force_volume(p):
    """The volume with the sum taken in the order of the issue: thread = rank % 256, then the halving tree per 64, then the
    four wave sums left to right."""
    V, n = p.shape
    partial = [0.0] * 256
    for rank, F in enumerate(itertools.combinations(range(V), n)):
        s = sides_of(p, F)
        out = [x for q, x in enumerate(s) if q not in F]
        if all(x > 0 for x in out) or all(x < 0 for x in out):
            partial[rank % 256] = partial[rank % 256] + abs(s[0])
    waves = []
    for w in range(4):
        x = partial[64 * w:64 * w + 64]
        for d in (32, 16, 8, 4, 2, 1):
            x = [x[i] + x[i + d] for i in range(d)]
        waves.append(x[0])
    return (((waves[0] + waves[1]) + waves[2]) + waves[3]) / math.factorial(n)


# ----------------------------------------------------------------------------------------------- closed forms on the host

def facet_tables(p):
    """(mask [V], T [V][V]) of one graph as lift_hull_kernel forms them: every facet ORs its other vertices into mask[a] and
    its third vertices into T[a][b]."""
    V = len(p)
    m, T = [0] * V, [[0] * V for _ in range(V)]
    for F in brute_force_facets(p)[0]:
        bits = sum(1 << f for f in F)
        for a in F:
            m[a] |= bits & ~(1 << a)
            for b in F:
                if b != a:
                    T[a][b] |= bits & ~(1 << a) & ~(1 << b)
    return m, T


def closed_form_structure(points32, n_graphs, max_dim, capacity):
    """The structure tensors as csrc/lift.hip places them for the hull lift: rips_lift_helpers.closed_form_structure with the
    triangles of an edge = T[a][b] & above(b) and its cofaces = T[a][b]. None if the batch does not fit."""
    B = n_graphs
    p = split(points32, B)
    V = p.shape[1]
    tabs, n1, n2 = [], [], []
    for g in range(B):
        m, T = facet_tables(p[g])
        tabs.append((m, T))
        up = [m[a] & _above(a) for a in range(V)]
        n1.append(sum(_popc(u) for u in up))
        n2.append(sum(_popc(T[a][b] & _above(b)) for a in range(V) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0)
    N1, N2 = sum(n1), sum(n2)
    E = B * V * (V - 1) + 5 * N1 + 12 * N2
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
        m, T = tabs[g]
        up = [m[a] & _above(a) for a in range(V)]
        tri = [sum(_popc(T[a][b] & _above(b)) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
        cof = [sum(_popc(T[a][b]) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
        scan = lambda xs: [sum(xs[:i]) for i in range(V)]
        deg_s, up_s, tri_s, cof_s = scan([_popc(x) for x in m]), scan([_popc(x) for x in up]), scan(tri), scan(cof)
        VV = V * (V - 1)
        o1 = adj0
        o2 = o1 + 2 * n1[g]
        o3 = adj0 + VV + n1[g]
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
                if b != a and not (b > a and (m[a] >> b) & 1):
                    put(o2 + a * (V - 1) - up_s[a] + b - (1 if b > a else 0) - _popc(up[a] & _below(b)), row0 + a, row0 + b, 0, 0)
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
        adj0 += VV + 5 * n1[g] + 12 * n2[g]
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


# ----------------------------------------------------------------------------------------------- hulls-shaped data

def hulls_case(seed, n_graphs=4, verts=8, dim=5):
    """(points float32 [B V, 5], the collated host batch of their exact hull complexes laid out as hulls samples: `input` =
    the points in the vertex rows, `target` = hull_facets' volumes as float32)."""
    from csmpn.data import complexes as cx
    pts = np.random.default_rng(seed).standard_normal((n_graphs * verts, dim)).astype(np.float32)
    graphs = []
    for p in split(pts, n_graphs):
        c = cx.hull_complex(p, 2, method="exact")
        inp = torch.zeros(c.n_simplices, dim, dtype=torch.float32)
        inp[:verts] = torch.from_numpy(p.astype(np.float32))
        c.features["input"] = inp
        c.labels["target"] = torch.tensor(cx.hull_facets(p)[1], dtype=torch.float32)
        graphs.append(c)
    return pts, cx.collate(graphs)
