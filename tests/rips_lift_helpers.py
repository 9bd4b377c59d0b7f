"""Shared by tests/test_rips_lift_cpu.py and tests/test_rips_lift_gpu.py: seeded point sets with a checked distance margin,
the host reference of the device lift (pad_batch(collate([rips_complex(...)]), capacity) on the float64 copy of the very
float32 points the device gets), the comparison of the structure tensors, and the closed-form positions of csrc/lift.hip
restated on the host (popcounts of neighbour masks + scans), which the CPU tests hold against lift()."""
import numpy as np
import torch

STRUCTURE = ("x_ind", "node_types", "batch", "x_ind_batch", "ptr", "x_ind_ptr", "edge_index", "edge_types")
MARGIN = 1e-6          # no pair distance within MARGIN * dis of dis (double rounding is of the order of 1e-16)

# name: (graphs, vertices per graph, point dimension, dis, max_dim, seed, capacity mode)
#   capacity modes: "spare" = the batch's counts + varying_helpers.SPARE, "exact" = its counts (no filler at all)
CASES = {
    "rips_seed1": (4, 6, 3, 1.6, 2, 1, "spare"),
    "rips_seed2": (4, 6, 3, 1.6, 2, 2, "spare"),
    "rips_seed3": (4, 6, 3, 1.6, 2, 3, "spare"),
    "rips_seed4": (4, 6, 3, 1.6, 2, 4, "spare"),
    "nba_16x11_r2": (16, 11, 2, 1.0, 2, 5, "spare"),
    "all_mask_bits_3x64": (3, 64, 3, 0.9, 2, 6, "spare"),
    "mask_halves_2x33": (2, 33, 3, 1.0, 2, 7, "spare"),
    "smallest_triangle_2x3": (2, 3, 3, 2.0, 2, 8, "spare"),
    "one_graph_1x3": (1, 3, 3, 2.0, 2, 9, "spare"),
    "max_dim_1_2x2": (2, 2, 3, 1.5, 1, 10, "spare"),
    "complete_2x12": (2, 12, 3, 1e3, 2, 11, "spare"),
    "vertices_only_2x8": (2, 8, 3, 1e-3, 2, 12, "spare"),
    "second_scan_pass_300x4": (300, 4, 3, 1.4, 2, 13, "spare"),
    "exact_capacity": (4, 6, 3, 1.6, 2, 14, "exact"),
    "coincident_points": (2, 7, 3, 1.2, 2, 15, "spare"),      # vertex 3 of graph 1 moved onto vertex 1: distance 0
}


def min_margin(points, n_graphs, dis):
    """Smallest | |p_a - p_b| - dis | / dis over the pairs inside a graph, in float64."""
    p = np.asarray(points, dtype=np.float64).reshape(n_graphs, -1, points.shape[-1])
    d = np.linalg.norm(p[:, :, None] - p[:, None], axis=-1)
    iu = np.triu_indices(p.shape[1], 1)
    return float(np.abs(d[:, iu[0], iu[1]] - dis).min()) / dis


def seeded_points(seed, n_graphs, verts, dim, dis):
    """Standard normal float32 points [n_graphs * verts, dim] whose pair distances keep the margin; a seed that misses it
    is replaced by seed + 1000, + 2000, ... (returned: points, the seed used)."""
    for s in range(seed, seed + 10000, 1000):
        pts = np.random.default_rng(s).standard_normal((n_graphs * verts, dim)).astype(np.float32)
        if min_margin(pts, n_graphs, dis) > MARGIN:
            return pts, s
    raise AssertionError(f"no seed {seed} + 1000 k keeps the margin")


def host_lift(points32, n_graphs, dis, max_dim):
    """The collated, unpadded host batch of the float64 copy of the points; asserts the margin first."""
    from csmpn.data import complexes as cx
    assert min_margin(points32, n_graphs, dis) > MARGIN, "a pair distance lies within the margin of dis: take another seed"
    p = np.asarray(points32).astype(np.float64).reshape(n_graphs, -1, points32.shape[-1])
    return cx.collate([cx.rips_complex(p[g], dis, max_dim) for g in range(n_graphs)])


def counts_of(batch, max_dim):
    rows = torch.bincount(batch.node_types, minlength=max_dim + 1).tolist()
    return rows + [int(batch.edge_index.shape[1])]


def capacity_for(batch, max_dim, mode):
    from csmpn.data.complexes import BatchCapacity
    import varying_helpers as V
    c = counts_of(batch, max_dim)
    if mode == "exact":
        return BatchCapacity(tuple(c[:-1]), c[-1])
    assert mode == "spare"
    return BatchCapacity((c[0],) + tuple(r + s for r, s in zip(c[1:-1], V.SPARE[0])), c[-1] + V.SPARE[1])


_REFERENCES = {}


def reference(name):
    """(points float32, dis, max_dim, capacity, {structure tensor name: CPU tensor} + counts) of a case; computed once and
    shared - callers must not change it."""
    if name not in _REFERENCES:
        from csmpn.data import complexes as cx
        B, V, n, dis, max_dim, seed, mode = CASES[name]
        pts, _ = seeded_points(seed, B, V, n, dis)
        if name == "coincident_points":
            pts[V + 3] = pts[V + 1]
        raw = host_lift(pts, B, dis, max_dim)
        cap = capacity_for(raw, max_dim, mode)
        padded = cx.pad_batch(raw, cap)
        want = {k: getattr(padded, k) for k in STRUCTURE}
        want["counts"] = torch.tensor(counts_of(raw, max_dim), dtype=torch.int64)
        _REFERENCES[name] = (pts, dis, max_dim, cap, want)
    return _REFERENCES[name]


def differences(got, want):
    """Names of the tensors of `want` that `got` does not hold exactly (shape, dtype, every entry)."""
    out = []
    for k, w in want.items():
        g = got[k].cpu() if torch.is_tensor(got[k]) else torch.as_tensor(got[k])
        if g.dtype != w.dtype or tuple(g.shape) != tuple(w.shape) or not torch.equal(g, w):
            out.append(k)
    return out


# ----------------------------------------------------------------------------------------------- closed forms on the host

def _popc(x):
    return bin(x).count("1")


def _below(b):
    return (1 << b) - 1


def _above(a):
    return ((1 << 64) - 1) & ~((1 << (a + 1)) - 1)


def closed_form_structure(points32, n_graphs, dis, max_dim, capacity):
    """The structure tensors as csrc/lift.hip places them: every position from popcounts of the 64-bit neighbour masks and
    the scans over vertices and edges - no sorting, no search. None if the batch does not fit."""
    B = n_graphs
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    V = p.shape[1]
    masks, n1, n2 = [], [], []
    for g in range(B):
        m = [0] * V
        for a in range(V):
            for b in range(V):
                if a != b and float(((p[g, a] - p[g, b]) ** 2).sum()) <= dis * dis:
                    m[a] |= 1 << b
        masks.append(m)
        up = [m[a] & _above(a) for a in range(V)]
        n1.append(sum(_popc(u) for u in up))
        n2.append(sum(_popc(up[a] & m[b] & _above(b)) for a in range(V) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0)
    N1, N2 = sum(n1), sum(n2)
    E = B * V * (V - 1) + 5 * N1 + 12 * N2
    cap = list(capacity.simplices) + [0] * (3 - len(capacity.simplices))
    if N1 > cap[1] or (max_dim >= 2 and N2 > cap[2]) or E > capacity.edges:
        return None
    S_cap, M = capacity.rows, max_dim + 1
    x_ind = np.zeros((S_cap, M), np.int64)
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
        m = masks[g]
        up = [m[a] & _above(a) for a in range(V)]
        tri = [sum(_popc(up[a] & m[b] & _above(b)) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
        cof = [sum(_popc(m[a] & m[b]) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
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
                    if ((up[a] & m[b]) >> c) & 1:
                        trow = t0 + tb
                        put_row(trow, 2, g, [a, b, c])
                        for j, f in enumerate((erow, e0 + eidx(a, c), e0 + eidx(b, c))):
                            put(o6 + 3 * tb + j, f, trow, 1, 2)
                            put(o7 + 3 * tb + j, trow, f, 2, 1)
                        tb += 1
                for w in range(V):
                    if ((m[a] & m[b]) >> w) & 1:
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


# ----------------------------------------------------------------------------------------------- md17-shaped data

MD17_DIS, MD17_FRAMES = 1.6, 10
MD17_VERTEX_FEATURES = ("loc", "vel", "charges")


def md17_case(seed, n_graphs=4, verts=6):
    """varying_helpers.rips_batch(md17=True)-shaped data from float32 points: (points float32 [B V, 3], per-vertex
    features {loc, vel, charges: [B V, 10, .]}, the per-vertex target y, the collated host batch of the float64 copy of
    the points with those features in its vertex rows)."""
    from csmpn.data import complexes as cx
    pts, _ = seeded_points(seed, n_graphs, verts, 3, MD17_DIS)
    rng = np.random.default_rng(1000 + seed)
    N, F = n_graphs * verts, MD17_FRAMES
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    vf = {"loc": f32(pts)[:, None, :] + 0.05 * f32(rng.standard_normal((N, F, 3))),
          "vel": 0.1 * f32(rng.standard_normal((N, F, 3))),
          "charges": f32(rng.integers(1, 9, size=(N, 1, 1))).expand(N, F, 1).contiguous()}
    y = vf["loc"] + 0.1 * f32(rng.standard_normal((N, F, 3)))
    p64 = pts.astype(np.float64).reshape(n_graphs, verts, 3)
    assert min_margin(pts, n_graphs, MD17_DIS) > MARGIN
    graphs = []
    for g in range(n_graphs):
        c = cx.rips_complex(p64[g], MD17_DIS, 2)
        for k, v in vf.items():
            t = torch.zeros((c.n_simplices,) + tuple(v.shape[1:]))
            t[:verts] = v[g * verts:(g + 1) * verts]
            c.features[k] = t
        graphs.append(c)
    b = cx.collate(graphs)
    b.y = y
    b._names.append("y")
    return pts, vf, y, b
