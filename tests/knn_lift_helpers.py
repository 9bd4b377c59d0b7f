"""Shared by tests/test_knn_lift_cpu.py and tests/test_knn_lift_gpu.py: the point sets of the k-nearest-neighbour lift, its
host reference (pad_batch(collate([knn_clique_complex(...)]), capacity) on the float64 copy of the very float32 points the
device gets - host and device take the same float64 sum, so no distance margin is needed and ties are part of the cases),
the neighbour rule restated as a double loop, the closed-form positions of csrc/lift.hip WITHOUT the vertex block restated
on the host (next to rips_lift_helpers.closed_form_structure, which has the block), guarded device buffers, md17-shaped data."""
import numpy as np
import torch

from rips_lift_helpers import STRUCTURE, counts_of, differences, MD17_FRAMES, MD17_VERTEX_FEATURES  # noqa: F401

GUARD = -77

# name: (graphs, vertices per graph, point dimension, k, max_dim, seed, capacity mode, kind of points)
#   capacity modes: "spare" = the batch's counts + varying_helpers.SPARE, "exact" = its counts (no filler at all)
CASES = {
    "all_mask_bits_3x64": (3, 64, 3, 3, 2, 1, "spare", "outliers"),      # vertices 0 and 63 far out: nobody names them back
    "mask_halves_2x33_k1": (2, 33, 2, 1, 2, 2, "spare", "normal"),
    "aspirin_16x21": (16, 21, 3, 3, 2, 3, "spare", "normal"),
    "complete_2x5_k4": (2, 5, 3, 4, 2, 4, "spare", "normal"),
    "complete_2x5_k10": (2, 5, 3, 10, 2, 4, "spare", "normal"),
    "lattice_1x16": (1, 16, 2, 2, 2, 0, "spare", "lattice"),             # equal distances: the index decides
    "coincident_2x6": (2, 6, 3, 2, 2, 0, "spare", "coincident"),         # every distance 0
    "nan_vertex_2x8": (2, 8, 5, 3, 2, 5, "spare", "nan"),                # NaN as +infinity; point_dim 5
    "max_dim_1_4x7": (4, 7, 3, 2, 1, 6, "spare", "normal"),
    "second_scan_pass_300x4": (300, 4, 2, 1, 2, 7, "spare", "normal"),
    "one_graph_1x21": (1, 21, 3, 3, 2, 8, "spare", "normal"),
    "exact_capacity_16x21": (16, 21, 3, 3, 2, 3, "exact", "normal"),
}


def make_points(kind, seed, n_graphs, verts, dim):
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((n_graphs * verts, dim)).astype(np.float32)
    if kind == "outliers":
        p = pts.reshape(n_graphs, verts, dim)
        p[:, 0, 0] += 50.0
        p[:, verts - 1, 0] -= 50.0
    elif kind == "lattice":
        assert dim == 2 and verts == 16
        grid = np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.float32)
        pts = np.tile(grid, (n_graphs, 1))
    elif kind == "coincident":
        pts = np.tile(np.array([[0.5, -1.25, 2.0]], dtype=np.float32)[:, :dim], (n_graphs * verts, 1))
    elif kind == "nan":
        pts[verts + 2, 1] = np.nan                            # vertex 2 of graph 1
    else:
        assert kind == "normal"
    return np.ascontiguousarray(pts)


def pair_sums(p):
    """s[a, b] of one graph in float64 by a plain loop: sum over j ascending of (p_a[j] - p_b[j])^2, NaN -> +inf."""
    V, n = p.shape
    s = np.zeros((V, V))
    for a in range(V):
        for b in range(V):
            t = 0.0
            for j in range(n):
                d = float(p[a, j]) - float(p[b, j])
                t = t + d * d
            s[a, b] = np.inf if t != t else t
    return s


def brute_force_neighbours(p, k):
    """directed[a] = the set of neighbours of a by the rule of the issue, as a double loop over (b, c)."""
    s = pair_sums(np.asarray(p, dtype=np.float64))
    V = len(s)
    out = []
    for a in range(V):
        nb = set()
        for b in range(V):
            if b == a:
                continue
            rank = sum(1 for c in range(V) if c != a and c != b and (s[a, c] < s[a, b] or (s[a, c] == s[a, b] and c < b)))
            if rank < k:
                nb.add(b)
        out.append(nb)
    return out


def host_lift(points32, n_graphs, k, max_dim):
    """The collated, unpadded host batch of the float64 copy of the points."""
    from csmpn.data import complexes as cx
    p = np.asarray(points32).astype(np.float64).reshape(n_graphs, -1, points32.shape[-1])
    return cx.collate([cx.knn_clique_complex(p[g], k, max_dim) for g in range(n_graphs)])


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
    """(points float32, k, max_dim, capacity, {structure tensor name: CPU tensor} + counts) of a case; computed once and
    shared - callers must not change it."""
    if name not in _REFERENCES:
        from csmpn.data import complexes as cx
        B, V, n, k, max_dim, seed, mode, kind = CASES[name]
        pts = make_points(kind, seed, B, V, n)
        raw = host_lift(pts, B, k, max_dim)
        cap = capacity_for(raw, max_dim, mode)
        padded = cx.pad_batch(raw, cap)
        want = {key: getattr(padded, key) for key in STRUCTURE}
        want["counts"] = torch.tensor(counts_of(raw, max_dim), dtype=torch.int64)
        _REFERENCES[name] = (pts, k, max_dim, cap, want)
    return _REFERENCES[name]


# ----------------------------------------------------------------------------------------------- closed forms on the host

def _popc(x):
    return bin(x).count("1")


def _below(b):
    return (1 << b) - 1


def _above(a):
    return ((1 << 64) - 1) & ~((1 << (a + 1)) - 1)


def knn_masks(p, k):
    """The symmetrised 64-bit neighbour masks of one graph as lift_knn_kernel forms them: the directed mask of every vertex,
    then bit b of dir[a] | bit a of dir[b]."""
    directed = brute_force_neighbours(p, k)
    V = len(directed)
    d = [sum(1 << b for b in directed[a]) for a in range(V)]
    return [d[a] | sum(((d[b] >> a) & 1) << b for b in range(V)) for a in range(V)]


def closed_form_structure(points32, n_graphs, k, max_dim, capacity):
    """The structure tensors as csrc/lift.hip places them for the kNN lift: every position from popcounts of the neighbour
    masks and the scans over vertices and edges, block 3 directly behind block 1 (no block 2). None if the batch does not fit."""
    B = n_graphs
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    V = p.shape[1]
    masks, n1, n2 = [], [], []
    for g in range(B):
        m = knn_masks(p[g], k)
        masks.append(m)
        up = [m[a] & _above(a) for a in range(V)]
        n1.append(sum(_popc(u) for u in up))
        n2.append(sum(_popc(up[a] & m[b] & _above(b)) for a in range(V) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0)
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
        m = masks[g]
        up = [m[a] & _above(a) for a in range(V)]
        tri = [sum(_popc(up[a] & m[b] & _above(b)) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
        cof = [sum(_popc(m[a] & m[b]) for b in range(V) if (up[a] >> b) & 1) if max_dim >= 2 else 0 for a in range(V)]
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


# ----------------------------------------------------------------------------------------------- guarded device buffers

def guarded(shape, dev, pad=64):
    """An int64 tensor of `shape` inside a larger buffer of guard values: (view, whole buffer, offset)."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), GUARD, dtype=torch.int64, device=dev)
    return whole[pad:pad + n].view(shape), whole, pad


def buffers(cap, n_graphs, dev):
    S, E, nd = cap.rows, cap.edges, cap.max_dim + 1
    shapes = dict(x_ind=(S, nd), node_types=(S,), batch=(S,), x_ind_batch=(S,), ptr=(n_graphs + 1,), x_ind_ptr=(n_graphs + 1,),
                  edge_index=(2, E), edge_types=(E, 2), counts=(nd + 1,))
    return {k: guarded(s, dev) for k, s in shapes.items()}


def guards_intact(bufs):
    """None, or the name of the first buffer whose guard region was written."""
    for k, (view, whole, pad) in bufs.items():
        n = view.numel()
        if not (bool((whole[:pad] == GUARD).all()) and bool((whole[pad + n:] == GUARD).all())):
            return k
    return None


# ----------------------------------------------------------------------------------------------- md17-shaped data

MD17_K = 3


def md17_case(seed, n_graphs=4, verts=6):
    """rips_lift_helpers.md17_case with the kNN clique complex: (points float32 [B V, 3], per-vertex features {loc, vel,
    charges: [B V, 10, .]}, the per-vertex target y, the collated host batch with those features in its vertex rows)."""
    from csmpn.data import complexes as cx
    pts = np.random.default_rng(seed).standard_normal((n_graphs * verts, 3)).astype(np.float32)
    rng = np.random.default_rng(1000 + seed)
    N, F = n_graphs * verts, MD17_FRAMES
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    vf = {"loc": f32(pts)[:, None, :] + 0.05 * f32(rng.standard_normal((N, F, 3))),
          "vel": 0.1 * f32(rng.standard_normal((N, F, 3))),
          "charges": f32(rng.integers(1, 9, size=(N, 1, 1))).expand(N, F, 1).contiguous()}
    y = vf["loc"] + 0.1 * f32(rng.standard_normal((N, F, 3)))
    p64 = pts.astype(np.float64).reshape(n_graphs, verts, 3)
    graphs = []
    for g in range(n_graphs):
        c = cx.knn_clique_complex(p64[g], MD17_K, 2)
        for k, v in vf.items():
            t = torch.zeros((c.n_simplices,) + tuple(v.shape[1:]))
            t[:verts] = v[g * verts:(g + 1) * verts]
            c.features[k] = t
        graphs.append(c)
    b = cx.collate(graphs)
    b.y = y
    b._names.append("y")
    return pts, vf, y, b
