"""Shared by tests/test_cloud_lift_cpu.py and tests/test_cloud_lift_gpu.py: the case table of the Rips lift of point clouds
(csmpn_cloud_lift, more than 64 vertices per graph), the conditioning every case must have, and a vectorised numpy
restatement of lift + to_complex + collate + pad_batch for the Rips rule in both vertex_block forms - lift() is a Python
loop over pairs of simplices and needs about a minute on the dense cases; the CPU tests hold the restatement against it on
the cases where it is quick."""
import numpy as np
import torch

import rips_lift_helpers as R
import varying_helpers as VH

STRUCTURE = R.STRUCTURE
MARGIN = 1e-4          # every pair sum s of a case that is not exact keeps |s - dis^2| >= MARGIN * dis^2
differences = R.differences

# name: graphs B, vertices per graph V, point dimension, dis, max_dim, how the points are made (points_of), capacity mode
# ("spare" = the batch's counts + varying_helpers.SPARE, "exact" = its counts), host = lift() takes under about 2 s,
# exact = both rules (norm <= dis on the host, s <= dis^2 on the device) are exact on the case instead of the margin
_DEG = 6.0             # expected degree of the "sparse" clouds: uniform points in a cube, dis = 1
CASES = {
    "sparse_64": dict(B=1, V=64, n=3, dis=1.0, max_dim=2, kind="sparse", seed=1, host=True),
    "sparse_65": dict(B=1, V=65, n=3, dis=1.0, max_dim=2, kind="sparse", seed=2, host=True),      # vertex 64 alone in word 1
    "sparse_66": dict(B=1, V=66, n=3, dis=1.0, max_dim=2, kind="sparse", seed=3, host=True),
    "sparse_128": dict(B=1, V=128, n=3, dis=1.0, max_dim=2, kind="sparse", seed=4, host=True),
    "sparse_129": dict(B=1, V=129, n=3, dis=1.0, max_dim=2, kind="sparse", seed=5, host=True),
    "sparse_200": dict(B=1, V=200, n=3, dis=1.0, max_dim=2, kind="sparse", seed=6, host=False),   # 4 words, the last partial; 50 tiles
    "b3_65": dict(B=3, V=65, n=3, dis=1.0, max_dim=2, kind="sparse", seed=7, host=True),
    # (second pass of the offsets scan; 624 000 pairs: coordinates in sixteenths, dis^2 between two multiples of 1 / 256)
    "b300_65": dict(B=300, V=65, n=2, dis=float(np.sqrt(256.5 / 256.0)), max_dim=2, kind="sixteenths", seed=8, host=False),
    "placed_200": dict(B=1, V=200, n=2, dis=1.0, max_dim=2, kind="placed", host=False),
    "clique66_in_130": dict(B=1, V=130, n=3, dis=1.0, max_dim=2, kind="clique", first=31, size=66, seed=9, host=False),
    "complete_65_dim1": dict(B=1, V=65, n=3, dis=1.0, max_dim=1, kind="clique", first=0, size=65, seed=10, host=False),
    "lattice_tie_72": dict(B=1, V=72, n=2, dis=2.0, max_dim=2, kind="lattice", host=True, exact=True),
    "lattice_ulp_below_72": dict(B=1, V=72, n=2, dis=float(np.nextafter(2.0, 0.0)), max_dim=2, kind="lattice", host=True, exact=True),
    "dis0_coincident_70": dict(B=1, V=70, n=3, dis=0.0, max_dim=2, kind="coincident", seed=11, host=True, exact=True),
    "nan_vertex_70": dict(B=2, V=70, n=3, dis=1.0, max_dim=2, kind="nan", seed=12, host=True),
    "max_dim_1_100": dict(B=2, V=100, n=3, dis=1.0, max_dim=1, kind="sparse", seed=13, host=True),
    "exact_capacity_66": dict(B=2, V=66, n=3, dis=1.0, max_dim=2, kind="sparse", seed=14, mode="exact", host=True),
    "relift_96_a": dict(B=2, V=96, n=3, dis=1.0, max_dim=2, kind="sparse", seed=15, host=True),
    "relift_96_b": dict(B=2, V=96, n=3, dis=1.0, max_dim=2, kind="sparse", seed=16, host=True),
    "relift_96_c": dict(B=2, V=96, n=3, dis=1.0, max_dim=2, kind="sparse", seed=17, host=True),
    "grid_4096": dict(B=1, V=4096, n=2, dis=float(np.sqrt(650.5 / 256.0)), max_dim=2, kind="grid", seed=18, host=False),
}
SMALL = {"tiny_12": dict(B=2, V=12, n=3, dis=1.0, max_dim=2, kind="sparse", seed=19, host=True),
         "tiny_16": dict(B=1, V=16, n=3, dis=1.2, max_dim=2, kind="sparse", seed=20, host=True)}     # V <= 16: against clique_complex
CASES.update(SMALL)

PLACED = {                                                    # vertex: (cluster, x, y); clusters lie 1000 apart
    63: (1, 0.0, 0.0), 64: (1, 0.8, 0.0), 65: (1, 1.6, 0.0), 62: (1, 0.4, 0.6),      # edges (63,64), (64,65); triangle (62,63,64)
    127: (2, 0.0, 0.0), 128: (2, 0.7, 0.0),                                           # edge (127,128)
    0: (3, 0.0, 0.0), 199: (3, 0.6, 0.0),                                             # edge (0,199): vertex V - 1 has a neighbour
    5: (4, 0.0, 0.0), 70: (4, 0.6, 0.0), 140: (4, 0.3, 0.5),                          # a triangle over three words
    # the edge (66, 195) with cofaces in word 0 (below both ends), word 2 (between them) and above 195; 2 and 67 hang on one end
    66: (5, 0.0, 0.0), 195: (5, 0.5, 0.0), 10: (5, 0.25, 0.4), 130: (5, 0.25, -0.4), 197: (5, 0.25, 0.1),
    2: (5, -0.8, 0.0), 67: (5, 1.3, 0.0),
}


def pair_sums(p64):
    """s[g, a, b] = sum_j (p_a[j] - p_b[j])^2 of [B, V, n] float64 points, j ascending, one rounding per operation."""
    s = np.zeros(p64.shape[:2] + (p64.shape[1],))
    for j in range(p64.shape[2]):
        d = p64[:, :, None, j] - p64[:, None, :, j]
        s = s + d * d
    return s


def conditioning_ok(points32, B, dis, exact=False):
    """The margin of the case - or, for an exact case, that the host rule and the device rule name the same pairs and that the
    arithmetic is exact (integer coordinates, or dis = 0 where only a sum of exactly 0 counts)."""
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    iu = np.triu_indices(p.shape[1], 1)
    for g in range(B):                                       # one graph at a time: V^2 doubles
        s = pair_sums(p[g:g + 1])[0][iu]
        s = s[~np.isnan(s)]
        if exact:
            if not (dis == 0.0 or (np.all(p[g] == np.round(p[g])) and float(np.abs(p[g]).max()) < 2 ** 20)):
                return False
            if not np.array_equal(np.sqrt(s) <= dis, s <= dis * dis):
                return False
        elif s.size and float(np.abs(s - dis * dis).min()) < MARGIN * dis * dis:
            return False
    return True


def _make_points(c, seed):
    B, V, n, kind = c["B"], c["V"], c["n"], c["kind"]
    rng = np.random.default_rng(seed)
    if kind in ("sparse", "nan", "coincident", "sixteenths"):
        ball = {2: np.pi, 3: 4.0 * np.pi / 3.0}[n] * c["dis"] ** n if c["dis"] > 0 else 1.0
        side = (V * ball / _DEG) ** (1.0 / n)
        pts = rng.uniform(0.0, side, (B * V, n)) if kind != "sixteenths" else rng.integers(0, int(side * 16), (B * V, n)) / 16.0
        if kind == "nan":
            pts[65] = np.nan                                 # graph 0, a vertex of word 1
            pts[V + 3, 1] = np.nan                           # graph 1, one coordinate
        if kind == "coincident":
            pts[[64, 65, 69]] = pts[3]                       # four points at distance 0, over two words
            pts[20] = pts[10]
    elif kind == "placed":
        pts = np.stack([np.arange(V) * 10.0, np.full(V, -500.0)], axis=1)      # everything else is isolated
        for v, (cluster, x, y) in PLACED.items():
            pts[v] = (1000.0 * cluster + x, y)
    elif kind == "clique":
        pts = np.stack([np.arange(V) * 10.0 + 100.0] + [np.zeros(V)] * (n - 1), axis=1)
        first, size = c["first"], c["size"]
        pts[first:first + size] = rng.uniform(0.0, 0.45, (size, n))             # diameter < 0.45 sqrt(3) < 1
    elif kind == "lattice":
        pts = np.stack(np.meshgrid(np.arange(9.0), np.arange(8.0), indexing="ij"), axis=-1).reshape(V, 2)
        pts = pts[rng.permutation(V)]                        # neighbours of the lattice lie in both words
    elif kind == "grid":
        side = int(round(V ** 0.5))
        base = np.stack(np.meshgrid(np.arange(side, dtype=np.float64), np.arange(side, dtype=np.float64), indexing="ij"), axis=-1)
        # jitter in sixteenths: every pair sum is a multiple of 1 / 256 and dis^2 = 650.5 / 256 lies between two of them
        pts = (base.reshape(V, 2) + rng.integers(-2, 3, (V, 2)) / 16.0)[rng.permutation(V)]
    else:
        raise KeyError(kind)
    return pts.astype(np.float32)


_POINTS = {}


def points_of(name):
    """The float32 points [B * V, n] of a case, its conditioning asserted; a seed that misses the margin is replaced by
    seed + 1000, + 2000, ... as rips_lift_helpers.seeded_points does."""
    if name not in _POINTS:
        c = CASES[name]
        seeds = range(c["seed"], c["seed"] + 10000, 1000) if "seed" in c else (0,)
        for seed in seeds:
            pts = _make_points(c, seed)
            if conditioning_ok(pts, c["B"], c["dis"], c.get("exact", False)):
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the conditioning")
        _POINTS[name] = pts
    return _POINTS[name]


# ------------------------------------------------------------------------------------------------ the fast restatement

def _graph_structure(p64, dis2, max_dim, vertex_block):
    """Rows and adjacencies of one graph in its own row numbering (vertices, edges, triangles), in the order of lift() +
    to_complex(): (x_ind, node_types, edge_index, edge_types, n1, n2)."""
    V = len(p64)
    with np.errstate(invalid="ignore"):
        close = pair_sums(p64[None])[0] <= dis2              # False for a NaN
    close[np.arange(V), np.arange(V)] = False
    upper = np.triu(close, 1)
    ea, eb = np.nonzero(upper)                               # lexicographic
    n1 = len(ea)
    key = ea.astype(np.int64) * V + eb
    eid = lambda lo, hi: V + np.searchsorted(key, lo.astype(np.int64) * V + hi)   # row of the edge (lo, hi), lo < hi
    ce = cw = te = tc = np.zeros(0, np.int64)
    if max_dim >= 2 and n1:
        parts, step = [], max(1, (1 << 25) // V)             # the common neighbours of a slice of the edges at a time
        for i in range(0, n1, step):
            e, w = np.nonzero(close[ea[i:i + step]] & close[eb[i:i + step]])
            parts.append((e + i, w))
        ce, cw = (np.concatenate(x) for x in zip(*parts))    # (edge, coface vertex): edge-major, the vertex ascending
        third = cw > eb[ce]
        te, tc = ce[third], cw[third]                        # (edge (a, b), c > b): the triangles, lexicographic
    n2 = len(te)
    x_ind = np.zeros((V + n1 + n2, max_dim + 1), np.int64)
    x_ind[:V, 0] = np.arange(V)
    x_ind[V:V + n1, 0], x_ind[V:V + n1, 1] = ea, eb
    if n2:
        x_ind[V + n1:, 0], x_ind[V + n1:, 1], x_ind[V + n1:, 2] = ea[te], eb[te], tc
    types = np.concatenate([np.zeros(V, np.int64), np.ones(n1, np.int64), np.full(n2, 2, np.int64)])
    erow, trow = V + np.arange(n1), V + n1 + np.arange(n2)
    pair = lambda x, y: np.stack([x, y], axis=1).ravel()
    t, u = np.nonzero(close)                                 # block 1: for s, for its neighbours u ascending: (u, s)
    blocks = [(u, t, 0, 0)]
    if vertex_block:                                         # block 2: every ordered pair but i < j that is an edge
        i, j = np.nonzero(~upper & ~np.eye(V, dtype=bool))
        blocks.append((i, j, 0, 0))
    b3 = (pair(ea, eb), np.repeat(erow, 2))
    blocks += [(b3[0], b3[1], 0, 1), (b3[1], b3[0], 1, 0)]
    if max_dim >= 2:
        a, b = ea[ce], eb[ce]
        blocks.append((pair(eid(np.minimum(a, cw), np.maximum(a, cw)), eid(np.minimum(b, cw), np.maximum(b, cw))), np.repeat(erow[ce], 2), 1, 1))
        b6 = (np.stack([erow[te], eid(ea[te], tc), eid(eb[te], tc)], axis=1).ravel(), np.repeat(trow, 3))
        blocks += [(b6[0], b6[1], 1, 2), (b6[1], b6[0], 2, 1)]
    ei = np.stack([np.concatenate([x[0] for x in blocks]), np.concatenate([x[1] for x in blocks])]).astype(np.int64)
    et = np.concatenate([np.tile(np.array([[x[2], x[3]]], np.int64), (len(x[0]), 1)) for x in blocks])
    return x_ind, types, ei, et, n1, n2


def fast_structure(points32, B, dis, max_dim, vertex_block, capacity=None):
    """The structure tensors and counts of pad_batch(collate([rips_complex(points_g, dis, max_dim, vertex_block)]), capacity)
    - of the collated batch itself for capacity = None - as CPU int64 tensors. ValueError where pad_batch raises one."""
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    V = p.shape[1]
    graphs = [_graph_structure(p[g], dis * dis, max_dim, vertex_block) for g in range(B)]
    sizes = np.array([len(g[1]) for g in graphs], np.int64)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    x_ind = np.concatenate([g[0] for g in graphs])
    types = np.concatenate([g[1] for g in graphs])
    graph = np.repeat(np.arange(B, dtype=np.int64), sizes)
    ei = np.concatenate([g[2] + ptr[i] for i, g in enumerate(graphs)], axis=1)
    et = np.concatenate([g[3] for g in graphs])
    N1, N2, S, E = sum(g[4] for g in graphs), sum(g[5] for g in graphs), int(ptr[-1]), int(ei.shape[1])
    counts = [B * V, N1] + ([N2] if max_dim >= 2 else []) + [E]
    raw = dict(x_ind=x_ind, node_types=types, batch=graph, ptr=ptr, edge_index=ei, edge_types=et, counts=counts)
    return _as_tensors(raw if capacity is None else _padded(raw, capacity))


def _padded(raw, capacity):
    """pad_batch on the arrays of fast_structure: fillers dimension by dimension, self-loops on them round-robin."""
    x_ind, types, graph, ptr, ei, et, counts = (raw[k] for k in ("x_ind", "node_types", "batch", "ptr", "edge_index", "edge_types", "counts"))
    max_dim, B, S, E = len(counts) - 2, len(ptr) - 1, int(ptr[-1]), counts[-1]
    N1, N2 = counts[1], counts[2] if max_dim >= 2 else 0
    if True:
        cap = list(capacity.simplices)
        if cap[0] != counts[0] or N1 > cap[1] or (max_dim >= 2 and N2 > cap[2]) or E > capacity.edges:
            raise ValueError("the batch does not fit the capacity")
        fill = [0, cap[1] - N1] + ([cap[2] - N2] if max_dim >= 2 else [])
        n_fill, e_fill = sum(fill), capacity.edges - E
        if e_fill and not n_fill:
            raise ValueError("filler adjacencies without a filler row")
        f_types = np.repeat(np.arange(max_dim + 1, dtype=np.int64), fill)
        cols = np.arange(max_dim + 1, dtype=np.int64)[None, :]
        x_ind = np.concatenate([x_ind, np.where(cols <= f_types[:, None], cols, 0)])
        types = np.concatenate([types, f_types])
        graph = np.concatenate([graph, np.full(n_fill, B - 1, np.int64)])
        f_rows = S + np.arange(e_fill, dtype=np.int64) % max(n_fill, 1)
        ei = np.concatenate([ei, np.stack([f_rows, f_rows])], axis=1)
        f_et = f_types[f_rows - S] if e_fill else np.zeros(0, np.int64)
        et = np.concatenate([et, np.stack([f_et, f_et], axis=1)])
    return dict(x_ind=x_ind, node_types=types, batch=graph, ptr=ptr, edge_index=ei, edge_types=et, counts=counts)


def _as_tensors(arrays):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {k: t(arrays[k]) for k in ("x_ind", "node_types", "batch", "ptr", "edge_index", "edge_types")}
    out["x_ind_batch"], out["x_ind_ptr"] = out["batch"].clone(), out["ptr"].clone()
    out["counts"] = torch.tensor(arrays["counts"], dtype=torch.int64)
    return out


def capacity_for(counts, max_dim, mode):
    from csmpn.data.complexes import BatchCapacity
    c = list(counts)
    if mode == "exact":
        return BatchCapacity(tuple(c[:-1]), c[-1])
    assert mode == "spare"
    return BatchCapacity((c[0],) + tuple(r + s for r, s in zip(c[1:-1], VH.SPARE[0])), c[-1] + VH.SPARE[1])


_REFERENCES = {}


def reference(name, vertex_block):
    """(points float32, dis, max_dim, capacity, {structure tensor name: CPU tensor} + counts) of a case by the fast
    restatement; computed once and shared - callers must not change it."""
    key = (name, bool(vertex_block))
    if key not in _REFERENCES:
        c = CASES[name]
        pts = points_of(name)
        counts = fast_structure(pts, c["B"], c["dis"], c["max_dim"], vertex_block)["counts"].tolist()
        cap = capacity_for(counts, c["max_dim"], c.get("mode", "spare"))
        _REFERENCES[key] = (pts, c["dis"], c["max_dim"], cap, fast_structure(pts, c["B"], c["dis"], c["max_dim"], vertex_block, cap))
    return _REFERENCES[key]


def host_complexes(name, vertex_block):
    """The complexes of a case as rips_complex builds them on the float64 copy of its points (lift(): slow)."""
    from csmpn.data import complexes as cx
    c = CASES[name]
    p = points_of(name).astype(np.float64).reshape(c["B"], c["V"], c["n"])
    return [cx.rips_complex(p[g], c["dis"], c["max_dim"], vertex_block=vertex_block) for g in range(c["B"])]


def host_structure(name, vertex_block, capacity):
    """pad_batch(collate([rips_complex(...)]), capacity) of a case: the structure tensors and the counts."""
    from csmpn.data import complexes as cx
    raw = cx.collate(host_complexes(name, vertex_block))
    padded = cx.pad_batch(raw, capacity)
    want = {k: getattr(padded, k) for k in STRUCTURE}
    want["counts"] = torch.tensor(R.counts_of(raw, CASES[name]["max_dim"]), dtype=torch.int64)
    return want


# ------------------------------------------------------------------------------------------------ md17-shaped data, V = 70

MD17_DIS, MD17_VERTS = 1.0, 70


def md17_cloud_case(seed, vertex_block=False):
    """rips_lift_helpers.md17_case for ONE graph of 70 vertices: (points float32 [70, 3], per-vertex features, the per-vertex
    target y, the collated host batch of the float64 copy of the points with those features in its vertex rows)."""
    from csmpn.data import complexes as cx
    c = dict(B=1, V=MD17_VERTS, n=3, dis=MD17_DIS, kind="sparse")
    for s in range(seed, seed + 10000, 1000):
        pts = _make_points(c, s)
        if conditioning_ok(pts, 1, MD17_DIS):
            break
    rng = np.random.default_rng(1000 + seed)
    N, F = MD17_VERTS, R.MD17_FRAMES
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    vf = {"loc": f32(pts)[:, None, :] + 0.05 * f32(rng.standard_normal((N, F, 3))),
          "vel": 0.1 * f32(rng.standard_normal((N, F, 3))),
          "charges": f32(rng.integers(1, 9, size=(N, 1, 1))).expand(N, F, 1).contiguous()}
    y = vf["loc"] + 0.1 * f32(rng.standard_normal((N, F, 3)))
    comp = cx.rips_complex(pts.astype(np.float64), MD17_DIS, 2, vertex_block=vertex_block)
    for k, v in vf.items():
        t = torch.zeros((comp.n_simplices,) + tuple(v.shape[1:]))
        t[:N] = v
        comp.features[k] = t
    b = cx.collate([comp])
    b.y = y
    b._names.append("y")
    return pts, vf, y, b


# ------------------------------------------------------------------------- the closed forms of the kernels on the host

_M64 = (1 << 64) - 1


def _popc(x):
    return bin(x).count("1")


def _above_in(word, v):
    """The bits of word `word` that belong to vertices above v (csrc/lift.hip: above_in)."""
    return 0 if word < v >> 6 else _M64 & ~((1 << ((v & 63) + 1)) - 1) if word == v >> 6 else _M64


def closed_form_structure(points32, B, dis, max_dim, vertex_block, capacity):
    """The real part of the structure tensors as the kernels of csmpn_cloud_lift place it: W = ceil(V / 64) mask words per
    vertex, the rank table, the scanned per-vertex counts, and every position a popcount away from them - word by word, with
    the carries over the words, as cloud_scatter_vertex walks them. Fillers as pad_batch lays them out."""
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    V = p.shape[1]
    W = (V + 63) // 64
    below = lambda b: (1 << b) - 1
    per_graph = []
    for g in range(B):
        with np.errstate(invalid="ignore"):
            close = pair_sums(p[g:g + 1])[0] <= dis * dis
        m = [[sum(1 << i for i in range(64) if 64 * w + i < V and 64 * w + i != a and close[a, 64 * w + i]) for w in range(W)] for a in range(V)]
        rank = [[sum(_popc(m[a][x] & _above_in(x, a)) for x in range(w)) for w in range(W)] for a in range(V)]
        deg = [sum(_popc(x) for x in m[a]) for a in range(V)]
        up = [sum(_popc(m[a][w] & _above_in(w, a)) for w in range(W)) for a in range(V)]
        nbrs = lambda a: [64 * w + i for w in range(W) for i in range(64) if (m[a][w] & _above_in(w, a)) >> i & 1]
        tri = [sum(_popc(m[a][w] & m[b][w] & _above_in(w, b)) for b in nbrs(a) for w in range(W)) if max_dim >= 2 else 0 for a in range(V)]
        cof = [sum(_popc(m[a][w] & m[b][w]) for b in nbrs(a) for w in range(W)) if max_dim >= 2 else 0 for a in range(V)]
        scan = lambda xs: [sum(xs[:i]) for i in range(V)]
        per_graph.append((m, rank, scan(deg), scan(up), scan(tri), scan(cof), sum(up), sum(tri)))
    N1, N2 = sum(x[6] for x in per_graph), sum(x[7] for x in per_graph)
    VV = V * (V - 1) if vertex_block else 0
    E = B * VV + (5 if vertex_block else 6) * N1 + 12 * N2
    S_cap = capacity.rows
    x_ind = np.full((S_cap, max_dim + 1), -1, np.int64)
    types, graph = np.full(S_cap, -1, np.int64), np.full(S_cap, -1, np.int64)
    ei, et = np.full((2, capacity.edges), -1, np.int64), np.full((capacity.edges, 2), -1, np.int64)
    ptr = np.zeros(B + 1, np.int64)

    def put_row(r, d, g, vs):
        assert types[r] == -1                              # every position is written once
        x_ind[r] = 0
        x_ind[r, :len(vs)] = vs
        types[r], graph[r] = d, g

    def put(pos, s, t, ts, tt):
        assert ei[0, pos] == -1
        ei[0, pos], ei[1, pos], et[pos] = s, t, (ts, tt)

    row0 = adj0 = 0
    for g in range(B):
        m, rank, deg_s, up_s, tri_s, cof_s, n1, n2 = per_graph[g]
        edge = lambda lo, hi: up_s[lo] + rank[lo][hi >> 6] + _popc(m[lo][hi >> 6] & _above_in(hi >> 6, lo) & below(hi & 63))
        o1 = adj0
        o2 = o1 + 2 * n1
        o3 = adj0 + VV + n1 if vertex_block else o2
        o4 = o3 + 2 * n1
        o5 = o4 + 2 * n1
        o6 = o5 + 6 * n2
        o7 = o6 + 3 * n2
        e0 = row0 + V
        t0 = e0 + n1
        ptr[g] = row0
        for a in range(V):
            put_row(row0 + a, 0, g, [a])
            nd, nu, tb, cb = deg_s[a], up_s[a], tri_s[a], cof_s[a]
            for w in range(W):
                maw = m[a][w]
                uaw = maw & _above_in(w, a)
                for lane in range(64):
                    b = 64 * w + lane
                    if maw >> lane & 1:
                        put(o1 + nd + _popc(maw & below(lane)), row0 + b, row0 + a, 0, 0)
                    if vertex_block and b < V and b != a and not uaw >> lane & 1:
                        put(o2 + a * (V - 1) + b - (1 if b > a else 0) - nu - _popc(uaw & below(lane)), row0 + a, row0 + b, 0, 0)
                nd += _popc(maw)
                for lane in range(64):                     # the wave scan: the edge lanes in ascending order
                    if not uaw >> lane & 1:
                        continue
                    b = 64 * w + lane
                    e = nu + _popc(uaw & below(lane))
                    erow = e0 + e
                    put_row(erow, 1, g, [a, b])
                    put(o3 + 2 * e, row0 + a, erow, 0, 1)
                    put(o3 + 2 * e + 1, row0 + b, erow, 0, 1)
                    put(o4 + 2 * e, erow, row0 + a, 1, 0)
                    put(o4 + 2 * e + 1, erow, row0 + b, 1, 0)
                    if max_dim < 2:
                        continue
                    for x in range(w, W):
                        ubx = m[b][x] & _above_in(x, b)
                        for ci in range(64):
                            if (m[a][x] & ubx) >> ci & 1:
                                c = 64 * x + ci
                                trow = t0 + tb
                                ebc = e0 + up_s[b] + rank[b][x] + _popc(ubx & below(ci))
                                put_row(trow, 2, g, [a, b, c])
                                for j, f in enumerate((erow, e0 + edge(a, c), ebc)):
                                    put(o6 + 3 * tb + j, f, trow, 1, 2)
                                    put(o7 + 3 * tb + j, trow, f, 2, 1)
                                tb += 1
                    for x in range(W):
                        for i in range(64):
                            if (m[a][x] & m[b][x]) >> i & 1:
                                y = 64 * x + i
                                put(o5 + 2 * cb, e0 + edge(min(a, y), max(a, y)), erow, 1, 1)
                                put(o5 + 2 * cb + 1, e0 + edge(min(b, y), max(b, y)), erow, 1, 1)
                                cb += 1
                nu += _popc(uaw)
        row0 += V + n1 + n2
        adj0 += VV + (5 if vertex_block else 6) * n1 + 12 * n2
    ptr[B] = row0
    assert adj0 == E
    fill1 = capacity.simplices[1] - N1
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
