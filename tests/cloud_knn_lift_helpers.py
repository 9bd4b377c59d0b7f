"""Shared by tests/test_cloud_knn_lift_cpu.py and tests/test_cloud_knn_lift_gpu.py: the case table of the kNN clique lift of point
clouds (csmpn_cloud_knn_lift, more than 64 vertices per graph), the conditioning every case must have, a vectorised numpy
restatement of lift + to_complex + collate + pad_batch for the kNN rule - knn_clique_complex is a Python loop over triples and
lift() one over pairs of simplices - and the two new kernels restated word by word on the host. The row and adjacency order is
that of cloud_lift_helpers for vertex_block=False; the CPU tests hold the restatement against knn_clique_complex where that
is quick."""
import numpy as np
import torch

import cloud_lift_helpers as CL
import knn_lift_helpers as KH
import rips_lift_helpers as R

STRUCTURE = CL.STRUCTURE
MARGIN = CL.MARGIN     # a case that is no deliberate tie: (s_(k+1) - s_(k)) >= MARGIN * s_(k+1) in the sorted row of every vertex
differences = CL.differences
MD17_VERTEX_FEATURES = R.MD17_VERTEX_FEATURES

# name: graphs B, vertices per graph V, point dimension n, k, max_dim, how the points are made (make_points), capacity mode
# ("spare" = the batch's counts + varying_helpers.SPARE, the default; "exact" = its counts), host = knn_clique_complex + lift()
# take under about 2 s, tie = the case holds equal pair sums on purpose (the index decides) instead of keeping the margin
CASES = {
    "v64_k3": dict(B=1, V=64, n=3, k=3, max_dim=2, kind="normal", seed=1, host=True),              # the bits of csmpn_knn_lift
    "v65_k1": dict(B=1, V=65, n=3, k=1, max_dim=2, kind="normal", seed=2, host=True),              # vertex 64 alone in word 1
    "v66_k8": dict(B=1, V=66, n=3, k=8, max_dim=2, kind="normal", seed=3, host=False),
    "v128_k3": dict(B=1, V=128, n=2, k=3, max_dim=2, kind="normal", seed=4, host=False),
    "v129_k8": dict(B=1, V=129, n=3, k=8, max_dim=2, kind="normal", seed=5, host=False),
    "v129_k1": dict(B=1, V=129, n=3, k=1, max_dim=2, kind="normal", seed=5, host=True),
    "v200_k3": dict(B=1, V=200, n=5, k=3, max_dim=2, kind="normal", seed=6, host=False),           # 4 words, the last partial; 50 tiles
    "v1000_k8": dict(B=1, V=1000, n=3, k=8, max_dim=2, kind="normal", seed=23, host=False),         # 16 words, the last partial
    "b3_65_k3": dict(B=3, V=65, n=3, k=3, max_dim=2, kind="normal", seed=7, host=True),
    # (second pass of the offsets scan; coordinates in sixteenths: every sum is exact, equal sums are common)
    "b300_65_k3": dict(B=300, V=65, n=2, k=3, max_dim=2, kind="sixteenths", seed=8, host=False, tie=True),
    "boundary_130_k1": dict(B=1, V=130, n=2, k=1, max_dim=2, kind="boundary", seed=9, host=False),
    "outliers_3x70_k3": dict(B=3, V=70, n=3, k=3, max_dim=2, kind="outliers", seed=10, host=True),
    "clique_66_k65": dict(B=1, V=66, n=3, k=65, max_dim=2, kind="normal", seed=11, host=False),    # k = V - 1: no selection pass
    "clique_66_k100": dict(B=1, V=66, n=3, k=100, max_dim=2, kind="normal", seed=11, host=False),
    "lattice_72_k3": dict(B=1, V=72, n=2, k=3, max_dim=2, kind="lattice", seed=12, host=True, tie=True),
    "coincident_70_k3": dict(B=1, V=70, n=3, k=3, max_dim=2, kind="coincident", seed=13, host=True, tie=True),
    "one_point_65_k3": dict(B=1, V=65, n=3, k=3, max_dim=2, kind="one_point", seed=0, host=True, tie=True),   # every sum is 0
    "nan_vertex_2x70_k3": dict(B=2, V=70, n=3, k=3, max_dim=2, kind="nan", seed=14, host=True, tie=True),
    "max_dim_1_2x100_k3": dict(B=2, V=100, n=3, k=3, max_dim=1, kind="normal", seed=15, host=True),
    "exact_capacity_2x66_k3": dict(B=2, V=66, n=3, k=3, max_dim=2, kind="normal", seed=16, mode="exact", host=True),
    "relift_96_a": dict(B=2, V=96, n=3, k=3, max_dim=2, kind="normal", seed=17, host=False),
    "relift_96_b": dict(B=2, V=96, n=3, k=3, max_dim=2, kind="normal", seed=18, host=False),
    "relift_96_c": dict(B=2, V=96, n=3, k=3, max_dim=2, kind="normal", seed=19, host=False),
    "grid_4096_k8": dict(B=1, V=4096, n=2, k=8, max_dim=2, kind="grid", seed=20, host=False, tie=True),
}
SMALL = {f"tiny_12_k{k}": dict(B=2, V=12, n=3, k=k, max_dim=2, kind="normal", seed=21, host=True) for k in (1, 3, 8, 11)}
SMALL["tiny_33_k32"] = dict(B=1, V=33, n=3, k=32, max_dim=2, kind="normal", seed=22, host=True)
CASES.update(SMALL)


def make_points(c, seed):
    B, V, n, kind = c["B"], c["V"], c["n"], c["kind"]
    rng = np.random.default_rng(seed)
    pts = rng.standard_normal((B * V, n))
    if kind == "sixteenths":
        pts = rng.integers(0, 160, (B * V, n)) / 16.0
    elif kind == "boundary":
        # 64 names 63 and 63 names 10, which names it back: the edge (63, 64) exists in one direction only, across the words
        # 0 | 1; likewise 127 names 128 and 128 names 20, across 1 | 2 in the other direction
        pts[63], pts[10], pts[64] = (100.0, 0.0), (100.1, 0.0), (99.5, 0.0)
        pts[128], pts[20], pts[127] = (200.0, 0.0), (200.1, 0.0), (199.5, 0.0)
    elif kind == "outliers":                                 # vertices 0 and V - 1 far out: they name, nobody names them back
        p = pts.reshape(B, V, n)
        p[:, 0, 0] += 50.0
        p[:, V - 1, 0] -= 50.0
    elif kind == "lattice":
        pts = np.stack(np.meshgrid(np.arange(9.0), np.arange(8.0), indexing="ij"), axis=-1).reshape(V, 2)[rng.permutation(V)]
    elif kind == "coincident":
        pts[[64, 65, 69]] = pts[3]                           # four points at distance 0, over two words
        pts[20] = pts[10]
    elif kind == "one_point":
        pts[:] = (0.5, -1.25, 2.0)
    elif kind == "nan":
        pts[65] = np.nan                                     # graph 0, a vertex of word 1
        pts[V + 3, 1] = np.nan                               # graph 1, one coordinate
    elif kind == "grid":
        pts = CL._make_points(dict(c, kind="grid"), seed).astype(np.float64)
    else:
        assert kind == "normal", kind
    return np.ascontiguousarray(pts.astype(np.float32))


def pair_sums(p64):
    """csmpn.data.complexes._pair_sums of one graph: float64, j ascending, one rounding per operation, NaN -> +infinity."""
    from csmpn.data import complexes as cx
    return cx._pair_sums(p64)


def _sorted_rows(p64):
    """For one graph: others[a] = the V - 1 vertices but a in the order of (s(a, .), index), and their sums."""
    s = pair_sums(p64)
    V = len(s)
    others = np.arange(V - 1)[None, :] + (np.arange(V - 1)[None, :] >= np.arange(V)[:, None])
    so = np.take_along_axis(s, others, axis=1)
    order = np.argsort(so, axis=1, kind="stable")            # ties: the smaller index first
    return np.take_along_axis(others, order, axis=1), np.take_along_axis(so, order, axis=1)


def conditioning_ok(points32, B, k, tie=False):
    """The margin of a case between the k-th and the (k + 1)-th sum of every vertex; a tie case has none to keep (host and
    device take the same float64 sums: equal sums are equal on both sides)."""
    if tie:
        return True
    p = np.asarray(points32).astype(np.float64).reshape(B, -1, points32.shape[-1])
    if k >= p.shape[1] - 1:
        return True
    for g in range(B):
        so = _sorted_rows(p[g])[1]
        if not np.all(so[:, k] - so[:, k - 1] >= MARGIN * so[:, k]):
            return False
    return True


_POINTS = {}


def points_of(name):
    """The float32 points [B * V, n] of a case, its conditioning asserted; a seed that misses the margin is replaced by
    seed + 1000, + 2000, ... as cloud_lift_helpers.points_of does."""
    if name not in _POINTS:
        c = CASES[name]
        for seed in range(c["seed"], c["seed"] + 10000, 1000):
            pts = make_points(c, seed)
            if conditioning_ok(pts, c["B"], c["k"], c.get("tie", False)):
                break
        else:
            raise AssertionError(f"{name}: no seed keeps the margin")
        _POINTS[name] = pts
    return _POINTS[name]


# ------------------------------------------------------------------------------------------------ the fast restatement

def directed_neighbours(p64, k):
    """named[a, b] = b is one of the k nearest neighbours of a (one graph): the first k of the stable order on (s, index)."""
    idx = _sorted_rows(p64)[0]
    V = len(idx)
    named = np.zeros((V, V), dtype=bool)
    named[np.arange(V)[:, None], idx[:, :min(int(k), V - 1)]] = True
    return named


def knn_adjacency(p64, k):
    named = directed_neighbours(p64, k)
    return named | named.T


def fast_structure(points32, B, k, max_dim, capacity=None):
    """The structure tensors and counts of pad_batch(collate([knn_clique_complex(points_g, k, max_dim)]), capacity) - of the
    collated batch itself for capacity = None - as CPU int64 tensors; ValueError where pad_batch raises one.
    cloud_lift_helpers.fast_structure orders rows and adjacencies (vertex_block=False) from the matrix `pair sums <= dis^2`;
    for the length of the call its pair sums are 0 on the pairs of the kNN graph and 1 elsewhere, and dis^2 is 1 / 4."""
    graph_sums = lambda p: np.where(knn_adjacency(p[0], k), 0.0, 1.0)[None]
    kept = CL.pair_sums
    CL.pair_sums = graph_sums
    try:
        return CL.fast_structure(points32, B, 0.5, max_dim, False, capacity)
    finally:
        CL.pair_sums = kept


_REFERENCES = {}


def reference(name):
    """(points float32, k, max_dim, capacity, {structure tensor name: CPU tensor} + counts) of a case by the fast
    restatement; computed once and shared - callers must not change it."""
    if name not in _REFERENCES:
        c = CASES[name]
        pts = points_of(name)
        raw = fast_structure(pts, c["B"], c["k"], c["max_dim"])          # once: the sort of a 4096-vertex graph takes seconds
        cap = CL.capacity_for(raw["counts"].tolist(), c["max_dim"], c.get("mode", "spare"))
        arrays = {key: raw[key].numpy() for key in ("x_ind", "node_types", "batch", "ptr", "edge_index", "edge_types")}
        arrays["counts"] = raw["counts"].tolist()
        _REFERENCES[name] = (pts, c["k"], c["max_dim"], cap, CL._as_tensors(CL._padded(arrays, cap)))
    return _REFERENCES[name]


def host_complexes(name):
    from csmpn.data import complexes as cx
    c = CASES[name]
    p = points_of(name).astype(np.float64).reshape(c["B"], c["V"], c["n"])
    return [cx.knn_clique_complex(p[g], c["k"], c["max_dim"]) for g in range(c["B"])]


def host_structure(name, capacity):
    """pad_batch(collate([knn_clique_complex(...)]), capacity) of a case: the structure tensors and the counts."""
    from csmpn.data import complexes as cx
    raw = cx.collate(host_complexes(name))
    padded = cx.pad_batch(raw, capacity)
    want = {key: getattr(padded, key) for key in STRUCTURE}
    want["counts"] = torch.tensor(R.counts_of(raw, CASES[name]["max_dim"]), dtype=torch.int64)
    return want


# ------------------------------------------------------------------------- the two new kernels, word by word on the host

_INF_BITS, _ALL = 0x7FF0000000000000, (1 << 64) - 1


def _popc(x):
    return bin(x).count("1")


def selected_words(bits_row, a, V, k):
    """dir[a][0 .. W) as cloud_knn_select_kernel forms it from the row of s(a, .) as 64-bit integers (bits_row[b]; entry a is
    never read; the kernel's row length kWords >= W adds only words of ~0): the bisection two bits a pass, ended early by a candidate with exactly k sums below it, then the words of
    `s < T` and the first k - #{s < T} of `s == T`."""
    W = (V + 63) // 64
    # a lane at or past V, and the lane of a itself, holds ~0: above every candidate, equal to no T
    held = lambda w, i: int(bits_row[64 * w + i]) if 64 * w + i < V and 64 * w + i != a else _ALL
    ballot = lambda w, pred: sum(1 << i for i in range(64) if pred(held(w, i)))
    if k >= V - 1:
        return [ballot(w, lambda s: s != _ALL) for w in range(W)]
    T = less = 0
    for bit in range(62, -1, -2):
        cands = [T | (j << bit) for j in (1, 2, 3)]
        n = [sum(_popc(ballot(w, lambda s, c=c: s < c)) for w in range(W)) for c in cands]
        if k in n:                                           # exactly k sums below a candidate: no tie is left to take
            T, less = cands[n.index(k)], k
            break
        for c, m in reversed(list(zip(cands, n))):
            if m < k:
                T, less = c, m
                break
    assert less <= k and T <= _INF_BITS
    ties, words = k - less, []
    for w in range(W):
        eq = ballot(w, lambda s: s == T)
        take = sum(1 << i for i in range(64) if eq >> i & 1 and _popc(eq & ((1 << i) - 1)) < ties)
        words.append(ballot(w, lambda s: s < T) | take)
        ties -= min(ties, _popc(eq))
    assert ties == 0
    return words


def symmetric_words(dirs, a, V):
    """masks[a][0 .. W) as cloud_knn_mask_kernel forms it: dir[a][w] | the ballot over the lanes i of bit a of dir[64 w + i]."""
    W = (V + 63) // 64
    return [dirs[a][w] | sum(1 << i for i in range(64) if 64 * w + i < V and dirs[64 * w + i][a >> 6] >> (a & 63) & 1) for w in range(W)]


def kernel_masks(p64, k):
    """(dir, masks) of one graph, [V][W] Python ints, by the two restatements above."""
    s = pair_sums(p64)
    V = len(s)
    bits = s.view(np.uint64)
    dirs = [selected_words(bits[a], a, V, k) for a in range(V)]
    return dirs, [symmetric_words(dirs, a, V) for a in range(V)]


def words_of(matrix_row):
    """A boolean row [V] as ceil(V / 64) mask words."""
    V = len(matrix_row)
    return [sum(1 << i for i in range(64) if 64 * w + i < V and matrix_row[64 * w + i]) for w in range((V + 63) // 64)]


# ------------------------------------------------------------------------------------------------ md17-shaped data, V = 70

MD17_K, MD17_VERTS = 3, 70


def md17_cloud_case(seed):
    """knn_lift_helpers.md17_case for ONE graph of 70 vertices: (points float32 [70, 3], per-vertex features, the per-vertex
    target y, the collated host batch of the float64 copy of the points with those features in its vertex rows)."""
    from csmpn.data import complexes as cx
    c = dict(B=1, V=MD17_VERTS, n=3, kind="normal")
    for s in range(seed, seed + 10000, 1000):
        pts = make_points(c, s)
        if conditioning_ok(pts, 1, MD17_K):
            break
    rng = np.random.default_rng(1000 + seed)
    N, F = MD17_VERTS, R.MD17_FRAMES
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    vf = {"loc": f32(pts)[:, None, :] + 0.05 * f32(rng.standard_normal((N, F, 3))),
          "vel": 0.1 * f32(rng.standard_normal((N, F, 3))),
          "charges": f32(rng.integers(1, 9, size=(N, 1, 1))).expand(N, F, 1).contiguous()}
    y = vf["loc"] + 0.1 * f32(rng.standard_normal((N, F, 3)))
    comp = cx.knn_clique_complex(pts.astype(np.float64), MD17_K, 2)
    for key, v in vf.items():
        t = torch.zeros((comp.n_simplices,) + tuple(v.shape[1:]))
        t[:N] = v
        comp.features[key] = t
    b = cx.collate([comp])
    b.y = y
    b._names.append("y")
    return pts, vf, y, b


guarded, buffers, guards_intact, GUARD = KH.guarded, KH.buffers, KH.guards_intact, KH.GUARD
