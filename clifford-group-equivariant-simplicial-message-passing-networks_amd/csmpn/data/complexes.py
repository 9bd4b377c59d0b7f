"""Lifted-graph input format of the shared simplicial message-passing path, without
torch_geometric / gudhi.

The reference turns every simplicial complex into ONE "big graph" whose nodes are all simplices
(vertices first, then edges, then triangles) and whose `edge_index` is the union of the adjacency
types `adj_{s}_{t}` with per-dimension row offsets (csmpn/data/modules/simplicial_data.py:105-157),
then lets PyG collate graphs into a batch with `follow_batch=["node_types", "x_ind"]`
(csmpn/data/hulls.py:109-122). This module restates that format:

  lift(n_vertices, top_simplices, max_dim)   faces + the reference's adjacency rules
                                             (csmpn/data/modules/utils.py:63-103: boundaries,
                                             upper adjacencies through a shared coface, the
                                             fully connected 0-0 block with its duplicate
                                             directed edges, and the flipped k+1 -> k copies,
                                             simplicial_data.py:105-110)
  hull_complex(points) / rips_complex(...)   the two complex constructions the task data use
                                             (utils.py:210-247 convex hull faces; utils.py:106-137
                                             distance-thresholded cliques)
  knn_edges / knn_clique_complex(points, k)  the third one, md17's aspirin configuration: the 2- and
                                             3-cliques of the k-nearest-neighbour graph
                                             (csmpn/data/md17.py:64 knn_graph; utils.py:151-207
                                             simplicial_lift) with the adjacencies of
                                             utils.py:322-375 generate_adjacencies, which has NO
                                             fully connected 0-0 block: lift(..., vertex_block=False)
  clique_complex(points, edge_index,         the same lift of ANY edge list with the reference's finite
                 edge_th, tri_th)            thresholds (utils.py:183-200): edges longer than edge_th and
                                             triangles of area above tri_th are dropped, a kept triangle
                                             brings its pairs back
  collate(complexes)                        the batch the task models read: x_ind (vertex ids
                                             LOCAL to each graph, as in the reference: x_ind has no
                                             `__inc__`), node_types, edge_index (offset per graph),
                                             batch / ptr / x_ind_batch / x_ind_ptr

A batch caches the target-sorted CSR of its `edge_index` (complexes are static: built once in
`pre_transform`, hulls.py:68-78), so no layer or step rebuilds it.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch


@dataclass
class SimplicialComplex:
    n_vertices: int
    x_ind: torch.Tensor          # [S, max_dim + 1] int64: vertex ids of every simplex, zero padded
    node_types: torch.Tensor     # [S] int64: dimension of every simplex
    edge_index: torch.Tensor     # [2, E] int64 over the S simplices (row 0 = source, row 1 = target)
    edge_types: torch.Tensor     # [E, 2] int64: (source dimension, target dimension)
    features: Dict[str, torch.Tensor] = field(default_factory=dict)   # per-simplex tensors [S, ...]
    labels: Dict[str, torch.Tensor] = field(default_factory=dict)     # per-graph tensors

    @property
    def n_simplices(self) -> int:
        return int(self.x_ind.shape[0])


def lift(n_vertices: int, top_simplices: Sequence[Sequence[int]], max_dim: int = 2, vertex_block: bool = True):
    """All faces up to `max_dim` of the given simplices and the reference's adjacencies. vertex_block=False leaves out the
    fully connected 0-0 block over the non-edges (the clique lift of a graph, utils.py:322-375, has none).

    Returns (x_dict, adj): x_dict[d] = int64 [n_d, d+1] (sorted vertex tuples, lexicographic order),
    adj["s_t"] = int64 [2, n] (source index in dimension s, target index in dimension t)."""
    faces: List[set] = [set((v,) for v in range(n_vertices))] + [set() for _ in range(max_dim)]
    for simplex in top_simplices:
        verts = tuple(sorted(int(v) for v in simplex))
        for k in range(1, max_dim + 1):
            for sub in itertools.combinations(verts, k + 1):
                faces[k].add(sub)
    ordered = [sorted(f) for f in faces]
    index = [{s: i for i, s in enumerate(f)} for f in ordered]
    adj: Dict[str, List] = {}

    def add(key, src, dst):
        adj.setdefault(key, []).append((src, dst))

    for k in range(max_dim + 1):
        for s in ordered[k]:
            si = index[k][s]
            # upper adjacency: the other boundaries of every coface of s (utils.py:72-83)
            if k + 1 <= max_dim:
                sset = set(s)
                for c in ordered[k + 1]:
                    if sset.issubset(c):
                        for b in itertools.combinations(c, k + 1):
                            if b != s:
                                add(f"{k}_{k}", index[k][b], si)
            # boundaries (utils.py:86-89)
            if k >= 1:
                for b in itertools.combinations(s, k):
                    add(f"{k - 1}_{k}", index[k - 1][b], si)
    # fully connected 0-0 block over the non-edges; the test `[i, j] not in edges_present` compares with
    # SORTED vertex lists, so (i, j) with i > j is added even when {i, j} is an edge (utils.py:91-97)
    if max_dim >= 1 and vertex_block:
        present = set(ordered[1])
        for i in range(n_vertices):
            for j in range(n_vertices):
                if i != j and (i, j) not in present:
                    add("0_0", i, j)
    out = {k: torch.tensor(v, dtype=torch.int64).t().contiguous() for k, v in adj.items()}
    # downward communication: the flipped copies (simplicial_data.py:105-110)
    for k in range(max_dim):
        if f"{k}_{k + 1}" in out:
            out[f"{k + 1}_{k}"] = out[f"{k}_{k + 1}"][[1, 0]].clone()
    x_dict = {k: torch.tensor(ordered[k], dtype=torch.int64).reshape(-1, k + 1) for k in range(max_dim + 1)}
    return x_dict, out


def to_complex(n_vertices: int, x_dict, adj, max_dim: int = 2) -> SimplicialComplex:
    """The big graph of one complex (simplicial_data.py:112-157): simplices of all dimensions are the
    rows, adjacency types are concatenated in (source dimension, target dimension) order."""
    counts = [int(x_dict[d].shape[0]) if d in x_dict else 0 for d in range(max_dim + 1)]
    offs = np.concatenate([[0], np.cumsum(counts)])
    S = int(offs[-1])
    x_ind = torch.zeros(S, max_dim + 1, dtype=torch.int64)
    node_types = torch.zeros(S, dtype=torch.int64)
    for d in range(max_dim + 1):
        x_ind[offs[d]:offs[d + 1], :d + 1] = x_dict[d]
        node_types[offs[d]:offs[d + 1]] = d
    ei, et = [], []
    for s in range(max_dim + 1):
        for t in range(max_dim + 1):
            a = adj.get(f"{s}_{t}")
            if a is None or a.numel() == 0:
                continue
            e = a.clone()
            e[0] += int(offs[s])
            e[1] += int(offs[t])
            ei.append(e)
            et.append(torch.tensor([[s, t]], dtype=torch.int64).expand(a.shape[1], 2))
    edge_index = torch.cat(ei, dim=1) if ei else torch.zeros(2, 0, dtype=torch.int64)
    edge_types = torch.cat(et, dim=0) if et else torch.zeros(0, 2, dtype=torch.int64)
    return SimplicialComplex(n_vertices, x_ind, node_types, edge_index, edge_types)


def _hull_det(M, row: int, cols):
    """Determinant of the rows row .. of M and the columns `cols` (as many as rows), M[i][j] float64 arrays: the Laplace
    expansion along the first row over the columns ascending, ((M[c0] d0 - M[c1] d1) + M[c2] d2) - ..., every product
    rounded before it is added - the expression minor_det / laplace of csrc/lift.hip state."""
    if len(cols) == 1:
        return M[row][cols[0]]
    acc = None
    for k, c in enumerate(cols):
        term = M[row][c] * _hull_det(M, row + 1, [x for x in cols if x != c])
        acc = term if k == 0 else (acc - term if k & 1 else acc + term)
    return acc


HULL_LANES = 256       # the candidates rank, rank + 256, ... are summed by one thread of lift_hull_kernel


def hull_facets(points: np.ndarray) -> Tuple[np.ndarray, float]:
    """(facets int64 [F, n] in lexicographic order, volume) of the convex hull of `points` [V, n], V > n >= 2, by the rule
    csmpn_hull_lift applies on the device, in float64 with the very order of operations of lift_hull_kernel, so that both
    give the same facets and the same volume to the bit.

    A candidate is an n-subset F = (f_0 < ... < f_{n-1}). With the rows M_i = p_{f_{i+1}} - p_{f_0}, its normal is
    N_j = (-1)^(n-1+j) det(M without column j) (_hull_det) and side(F, q) = sum_j N_j (q_j - p_{f_0, j}), j ascending. F is a
    facet iff side(F, q) > 0 for every vertex q outside F, or < 0 for every one; a zero or a NaN makes F no facet. Coplanar
    point sets, coincident points and NaN vertices therefore give fewer facets, or none: what qhull does with degenerate
    input (merged or joggled facets) is not restated. On points in general position this is the facet set of the hull,
    whatever the implementation.

    volume = (sum over the facets of |side(F, p_0)|) / n!: vertex 0 lies in or on the hull, so every term is n! times the
    volume of the simplex over a facet with apex p_0 (0 for the facets through p_0). Order of the sum: the candidates
    rank, rank + 256, ... (rank = the lexicographic index) ascending into one of 256 partial sums; each run of 64 of those
    halved by adding the upper half onto the lower (32, 16, ..., 1); the four results added left to right."""
    pts = np.asarray(points, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] < 2 or pts.shape[0] <= pts.shape[1]:
        raise ValueError(f"hull_facets: points must be [V, n] with V > n >= 2, got {tuple(pts.shape)}")
    V, n = pts.shape
    cand = np.array(list(itertools.combinations(range(V), n)), dtype=np.int64).reshape(-1, n)
    origin = pts[cand[:, 0]]
    with np.errstate(invalid="ignore", over="ignore"):
        M = [[pts[cand[:, i + 1], j] - origin[:, j] for j in range(n)] for i in range(n - 1)]
        normal = []
        for j in range(n):
            d = _hull_det(M, 0, [c for c in range(n) if c != j])
            normal.append(-d if (n - 1 + j) & 1 else d)

        def side(q):
            s = normal[0] * (q[0] - origin[:, 0])
            for j in range(1, n):
                s = s + normal[j] * (q[j] - origin[:, j])
            return s

        pos, neg = np.ones(len(cand), dtype=bool), np.ones(len(cand), dtype=bool)
        for q in range(V):
            s, inside = side(pts[q]), (cand == q).any(axis=1)
            pos &= inside | (s > 0)
            neg &= inside | (s < 0)
        facet = pos | neg
        terms = np.where(facet, np.abs(side(pts[0])), 0.0)
        terms = np.concatenate([terms, np.zeros(-len(terms) % HULL_LANES)]).reshape(-1, HULL_LANES)
        partial = np.zeros(HULL_LANES)
        for row in terms:
            partial = partial + row
        x = partial.reshape(-1, 64)
        for d in (32, 16, 8, 4, 2, 1):
            x = x[:, :d] + x[:, d:2 * d]
        total = x[0, 0]
        for w in range(1, x.shape[0]):
            total = total + x[w, 0]
    return cand[facet], float(total / math.factorial(n))


def hull_complex(points: np.ndarray, max_dim: int = 2, method: str = "qhull") -> SimplicialComplex:
    """Faces of the convex hull of `points` [V, n] (utils.py:210-247). method="qhull": the facets scipy's qhull reports (the
    reference's); method="exact": those of hull_facets - the same set on points in general position, the rule of the device
    lift (csmpn_hull_lift) on every input."""
    if method == "qhull":
        from scipy.spatial import ConvexHull
        facets = ConvexHull(np.asarray(points, dtype=np.float64)).simplices.tolist()
    elif method == "exact":
        facets = hull_facets(points)[0].tolist()
    else:
        raise ValueError(f"hull_complex: method {method!r} (\"qhull\" or \"exact\")")
    x_dict, adj = lift(len(points), facets, max_dim)
    return to_complex(len(points), x_dict, adj, max_dim)


def rips_complex(points: np.ndarray, dis: float, max_dim: int = 2, vertex_block: bool = True) -> SimplicialComplex:
    """Vietoris-Rips complex: an edge for every pair closer than `dis`, higher simplices = cliques
    (utils.py:106-137). vertex_block=False: without the fully connected 0-0 block over the non-edges (lift), the
    adjacencies of clique_complex - V (V - 1) - n1 entries that a cloud of thousands of points does not want."""
    pts = np.asarray(points, dtype=np.float64)
    V = len(pts)
    close = np.linalg.norm(pts[:, None] - pts[None], axis=-1) <= dis
    tops = []
    for k in range(1, max_dim + 1):
        for sub in itertools.combinations(range(V), k + 1):
            if all(close[a, b] for a, b in itertools.combinations(sub, 2)):
                tops.append(sub)
    x_dict, adj = lift(V, tops, max_dim, vertex_block=vertex_block)
    return to_complex(V, x_dict, adj, max_dim)


def _pair_sums(points: np.ndarray) -> np.ndarray:
    """s[a, b] = sum_j (p_a[j] - p_b[j])^2 in float64, j ascending, one rounding per product and per sum (what
    csrc/lift.hip takes); a NaN sum counts as +infinity."""
    pts = np.asarray(points, dtype=np.float64)
    s = np.zeros((len(pts), len(pts)), dtype=np.float64)
    for j in range(pts.shape[1]):
        d = pts[:, None, j] - pts[None, :, j]
        s = s + d * d
    s[np.isnan(s)] = np.inf
    return s


def knn_edges(points: np.ndarray, k: int) -> torch.Tensor:
    """The directed k-nearest-neighbour list of `points` [V, n] as int64 [2, E] (row 0 = the neighbour, row 1 = the vertex:
    the source_to_target flow of knn_graph), targets ascending, the neighbours of a target ascending.

    With s(a, b) the float64 sum of _pair_sums, the rank of b for a is the number of c outside {a, b} with s(a, c) < s(a, b),
    or s(a, c) == s(a, b) and c < b; b is a neighbour of a iff that rank is below k. Ties - coincident points and NaN
    vertices among them - go to the smaller index; k >= V - 1 makes every other vertex a neighbour. On points with pairwise
    distinct distances this is THE k-nearest-neighbour graph, whatever the implementation; how torch_cluster.knn_graph
    breaks ties is a detail of its search and is not restated here."""
    if int(k) < 1:
        raise ValueError("knn_edges: k must be at least 1")
    s = _pair_sums(points)
    V = len(s)
    src, dst = [], []
    for a in range(V):
        others = [b for b in range(V) if b != a]
        others.sort(key=lambda b: (s[a, b], b))
        for b in sorted(others[:int(k)]):
            src.append(b)
            dst.append(a)
    return torch.tensor([src, dst], dtype=torch.int64).reshape(2, -1)


def knn_clique_complex(points: np.ndarray, k: int, max_dim: int = 2) -> SimplicialComplex:
    """The clique complex of the undirected k-nearest-neighbour graph of `points` (knn_edges: {a, b} is an edge iff b is a
    neighbour of a or a one of b - what nx.Graph makes of the directed list): the vertices, the edges and, for max_dim = 2,
    every triple whose three pairs are edges (utils.py:151-207), with the adjacencies of lift(..., vertex_block=False).
    The tie rule is knn_edges' own; see there what is and is not claimed about torch_cluster."""
    ei = knn_edges(points, k)
    V = len(np.asarray(points))
    adj = np.zeros((V, V), dtype=bool)
    adj[ei[0].numpy(), ei[1].numpy()] = True
    adj |= adj.T
    tops = []
    for d in range(1, max_dim + 1):
        for sub in itertools.combinations(range(V), d + 1):
            if all(adj[a, b] for a, b in itertools.combinations(sub, 2)):
                tops.append(sub)
    x_dict, adjs = lift(V, tops, max_dim, vertex_block=False)
    return to_complex(V, x_dict, adjs, max_dim)


def _gram_dets(points: np.ndarray, triples: np.ndarray) -> np.ndarray:
    """g = uu vv - uv uv of every triple (a, b, c) [T, 3] in float64: u = p_b - p_a, v = p_c - p_a, uu / vv / uv summed over j
    ascending, one rounding per difference, product and sum (what csrc/lift.hip takes); 4 area^2 of the triangle, in any
    dimension. A NaN counts as +infinity."""
    pts = np.asarray(points, dtype=np.float64)
    t = np.asarray(triples, dtype=np.int64).reshape(-1, 3)
    uu, vv, uv = np.zeros(len(t)), np.zeros(len(t)), np.zeros(len(t))
    for j in range(pts.shape[1]):
        u = pts[t[:, 1], j] - pts[t[:, 0], j]
        v = pts[t[:, 2], j] - pts[t[:, 0], j]
        uu, vv, uv = uu + u * u, vv + v * v, uv + u * v
    g = uu * vv - uv * uv
    g[np.isnan(g)] = np.inf
    return g


def _thresholds_squared(what: str, edge_th: float, tri_th: float) -> Tuple[float, float]:
    """(edge_th^2, 4 tri_th^2) in float64 - what s and g are compared against; ValueError for a negative one or a NaN."""
    edge_th, tri_th = float(edge_th), float(tri_th)
    if not (edge_th >= 0.0 and tri_th >= 0.0):
        raise ValueError(f"{what}: edge_th and tri_th must be >= 0 or +infinity, got {edge_th} and {tri_th}")
    return edge_th * edge_th, 4.0 * tri_th * tri_th


def clique_complex(points: np.ndarray, edge_index, edge_th: float = math.inf, tri_th: float = math.inf,
                   max_dim: int = 2) -> SimplicialComplex:
    """The thresholded clique lift of ANY graph G on `points` [V, n] (utils.py:151-207 simplicial_lift with finite
    edge_th / tri_th). edge_index [2, E]: {a, b} is an edge of G iff (a, b) or (b, a) is listed; duplicates and both
    directions are harmless, self-loops are ignored.

      E_keep = the edges of G with s(a, b) <= edge_th^2 (s of _pair_sums);
      T_keep = the triples a < b < c whose three pairs are edges of G - not of E_keep - with g <= 4 tri_th^2 (g of _gram_dets:
               4 area^2, in R^3 the reference's |u x v|^2, and defined in R^2 as well);
      1-simplices = E_keep and the three pairs of every triple of T_keep (gudhi's insert of a triangle inserts its faces: a kept
               triangle brings back an edge that edge_th removed), 2-simplices = T_keep.

    The result is NOT a clique complex: three surviving edges need not bound a surviving triangle. Adjacencies: those of
    lift(..., vertex_block=False). With both thresholds +infinity every comparison holds (a NaN counts as +infinity) and the
    result on knn_edges(points, k) is knn_clique_complex(points, k)."""
    pts = np.asarray(points, dtype=np.float64)
    V = len(pts)
    ei = np.asarray(edge_index.cpu() if torch.is_tensor(edge_index) else edge_index, dtype=np.int64).reshape(2, -1)
    if ei.size and (int(ei.min()) < 0 or int(ei.max()) >= V):
        raise ValueError(f"clique_complex: edge_index names vertices outside 0..{V - 1}")
    edge_th2, tri_th4 = _thresholds_squared("clique_complex", edge_th, tri_th)
    adj = np.zeros((V, V), dtype=bool)
    adj[ei[0], ei[1]] = True
    adj |= adj.T
    np.fill_diagonal(adj, False)
    s = _pair_sums(pts)
    tops = [(a, b) for a in range(V) for b in range(a + 1, V) if adj[a, b] and s[a, b] <= edge_th2]
    triples = [(a, b, c) for a in range(V) for b in range(a + 1, V) if adj[a, b]
               for c in range(b + 1, V) if adj[a, c] and adj[b, c]]
    if triples:
        keep = _gram_dets(pts, np.asarray(triples)) <= tri_th4
        tops += [t for t, k in zip(triples, keep) if k]
    x_dict, adjs = lift(V, tops, max_dim, vertex_block=False)
    return to_complex(V, x_dict, adjs, max_dim)


class SimplicialBatch:
    """What the task models read from a collated batch (hulls.py:109-122 with
    follow_batch=["node_types", "x_ind"]). Per-simplex feature tensors and per-graph labels are
    attributes under their own names (`input`, `target`, `pos`, ...)."""

    def __init__(self, **tensors):
        self._names = list(tensors)
        for k, v in tensors.items():
            setattr(self, k, v)
        self._csr = None

    def to(self, device, dtype=None):
        """The batch on `device`; dtype: cast the floating feature tensors to it (the index tensors stay as they are)."""
        def move(t):
            return t.to(device, dtype=dtype) if (dtype is not None and t.is_floating_point()) else t.to(device)
        out = SimplicialBatch(**{k: move(getattr(self, k)) for k in self._names})
        for k in ("n_real_rows", "n_real_edges"):      # set by pad_batch
            if hasattr(self, k):
                setattr(out, k, getattr(self, k))
        return out

    @property
    def num_graphs(self) -> int:
        return int(self.ptr.shape[0]) - 1

    def plan(self, max_dim: int = 2):
        """Index tables of the embedding stage, computed once per batch (the only host round trips of
        a model step: everything downstream uses fixed-shape index_select / index_copy and can be
        captured in a HIP graph):
          rows[d]   rows of the d-simplices                                    [n_d]
          verts[d]  their vertices in all (d+1)! orders, as batch rows          [n_d * (d+1)!, d+1]
          vertex_rows = rows[0]; graph_of_vertex = graph id of every vertex row."""
        cached = getattr(self, "_plan", None)
        if cached is not None and cached["max_dim"] == max_dim:
            return cached
        import itertools
        start = self.x_ind_ptr[:-1][self.x_ind_batch]
        vrows = self.x_ind.long() + start.unsqueeze(-1)
        plan = {"max_dim": max_dim, "rows": [], "verts": [], "nperm": []}
        for d in range(max_dim + 1):
            rows = torch.nonzero(self.node_types == d, as_tuple=False).flatten()
            perms = torch.tensor(list(itertools.permutations(range(d + 1))), device=rows.device)
            plan["rows"].append(rows)
            vt = vrows[rows][:, : d + 1]
            # once per batch: the fused embedding kernels (csmpn_embed_cemlp_*) index the vertex features with these rows
            # UNCHECKED (include/csmpn_hip.h states the precondition) and the composed path's gather clamps silently -
            # check here, where PyTorch indexing would have asserted
            if vt.numel() and (int(vt.min()) < 0 or int(vt.max()) >= int(self.node_types.shape[0])):
                raise IndexError(f"x_ind of the {d}-simplices points outside the batch ({int(vt.min())}..{int(vt.max())} "
                                 f"of {int(self.node_types.shape[0])} rows)")
            plan["verts"].append(vt[:, perms].reshape(-1, d + 1).contiguous())
            plan["nperm"].append(int(perms.shape[0]))
        plan["vertex_rows"] = plan["rows"][0]
        plan["graph_of_vertex"] = self.batch[plan["rows"][0]]
        plan["vertices_per_graph"] = torch.bincount(plan["graph_of_vertex"], minlength=self.num_graphs)
        self._plan = plan
        return plan

    def lazy_table(self, plan, key, build):
        """plan[key], built on first use by build(None). The builder is kept: refresh_() calls build(plan[key]) to refill
        the table IN PLACE for a batch of new topology - fixed-shape device ops only; the host-side checks of a table run
        on its first build."""
        if key not in plan:
            plan[key] = build(None)
            plan.setdefault("builders", {})[key] = build
        return plan[key]

    def refresh_(self, raw: "SimplicialBatch") -> "SimplicialBatch":
        """Make this DEVICE batch hold `raw` - a batch of exactly the same shapes, i.e. padded to the same capacity
        (pad_batch), on the CPU or the device - without changing the address of anything: the tensors are copied into this
        batch's, and every table derived from the topology is rebuilt in place on the current stream with no allocation
        (after the first call) and no host round trip: the tables of plan() (csmpn_simplex_tables), the target-sorted CSR
        (ops.Csr.rebuild_) and whatever the models have added to the plan (lazy_table). A training step captured over this
        batch (csmpn_hip.graphed.GraphedTrainStep) can then be replayed on the new batch. plan() and csr() must have been
        called. Nothing is validated here: pad_batch has checked the indices on the host; a batch whose row counts per
        dimension differ from this one's sets bits in plan()["status"] (ops.simplex_tables) instead of writing out of
        bounds."""
        plan = getattr(self, "_plan", None)
        if plan is None or self._csr is None:
            raise RuntimeError("refresh_: call plan() and csr() on the batch first")
        if sorted(raw._names) != sorted(self._names):
            raise ValueError(f"refresh_: the batches hold different tensors ({sorted(set(raw._names) ^ set(self._names))})")
        for k in self._names:
            if tuple(getattr(raw, k).shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"refresh_: {k} has shape {tuple(getattr(raw, k).shape)}, this batch "
                                 f"{tuple(getattr(self, k).shape)} (pad both to one BatchCapacity)")
        for k in self._names:
            getattr(self, k).copy_(getattr(raw, k), non_blocking=True)
        for k in ("n_real_rows", "n_real_edges"):
            if hasattr(raw, k):
                setattr(self, k, getattr(raw, k))
        return self._rebuild_in_place()

    def _rebuild_in_place(self) -> "SimplicialBatch":
        """Everything derived from the structure tensors, rebuilt in place on the current stream (refresh_, relift_)."""
        from csmpn_hip import ops
        plan = self._plan
        dev = self.x_ind.device
        if "tables_ws" not in plan:
            plan["tables_ws"] = ops.simplex_tables_workspace(self.node_types.shape[0], plan["max_dim"], dev)
            plan["status"] = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.simplex_tables(self.x_ind, self.node_types, self.x_ind_batch, self.x_ind_ptr, plan["max_dim"], plan["rows"],
                           plan["verts"], plan.get("verts_i32"), plan["graph_of_vertex"], plan["vertices_per_graph"],
                           plan.get("types_i32"), plan["status"], plan["tables_ws"])
        self._csr.rebuild_(self.edge_index)
        for key, build in plan.get("builders", {}).items():
            if key not in ("verts_i32", "types_i32"):      # those two are outputs of csmpn_simplex_tables
                build(plan[key])
        return self

    def relift_(self, points: torch.Tensor, dis: Optional[float] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                knn: Optional[int] = None, hull: bool = False, edges: Optional[torch.Tensor] = None,
                edge_th: Optional[float] = None, tri_th: Optional[float] = None) -> "SimplicialBatch":
        """Make this DEVICE batch hold the Vietoris-Rips complexes of `points` (device float32 [B * V, n], the V vertices of
        graph g contiguous; B and V are this batch's) at threshold `dis`, at the capacity the batch was built with: the
        structure tensors are written by ops.rips_lift (csmpn_rips_lift) as pad_batch(collate([rips_complex(...)]), capacity)
        would lay them out, then everything derived from them is rebuilt in place as in refresh_. With knn=k instead of
        dis (exactly one of the two, else ValueError) the complexes are the clique complexes of the k-nearest-neighbour
        graphs, knn_clique_complex(points, k), written by ops.knn_lift (csmpn_knn_lift); with hull=True (exactly one of the
        three) the convex-hull complexes hull_complex(points, method="exact"), written by ops.hull_lift (csmpn_hull_lift), which
        also writes the hulls' volumes into `target` where the batch has one, and - as hull_batch_device does - the points
        count as the vertex feature `input` where the batch has that tensor and vertex_features does not name it. vertex_features
        {name: per-vertex tensor [B * V, ...]}: the per-simplex tensor `name` is zeroed and gets these rows at the vertex
        rows of the new batch. plan() and csr() must have been called. After the first call: no allocation, no host
        synchronisation. A complex that does not fit the capacity leaves the batch as it was (the features excepted, which
        land on the old vertex rows) and sets bits in plan()["lift_status"] (ops.rips_lift). The host-side n_real_rows /
        n_real_edges are dropped: the real counts live on the device, in plan()["lift_counts"] (rows per dimension,
        adjacencies).

        edges=... (a device int64 [2, n] list of GLOBAL vertex ids g V + a; (-1, -1) entries are padding) is the fourth choice
        under the same rule: the thresholded clique complexes clique_complex(points, edges of the graph, edge_th, tri_th) of
        the listed graph, written by ops.clique_lift (csmpn_clique_lift). edge_th / tri_th (default +infinity each) go with
        edges=... or knn=...: knn=k with a threshold lifts clique_complex(points, knn_edges(points, k), edge_th, tri_th) through
        the same entry; knn=k without one is csmpn_knn_lift as before. A threshold with dis or hull is a ValueError. A list
        with an end outside the batch or across two graphs leaves the batch as it was and sets bit 5 of plan()["lift_status"].

        A batch of cloud_batch_device (up to 4096 vertices per graph) takes dis=... alone: it is re-lifted by ops.cloud_lift
        (csmpn_cloud_lift) with the vertex_block it was built with and its own workspace; knn, hull, edges and the thresholds
        are a ValueError there - those lifts hold at most 64 vertices per graph. A batch of knn_cloud_batch_device takes
        knn=k alone: it is re-lifted by ops.cloud_knn_lift (csmpn_cloud_knn_lift) with its own workspace; dis, hull, edges and
        the thresholds are a ValueError there."""
        from csmpn_hip import ops
        if (dis is not None) + (knn is not None) + bool(hull) + (edges is not None) != 1:
            raise ValueError("relift_: pass exactly one of dis=... (Rips), knn=... (k-nearest-neighbour cliques), hull=True "
                             "(convex hulls) and edges=... (the thresholded cliques of a listed graph)")
        thresholded = edge_th is not None or tri_th is not None
        plan = getattr(self, "_plan", None)
        cloud = None if plan is None else plan.get("cloud")
        if cloud is not None and (dis is None or thresholded):
            raise ValueError("relift_: a cloud batch (cloud_batch_device) is re-lifted with dis=... alone - the kNN, hull and "
                             "thresholded clique lifts (knn, hull, edges, edge_th, tri_th) hold at most 64 vertices per graph")
        cloud_knn = plan is not None and plan.get("cloud_knn") is not None
        if cloud_knn and (knn is None or thresholded):
            raise ValueError("relift_: a kNN cloud batch (knn_cloud_batch_device) is re-lifted with knn=... alone - its workspace "
                             "serves csmpn_cloud_knn_lift; dis, hull, edges, edge_th and tri_th go with the other batches")
        if thresholded and (dis is not None or hull):
            raise ValueError("relift_: edge_th / tri_th go with edges=... or knn=..., not with dis or hull")
        if plan is None or self._csr is None:
            raise RuntimeError("relift_: call plan() and csr() on the batch first")
        dev = self.x_ind.device
        if dev.type != "cuda" or points.device != dev:
            raise RuntimeError("relift_: the batch and the points must live on one GPU (no CPU fallback)")
        max_dim, B = plan["max_dim"], self.num_graphs
        rows = [int(r.shape[0]) for r in plan["rows"]]
        if points.dim() != 2 or int(points.shape[0]) != rows[0]:
            raise ValueError(f"relift_: points must be [{rows[0]}, n] (one row per vertex of the batch), got {tuple(points.shape)}")
        if hull and "input" in self._names and "input" not in (vertex_features or {}):
            vertex_features = dict(vertex_features or {}, input=points)
        for name, value in (vertex_features or {}).items():
            t = getattr(self, name, None)
            if name not in self._names or name in _STRUCTURE or int(t.shape[0]) != int(self.node_types.shape[0]):
                raise ValueError(f"relift_: {name!r} is not a per-simplex feature tensor of the batch")
            if tuple(value.shape) != (rows[0],) + tuple(t.shape[1:]):
                raise ValueError(f"relift_: vertex feature {name!r} has shape {tuple(value.shape)}, expected {(rows[0],) + tuple(t.shape[1:])}")
        if "lift_ws" not in plan:
            plan["lift_ws"] = _lift_workspace(B, rows[0] // B, max_dim, dev)
            plan["lift_status"] = torch.zeros(1, dtype=torch.int32, device=dev)
            plan["lift_counts"] = torch.zeros(max_dim + 2, dtype=torch.int64, device=dev)
        if cloud is not None:
            run = lambda *args: ops.cloud_lift(*args, vertex_block=cloud["vertex_block"])
        elif cloud_knn:
            run = ops.cloud_knn_lift
        elif edges is not None or thresholded:
            if "clique_lift_ws" not in plan:
                plan["clique_lift_ws"] = ops.clique_lift_workspace(B, rows[0] // B, max_dim, dev)
            ths = dict(edge_th=math.inf if edge_th is None else edge_th, tri_th=math.inf if tri_th is None else tri_th)
            run = lambda p, b, _, *rest: ops.clique_lift(p, b, knn if edges is None else edges, *rest[:-1], plan["clique_lift_ws"], **ths)
        elif hull:
            target = getattr(self, "target", None) if "target" in self._names else None
            run = lambda p, b, _, *rest: ops.hull_lift(p, b, *rest, volume=target)
        else:
            run = ops.rips_lift if knn is None else ops.knn_lift
        run(points, B, dis if knn is None else knn, max_dim, rows, int(self.edge_index.shape[1]), self.x_ind, self.node_types,
            self.batch, self.x_ind_batch, self.ptr, self.x_ind_ptr, self.edge_index, getattr(self, "edge_types", None),
            plan["lift_counts"], plan["lift_status"], plan["lift_ws"])
        for k in ("n_real_rows", "n_real_edges"):
            if hasattr(self, k):
                delattr(self, k)
        self._rebuild_in_place()
        for name, value in (vertex_features or {}).items():
            t = getattr(self, name)
            t.zero_()
            t.index_copy_(0, plan["vertex_rows"], value.to(t.dtype))
        return self

    def csr(self):
        """Target-sorted adjacency of the batch, built once (device batches only)."""
        if self._csr is None:
            from csmpn_hip import ops
            self._csr = ops.Csr(self.edge_index, int(self.node_types.shape[0]))
            try:   # the layers look the CSR up on the tensor object (ops.get_csr)
                self.edge_index._csmpn_csr = (self.edge_index._version, self._csr)
            except Exception:
                pass
        return self._csr


def collate(complexes: Sequence[SimplicialComplex]) -> SimplicialBatch:
    sizes = [c.n_simplices for c in complexes]
    ptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64)
    batch = torch.repeat_interleave(torch.arange(len(complexes)), torch.tensor(sizes))
    out = dict(
        x_ind=torch.cat([c.x_ind for c in complexes], dim=0),
        node_types=torch.cat([c.node_types for c in complexes], dim=0),
        edge_index=torch.cat([c.edge_index + int(ptr[i]) for i, c in enumerate(complexes)], dim=1),
        edge_types=torch.cat([c.edge_types for c in complexes], dim=0),
        batch=batch, ptr=ptr, x_ind_batch=batch.clone(), x_ind_ptr=ptr.clone(),
    )
    for name in complexes[0].features:
        out[name] = torch.cat([c.features[name] for c in complexes], dim=0)
    for name in complexes[0].labels:
        out[name] = torch.stack([c.labels[name] for c in complexes], dim=0)
    return SimplicialBatch(**out)


def hulls_example(points: np.ndarray, target: Optional[float] = None, max_dim: int = 2) -> SimplicialComplex:
    """One convex-hulls sample as the reference's transform lays it out (simplicial_data.py:177-196):
    `input` [S, n] holds the vertex coordinates in the vertex rows and zeros elsewhere."""
    c = hull_complex(points, max_dim)
    inp = torch.zeros(c.n_simplices, points.shape[1], dtype=torch.float32)
    inp[: c.n_vertices] = torch.as_tensor(points, dtype=torch.float32)
    c.features["input"] = inp
    if target is None:
        from scipy.spatial import ConvexHull
        target = float(ConvexHull(np.asarray(points, dtype=np.float64)).volume)
    c.labels["target"] = torch.tensor(target, dtype=torch.float32)
    return c


# ------------------------------------------------------------------------------- fixed-capacity batches
#
# A training step captured in a HIP graph (csmpn_hip.graphed.GraphedTrainStep) addresses every tensor of its batch, so it
# can be replayed only on batches of the same SHAPES. The batches of one dataset share their vertex count (the task
# models reshape the vertex rows per graph); what changes with the complex is the number of 1-simplices, 2-simplices and
# adjacencies. pad_batch() fills those up to a capacity with simplices and adjacencies that no real row ever hears of.


@dataclass(frozen=True)
class BatchCapacity:
    simplices: Tuple[int, ...]   # rows per dimension (n_0, ..., n_maxdim); n_0 is the exact vertex count, never padded
    edges: int                   # adjacencies

    @property
    def max_dim(self) -> int:
        return len(self.simplices) - 1

    @property
    def rows(self) -> int:
        return int(sum(self.simplices))


def _real_counts(batch, max_dim: int):
    """(rows per dimension, adjacencies) of the real part of a (possibly padded) batch."""
    n_rows = int(getattr(batch, "n_real_rows", batch.node_types.shape[0]))
    n_edges = int(getattr(batch, "n_real_edges", batch.edge_index.shape[1]))
    nt = batch.node_types[:n_rows].cpu()
    if nt.numel() and (int(nt.min()) < 0 or int(nt.max()) > max_dim):
        raise ValueError(f"node_types outside [0, {max_dim}]")
    return torch.bincount(nt, minlength=max_dim + 1).tolist(), n_edges


def capacity_of(batches: Sequence["SimplicialBatch"], slack: float = 0.0) -> BatchCapacity:
    """The element-wise maximum of the row counts per dimension and of the adjacency counts of `batches`, the d >= 1 counts
    and the adjacencies enlarged by the fraction `slack` (for batches yet to come) - and always at least one spare
    1-simplex: filler adjacencies are self-loops on filler rows, so there must be one."""
    if not batches:
        raise ValueError("capacity_of: no batches")
    if slack < 0:
        raise ValueError("capacity_of: slack must be >= 0")
    max_dim = int(batches[0].x_ind.shape[1]) - 1
    if max_dim < 1:
        raise ValueError("capacity_of: batches without 1-simplices cannot be padded")
    rows, edges = [0] * (max_dim + 1), 0
    for b in batches:
        if int(b.x_ind.shape[1]) - 1 != max_dim:
            raise ValueError("capacity_of: the batches differ in max_dim")
        r, e = _real_counts(b, max_dim)
        rows = [max(a, c) for a, c in zip(rows, r)]
        edges = max(edges, e)
    grow = lambda n: int(math.ceil(n * (1.0 + slack)))
    return BatchCapacity((rows[0], max(grow(rows[1]), rows[1] + 1)) + tuple(grow(n) for n in rows[2:]), grow(edges))


_STRUCTURE = ("x_ind", "node_types", "edge_index", "edge_types", "batch", "ptr", "x_ind_batch", "x_ind_ptr")


def pad_batch(batch: "SimplicialBatch", capacity: BatchCapacity, simplex_features: Sequence[str] = ()) -> "SimplicialBatch":
    """A CPU batch of exactly the capacity's shapes: `batch` (collated; an already padded one is cut back to its real part
    first) with filler simplices and filler adjacencies behind the real ones.

    Real rows keep their indices and real adjacencies their positions; ptr / x_ind_ptr are unchanged and still end at the
    real row count, so per-graph pooling over them never sees a filler. Filler d-simplices (d >= 1, dimension by dimension
    behind the last graph): node_types = d, x_ind = the local vertex ids 0..d, batch = x_ind_batch = B - 1 (their vertex
    rows are real vertices of the last graph: every gather stays in range), zero rows in the per-simplex tensors named in
    `simplex_features` (every other tensor - per-graph labels, per-vertex targets - is passed on as it is). Filler
    adjacencies: self-loops on the filler rows, round-robin, edge_types (d, d). No adjacency joins a filler and a real
    row: messages never cross, a loss that reads real rows sends no gradient into a filler row, and real results do not
    depend on what the fillers hold.

    Everything the device code will index with is validated HERE, on the host (the in-place rebuild on the device,
    SimplicialBatch.refresh_, checks nothing): ValueError for node_types outside [0, max_dim], x_ind outside its graph,
    x_ind_batch / edge_index out of range, a vertex count other than the capacity's, a count above its capacity, filler
    adjacencies without a filler row, a last graph with fewer than d + 1 vertices. The result records n_real_rows and
    n_real_edges."""
    max_dim = capacity.max_dim
    cpu = {k: getattr(batch, k).cpu() for k in batch._names}
    S = int(getattr(batch, "n_real_rows", cpu["node_types"].shape[0]))
    E = int(getattr(batch, "n_real_edges", cpu["edge_index"].shape[1]))
    S_all = int(cpu["node_types"].shape[0])
    for name in simplex_features:
        if name not in cpu:
            raise ValueError(f"pad_batch: the batch has no tensor {name!r}")
        if name in _STRUCTURE or int(cpu[name].shape[0]) != S_all:
            raise ValueError(f"pad_batch: {name!r} is not a per-simplex feature tensor [{S_all}, ...]")
    if S != S_all or E != int(cpu["edge_index"].shape[1]):        # padded before: back to the real part
        for k in ("x_ind", "node_types", "batch", "x_ind_batch") + tuple(simplex_features):
            cpu[k] = cpu[k][:S]
        cpu["edge_index"] = cpu["edge_index"][:, :E]
        if "edge_types" in cpu:
            cpu["edge_types"] = cpu["edge_types"][:E]
    # numpy from here on (views of the CPU tensors): this runs once per training step on the host, in front of every replay,
    # and a few dozen small single-threaded array operations cost a fraction of the same tensor operations
    x_ind, nt, ei = cpu["x_ind"].numpy(), cpu["node_types"].numpy(), cpu["edge_index"].numpy()
    ptr, xb = cpu["x_ind_ptr"].numpy().astype(np.int64), cpu["x_ind_batch"].numpy()
    B = int(ptr.shape[0]) - 1
    if x_ind.ndim != 2 or int(x_ind.shape[1]) < max_dim + 1:
        raise ValueError(f"pad_batch: x_ind has {tuple(x_ind.shape)[1:]} columns, max_dim = {max_dim} needs {max_dim + 1}")
    if int(x_ind.shape[0]) != S or int(xb.shape[0]) != S or int(cpu["batch"].shape[0]) != S:
        raise ValueError("pad_batch: x_ind, node_types, batch and x_ind_batch must have one row per simplex")
    if B < 1 or int(ptr[0]) != 0 or int(ptr[-1]) != S or bool((ptr[1:] < ptr[:-1]).any()) or not np.array_equal(cpu["ptr"].numpy(), ptr):
        raise ValueError("pad_batch: ptr / x_ind_ptr must ascend from 0 to the row count")
    if S and (int(nt.min()) < 0 or int(nt.max()) > max_dim):
        raise ValueError(f"pad_batch: node_types outside [0, {max_dim}]")
    for name, g in (("x_ind_batch", xb), ("batch", cpu["batch"].numpy())):
        if S and (int(g.min()) < 0 or int(g.max()) >= B):
            raise ValueError(f"pad_batch: {name} outside [0, {B})")
    size = (ptr[1:] - ptr[:-1])[xb]                      # rows of the graph of every simplex
    if S and (int(x_ind.min()) < 0 or bool((x_ind >= size[:, None]).any())):
        raise ValueError("pad_batch: x_ind points outside the graph of its simplex")
    if ei.ndim != 2 or int(ei.shape[0]) != 2:
        raise ValueError("pad_batch: edge_index must be [2, E]")
    if E and (int(ei.min()) < 0 or int(ei.max()) >= S):
        raise ValueError(f"pad_batch: edge_index outside [0, {S})")
    counts = np.bincount(nt, minlength=max_dim + 1).tolist()
    if counts[0] != capacity.simplices[0]:
        raise ValueError(f"pad_batch: {counts[0]} vertex rows, the capacity has {capacity.simplices[0]} (vertex rows are never padded)")
    for d in range(1, max_dim + 1):
        if counts[d] > capacity.simplices[d]:
            raise ValueError(f"pad_batch: {counts[d]} {d}-simplices exceed the capacity of {capacity.simplices[d]}")
    if E > capacity.edges:
        raise ValueError(f"pad_batch: {E} adjacencies exceed the capacity of {capacity.edges}")
    fill = [0] + [capacity.simplices[d] - counts[d] for d in range(1, max_dim + 1)]
    n_fill, e_fill = sum(fill), capacity.edges - E
    if e_fill and not n_fill:
        raise ValueError(f"pad_batch: {e_fill} filler adjacencies, but the capacity leaves no filler row to carry them")
    last_vertices = int((nt[int(ptr[B - 1]):] == 0).sum())
    for d in range(1, max_dim + 1):
        if fill[d] and last_vertices < d + 1:
            raise ValueError(f"pad_batch: the last graph has {last_vertices} vertices, a filler {d}-simplex needs {d + 1}")
    f_types = np.repeat(np.arange(max_dim + 1, dtype=np.int64), fill)
    cols = np.arange(int(x_ind.shape[1]), dtype=np.int64)[None, :]
    f_x = np.where(cols <= f_types[:, None], cols, 0)
    f_graph = np.full((n_fill,), B - 1, dtype=np.int64)
    f_rows = S + (np.arange(e_fill, dtype=np.int64) % max(n_fill, 1))

    def extend(name, tail, axis=0):
        a = cpu[name].numpy()
        return torch.from_numpy(np.ascontiguousarray(np.concatenate([a, tail.astype(a.dtype)], axis=axis)))

    out = dict(cpu)
    out["x_ind"] = extend("x_ind", f_x)
    out["node_types"] = extend("node_types", f_types)
    out["batch"] = extend("batch", f_graph)
    out["x_ind_batch"] = extend("x_ind_batch", f_graph)
    out["edge_index"] = extend("edge_index", np.stack([f_rows, f_rows]), axis=1)
    if "edge_types" in cpu:
        f_et = f_types[f_rows - S] if e_fill else np.zeros(0, dtype=np.int64)
        out["edge_types"] = extend("edge_types", np.stack([f_et, f_et], axis=1))
    for name in simplex_features:
        t = cpu[name]
        out[name] = extend(name, np.zeros((n_fill,) + tuple(t.shape[1:]), dtype=t.numpy().dtype))
    padded = SimplicialBatch(**{k: out[k] for k in batch._names})
    padded.n_real_rows, padded.n_real_edges = S, E
    return padded


# ------------------------------------------------------------------------------- complexes built on the device
#
# A complex that depends on the current positions (a loader that does not pre-lift, jittered positions, a rollout that
# re-lifts from predicted positions) is lifted on the device at a fixed capacity (csmpn_rips_lift, csrc/lift.hip): the
# structure tensors come out exactly as pad_batch(collate([rips_complex(...)])) lays them out, and relift_ rebuilds the
# rest in place in front of a replayed step. The clique complex of the k-nearest-neighbour graph (knn_clique_complex, the
# reference's aspirin configuration) is lifted the same way by csmpn_knn_lift: knn_capacity, knn_batch_device,
# relift_(points, knn=k); the convex-hull complex (hull_complex(method="exact"), the hulls task) with its volume by
# csmpn_hull_lift: hull_capacity, hull_batch_device, relift_(points, hull=True); the thresholded clique complex of any graph
# (clique_complex: a caller's edge list or the kNN graph, edge_th / tri_th) by csmpn_clique_lift: clique_capacity,
# clique_batch_device, relift_(points, edges=... | knn=k, edge_th=..., tri_th=...).
# Those four hold at most 64 vertices per graph (hulls: 16). The Rips complex of a point cloud of up to 4096 vertices per graph -
# one cloud of a few thousand points is a batch of one graph - is lifted by csmpn_cloud_lift, with or without the 0-0 block
# over the non-edges: cloud_capacity, cloud_batch_device, relift_(points, dis=...) on such a batch; the clique complex of its
# k-nearest-neighbour graph by csmpn_cloud_knn_lift: knn_capacity, knn_cloud_batch_device, relift_(points, knn=k).


def _lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """One workspace that serves all three device lifts of a batch: the largest of their queries."""
    from csmpn_hip import ops
    sizes = [query(n_graphs, verts_per_graph, max_dim, device)
             for query in (ops.rips_lift_workspace, ops.knn_lift_workspace, ops.hull_lift_workspace)]
    return max(sizes, key=lambda t: t.numel())


def rips_adjacencies(n_graphs: int, verts_per_graph: int, n_edges: int, n_triangles: int) -> int:
    """Adjacencies of a batch of Rips complexes with n_edges 1-simplices and n_triangles 2-simplices in all: per graph the
    V (V - 1) + n1 entries of the 0_0 block (2 n1 through a shared edge + the V (V - 1) - n1 ordered non-edges), 2 n1 each
    of 0_1 and 1_0, 6 n2 of 1_1 and 3 n2 each of 1_2 and 2_1 (lift())."""
    return int(n_graphs) * int(verts_per_graph) * (int(verts_per_graph) - 1) + 5 * int(n_edges) + 12 * int(n_triangles)


def rips_capacity(n_graphs: int, verts_per_graph: int, max_edges: int, max_triangles: int, max_dim: int = 2) -> BatchCapacity:
    """The capacity that serves every batch of n_graphs Rips complexes on verts_per_graph vertices each with at most
    max_edges 1-simplices and max_triangles 2-simplices in all - with one spare 1-simplex, the filler row that carries the
    filler adjacencies of every smaller batch."""
    if max_dim not in (1, 2):
        raise ValueError("rips_capacity: max_dim must be 1 or 2")
    if n_graphs < 1 or verts_per_graph < max_dim + 1 or max_edges < 0 or max_triangles < 0:
        raise ValueError("rips_capacity: need n_graphs >= 1, verts_per_graph >= max_dim + 1 and counts >= 0")
    if max_dim == 1:
        max_triangles = 0
    rows = (n_graphs * verts_per_graph, max_edges + 1) + ((max_triangles,) if max_dim == 2 else ())
    return BatchCapacity(rows, rips_adjacencies(n_graphs, verts_per_graph, max_edges, max_triangles))


def cloud_capacity(n_graphs: int, verts_per_graph: int, max_edges: int, max_triangles: int, max_dim: int = 2,
                   vertex_block: bool = False) -> BatchCapacity:
    """rips_capacity for the batches of cloud_batch_device (up to 4096 vertices per graph): the same rows; the adjacencies are
    rips_adjacencies with the vertex block and clique_adjacencies (6 n1 + 12 n2) without it, the default - the block has
    V (V - 1) - n1 entries per graph."""
    cap = rips_capacity(n_graphs, verts_per_graph, max_edges, max_triangles, max_dim)
    return cap if vertex_block else BatchCapacity(cap.simplices, clique_adjacencies(max_edges, cap.simplices[2] if max_dim == 2 else 0))


def clique_adjacencies(n_edges: int, n_triangles: int) -> int:
    """Adjacencies of clique complexes (lift(..., vertex_block=False)) with n_edges 1-simplices and n_triangles 2-simplices in
    all: 2 n1 each of 0_0 (through a shared edge), 0_1 and 1_0, 6 n2 of 1_1 and 3 n2 each of 1_2 and 2_1."""
    return 6 * int(n_edges) + 12 * int(n_triangles)


def knn_capacity(n_graphs: int, verts_per_graph: int, k: int, max_triangles: int, max_edges: Optional[int] = None,
                 max_dim: int = 2) -> BatchCapacity:
    """The capacity that serves every batch of n_graphs k-nearest-neighbour clique complexes on verts_per_graph vertices each
    with at most max_triangles 2-simplices and max_edges 1-simplices in all (default: the bound n_graphs * min(k V,
    V (V - 1) / 2) - every vertex names k neighbours) - with the one spare 1-simplex of rips_capacity."""
    if max_dim not in (1, 2):
        raise ValueError("knn_capacity: max_dim must be 1 or 2")
    if n_graphs < 1 or verts_per_graph < max_dim + 1 or k < 1 or max_triangles < 0 or (max_edges is not None and max_edges < 0):
        raise ValueError("knn_capacity: need n_graphs >= 1, verts_per_graph >= max_dim + 1, k >= 1 and counts >= 0")
    if max_edges is None:
        max_edges = n_graphs * min(k * verts_per_graph, verts_per_graph * (verts_per_graph - 1) // 2)
    if max_dim == 1:
        max_triangles = 0
    rows = (n_graphs * verts_per_graph, max_edges + 1) + ((max_triangles,) if max_dim == 2 else ())
    return BatchCapacity(rows, clique_adjacencies(max_edges, max_triangles))


def clique_capacity(n_graphs: int, verts_per_graph: int, max_edges: Optional[int] = None, max_triangles: Optional[int] = None,
                    max_dim: int = 2) -> BatchCapacity:
    """The capacity that serves every batch of n_graphs thresholded clique complexes (clique_complex) on verts_per_graph vertices
    each with at most max_edges 1-simplices and max_triangles 2-simplices in all (defaults: every pair and every triple,
    n_graphs C(V, 2) and n_graphs C(V, 3) - a caller's graph has no bound of its own) - with the one spare 1-simplex of
    rips_capacity. The adjacencies are clique_adjacencies of these counts (no vertex block)."""
    if max_dim not in (1, 2):
        raise ValueError("clique_capacity: max_dim must be 1 or 2")
    if n_graphs < 1 or verts_per_graph < max_dim + 1 or (max_edges is not None and max_edges < 0) or \
            (max_triangles is not None and max_triangles < 0):
        raise ValueError("clique_capacity: need n_graphs >= 1, verts_per_graph >= max_dim + 1 and counts >= 0")
    if max_edges is None:
        max_edges = n_graphs * math.comb(verts_per_graph, 2)
    if max_triangles is None:
        max_triangles = n_graphs * math.comb(verts_per_graph, 3)
    if max_dim == 1:
        max_triangles = 0
    rows = (n_graphs * verts_per_graph, max_edges + 1) + ((max_triangles,) if max_dim == 2 else ())
    return BatchCapacity(rows, clique_adjacencies(max_edges, max_triangles))


def hull_capacity(n_graphs: int, verts_per_graph: int, max_dim: int = 2, max_edges: Optional[int] = None,
                  max_triangles: Optional[int] = None) -> BatchCapacity:
    """The capacity that serves every batch of n_graphs convex-hull complexes on verts_per_graph vertices each with at most
    max_edges 1-simplices and max_triangles 2-simplices in all (defaults: every pair and every triple, n_graphs C(V, 2) and
    n_graphs C(V, 3)) - with the one spare 1-simplex of rips_capacity. The adjacencies are those of a Rips complex with
    these counts (rips_adjacencies: the lift has the vertex block)."""
    if max_dim not in (1, 2):
        raise ValueError("hull_capacity: max_dim must be 1 or 2")
    if n_graphs < 1 or verts_per_graph < max_dim + 1 or (max_edges is not None and max_edges < 0) or \
            (max_triangles is not None and max_triangles < 0):
        raise ValueError("hull_capacity: need n_graphs >= 1, verts_per_graph >= max_dim + 1 and counts >= 0")
    if max_edges is None:
        max_edges = n_graphs * math.comb(verts_per_graph, 2)
    if max_triangles is None:
        max_triangles = n_graphs * math.comb(verts_per_graph, 3)
    if max_dim == 1:
        max_triangles = 0
    rows = (n_graphs * verts_per_graph, max_edges + 1) + ((max_triangles,) if max_dim == 2 else ())
    return BatchCapacity(rows, rips_adjacencies(n_graphs, verts_per_graph, max_edges, max_triangles))


def rips_batch_device(points: torch.Tensor, n_graphs: int, dis: float, capacity: BatchCapacity,
                      features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                      x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """The device batch of the Rips complexes of `points` (device float32 [n_graphs * V, n]) at `capacity`, lifted on the
    device - the batch relift_ is then called on. features {name: tensor}: further tensors of the batch as they are
    (per-graph labels, per-vertex targets); vertex_features {name: per-vertex tensor [n_graphs * V, ...]}: per-simplex
    tensors [capacity.rows, ...] that hold these rows at the vertex rows and zeros elsewhere. Synchronises once;
    ValueError if the complex does not fit the capacity."""
    return _lifted_batch_device("rips_batch_device", "rips_lift", points, n_graphs, dis, capacity, features, vertex_features, x_ind_cols)


def knn_batch_device(points: torch.Tensor, n_graphs: int, k: int, capacity: BatchCapacity,
                     features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                     x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """rips_batch_device for the k-nearest-neighbour clique complexes of the points (knn_clique_complex; csmpn_knn_lift) -
    the batch relift_(points, knn=k) is then called on."""
    return _lifted_batch_device("knn_batch_device", "knn_lift", points, n_graphs, k, capacity, features, vertex_features, x_ind_cols)


def hull_batch_device(points: torch.Tensor, n_graphs: int, capacity: BatchCapacity,
                      features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                      x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """rips_batch_device for the convex-hull complexes of the points (hull_complex(method="exact"); csmpn_hull_lift) - the
    batch relift_(points, hull=True) is then called on, laid out as a hulls sample (hulls_example): `input` [rows, n] holds
    the points at the vertex rows (unless vertex_features names it), `target` [n_graphs] float32 the hulls' volumes as the
    device computed them (unless features names it)."""
    vertex_features = dict(vertex_features or {})
    vertex_features.setdefault("input", points)
    return _lifted_batch_device("hull_batch_device", "hull_lift", points, n_graphs, None, capacity, features, vertex_features, x_ind_cols)


def clique_batch_device(points: torch.Tensor, n_graphs: int, capacity: BatchCapacity, edges: Optional[torch.Tensor] = None,
                        knn: Optional[int] = None, edge_th: float = math.inf, tri_th: float = math.inf,
                        features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                        x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """rips_batch_device for the thresholded clique complexes of the points (clique_complex; csmpn_clique_lift) over exactly
    one of edges=... (int64 [2, n] of GLOBAL vertex ids g V + a, moved to the device of the points; (-1, -1) is padding) and
    knn=k (the k-nearest-neighbour graphs) - the batch relift_(points, edges=... | knn=k, edge_th=..., tri_th=...) is then called
    on. ValueError as well for a list with an end outside the batch or across two graphs (status bit 5)."""
    if (edges is None) == (knn is None):
        raise ValueError("clique_batch_device: pass exactly one of edges=... and knn=...")
    _thresholds_squared("clique_batch_device", edge_th, tri_th)
    source = int(knn) if edges is None else edges.to(points.device)
    return _lifted_batch_device("clique_batch_device", "clique_lift", points, n_graphs, (source, float(edge_th), float(tri_th)), capacity,
                                features, vertex_features, x_ind_cols)


def cloud_batch_device(points: torch.Tensor, n_graphs: int, dis: float, capacity: BatchCapacity, vertex_block: bool = False,
                       features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                       x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """rips_batch_device for point clouds of up to 4096 vertices per graph (rips_complex(points, dis, max_dim, vertex_block);
    csmpn_cloud_lift) - one cloud of a few thousand points is a batch of one graph. The batch's plan records that it is a
    cloud batch and its vertex_block: relift_(points, dis=...) then goes to ops.cloud_lift, and nothing else re-lifts it."""
    return _lifted_batch_device("cloud_batch_device", "cloud_lift", points, n_graphs, (float(dis), bool(vertex_block)), capacity, features,
                                vertex_features, x_ind_cols)


def knn_cloud_batch_device(points: torch.Tensor, n_graphs: int, k: int, capacity: BatchCapacity,
                           features: Optional[Dict[str, torch.Tensor]] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                           x_ind_cols: Optional[int] = None) -> SimplicialBatch:
    """knn_batch_device for point clouds of up to 4096 vertices per graph (knn_clique_complex(points, k, max_dim);
    csmpn_cloud_knn_lift), at a capacity of knn_capacity, whose formula holds for any V. The batch's plan records that it is a
    kNN cloud batch: relift_(points, knn=k) then goes to ops.cloud_knn_lift, and nothing else re-lifts it."""
    return _lifted_batch_device("knn_cloud_batch_device", "cloud_knn_lift", points, n_graphs, int(k), capacity, features, vertex_features,
                                x_ind_cols)


def _lifted_batch_device(what, op, points, n_graphs, param, capacity, features, vertex_features, x_ind_cols) -> SimplicialBatch:
    """The body of rips_batch_device (op = "rips_lift", param = dis), knn_batch_device (op = "knn_lift", param = k),
    hull_batch_device (op = "hull_lift", no parameter; the volumes become `target`), clique_batch_device (op =
    "clique_lift", param = (the list or k, edge_th, tri_th); its larger workspace serves the other lifts as well) and
    cloud_batch_device (op = "cloud_lift", param = (dis, vertex_block); its workspace serves that lift alone), as does that of
    knn_cloud_batch_device (op = "cloud_knn_lift", param = k)."""
    from csmpn_hip import ops
    if not points.is_cuda:
        raise RuntimeError(f"{what} needs device points (no CPU fallback)")
    dev, max_dim, S, E, B = points.device, capacity.max_dim, capacity.rows, capacity.edges, int(n_graphs)
    i64 = lambda *shape: torch.zeros(*shape, dtype=torch.int64, device=dev)
    tensors = dict(x_ind=i64(S, max_dim + 1 if x_ind_cols is None else int(x_ind_cols)), node_types=i64(S), edge_index=i64(2, E),
                   edge_types=i64(E, 2), batch=i64(S), ptr=i64(B + 1), x_ind_batch=i64(S), x_ind_ptr=i64(B + 1))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    counts = i64(max_dim + 2)
    clique, cloud, cloud_knn = op == "clique_lift", op == "cloud_lift", op == "cloud_knn_lift"
    ws = ops.clique_lift_workspace(B, int(points.shape[0]) // max(B, 1), max_dim, dev) if clique else \
        ops.cloud_lift_workspace(B, int(points.shape[0]) // max(B, 1), max_dim, dev) if cloud else \
        ops.cloud_knn_lift_workspace(B, int(points.shape[0]) // max(B, 1), max_dim, dev) if cloud_knn else \
        _lift_workspace(B, int(points.shape[0]) // max(B, 1), max_dim, dev)
    volume = torch.zeros(B, dtype=torch.float32, device=dev) if op == "hull_lift" else None
    run = getattr(ops, op) if volume is None else (lambda p, b, _, *rest: ops.hull_lift(p, b, *rest, volume=volume))
    if clique:
        run = lambda p, b, src, *rest: ops.clique_lift(p, b, src[0], *rest, edge_th=src[1], tri_th=src[2])
    if cloud:
        run = lambda p, b, prm, *rest: ops.cloud_lift(p, b, prm[0], *rest, vertex_block=prm[1])
    run(points, B, param, max_dim, capacity.simplices, E, tensors["x_ind"], tensors["node_types"], tensors["batch"],
        tensors["x_ind_batch"], tensors["ptr"], tensors["x_ind_ptr"], tensors["edge_index"], tensors["edge_types"], counts, status, ws)
    word = int(status.item())
    if word:
        raise ValueError(f"{what}: the complex does not fit the capacity {capacity} (status {word:#x}: bit 1 / 2 = too "
                         "many 1- / 2-simplices, bit 3 = too many adjacencies, bit 4 = filler adjacencies without a filler row"
                         + (", bit 5 = an edge list with an end outside the batch or across two graphs)" if clique else ")"))
    vertex_rows = torch.nonzero(tensors["node_types"] == 0, as_tuple=False).flatten()
    for name, value in (vertex_features or {}).items():
        t = torch.zeros((S,) + tuple(value.shape[1:]), dtype=value.dtype, device=dev)
        t.index_copy_(0, vertex_rows, value.to(dev))
        tensors[name] = t
    if volume is not None:
        tensors["target"] = volume
    for name, value in (features or {}).items():
        tensors[name] = value.to(dev)
    out = SimplicialBatch(**tensors)
    out.plan(max_dim)
    out.csr()
    plan = out._plan
    plan["lift_ws"], plan["lift_status"], plan["lift_counts"] = ws, status, counts
    if clique:
        plan["clique_lift_ws"] = ws
    if cloud:
        plan["cloud"] = {"vertex_block": param[1]}
    if cloud_knn:
        plan["cloud_knn"] = {"k": param}
    return out
