"""Thresholded clique-lift fixtures from the IMPORTED reference data modules (build container only; exits cleanly where the
reference is absent).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_thresholded_complex_golden.py

Pins csmpn.data.complexes.clique_complex - the edges of a graph G no longer than edge_th, the triangles of G of area at most
tri_th, the pairs of every kept triangle brought back, lift(..., vertex_block=False) - to the reference's own
`simplicial_lift(graph, edge_th, tri_th)` (csmpn/data/modules/utils.py:151-207) with FINITE thresholds, behind the stand-ins of
make_knn_complex_golden.py (imported from there: gudhi.SimplexTree as a face-closed set of vertex tuples, torch_geometric's
Data as an attribute bag; no arithmetic of the path), followed by `SimplicialTransform.add_missing_adj` / `get_num_simplicies`
/ `get_edge` / `gen_simplicial_type_feat` as there.

Cases: the k-nearest-neighbour lists (this project's knn_edges) of five seeded point sets in R^3, four threshold pairs each,
and one list that is no k-nearest-neighbour graph - a ring of 13 vertices with four chords - with two pairs. A threshold pair
(qe, qt) sits midway between two neighbouring values at the qe quantile of G's edge lengths and the qt quantile of the areas of
G's triangles; qe = 0.0 means HALF THE SHORTEST EDGE: every edge fails, the 1-simplices come from kept triangles alone. The
reference compares in float32, this project in float64: a case whose threshold lies within a relative 1e-4 of any edge length
or triangle area of G is refused, so the two cannot disagree.

Writes complexes_th_ref.npz: for every case its points, the list (`edges`), edge_th, tri_th and, from the reference: x_<d>
(the vertices of a row sorted), adj_<s>_<t> (incl. the flipped copies), edge_index, edge_attr (type pairs), node_types. Prints
for every case its rows, its "hollow" triples (three 1-simplices that bound no 2-simplex) and its edges brought back by a
triangle (1-simplices longer than edge_th).
"""
import itertools
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import make_knn_complex_golden as KG          # installs the stand-ins and imports the reference (or exits)

RU, Data, SimplicialTransform, SimplicialComplexData = KG.RU, KG.Data, KG.SimplicialTransform, KG.SimplicialComplexData

POINT_SETS = [(21, 3, 0), (9, 3, 1), (12, 4, 2), (6, 5, 3), (16, 5, 7)]                    # (vertices, k, seed)
QUANTILES = [(0.5, 0.5), (0.3, 0.8), (0.8, 0.3), (0.0, 0.5)]
RING = (13, 11, [(0, 2), (3, 5), (6, 8), (9, 11)], [(0.5, 0.5), (0.0, 0.5)])               # (vertices, seed, chords, quantiles)
MIN_GAP = 1e-4


def graph_values(points, edges):
    """(the pairs a < b of G, their lengths, the triples of G, their areas) in float64 on the float32 points."""
    p = points.astype(np.float64)
    pairs = sorted({(min(a, b), max(a, b)) for a, b in edges.T.tolist() if a != b})
    present = set(pairs)
    V = len(p)
    triples = [t for t in itertools.combinations(range(V), 3) if all(q in present for q in itertools.combinations(t, 2))]
    lengths = np.array([np.sqrt(((p[a] - p[b]) ** 2).sum()) for a, b in pairs])
    areas = np.array([0.5 * np.sqrt(max(((p[b] - p[a]) ** 2).sum() * ((p[c] - p[a]) ** 2).sum() - ((p[b] - p[a]) * (p[c] - p[a])).sum() ** 2, 0.0))
                      for a, b, c in triples])
    return pairs, lengths, triples, areas


def midpoint_at(values, q):
    """Midway between two neighbouring sorted values, so that floor(q n) of the n values lie below the threshold."""
    v = np.sort(values)
    i = max(0, min(int(q * len(v)) - 1, len(v) - 2))
    return float(0.5 * (v[i] + v[i + 1]))


def relative_gap(th, values):
    return float(np.min(np.abs(values - th) / np.maximum(np.abs(values), th))) if len(values) else float("inf")


def reference_lift(points, edges, edge_th, tri_th):
    tr = SimplicialTransform(dim=2, label="md17", molecule_type="aspirin", edge_th=edge_th, tri_th=tri_th)
    graph = Data(pos=torch.from_numpy(points), edge_index=torch.from_numpy(edges), y=torch.zeros(1))
    x_dict, adj = RU.simplicial_lift(graph, tr.edge_th, tr.tri_th)
    scd = SimplicialComplexData().from_dict(graph.to_dict())
    for d, v in x_dict.items():
        scd[f"x_{d}"] = v
    for key, v in adj.items():
        scd[f"adj_{key}"] = v
    num_per_dim = tr.get_num_simplicies(x_dict)
    scd = tr.add_missing_adj(scd)
    scd = tr.get_edge(x_dict, scd, num_per_dim)
    scd = tr.gen_simplicial_type_feat(num_per_dim, scd)
    return x_dict, scd


def cases():
    for verts, k, seed in POINT_SETS:
        pts = KG.points_of(seed, verts)
        edges = KG.knn_edges(pts, k).numpy().astype(np.int64)
        for qe, qt in QUANTILES:
            yield f"knn_{verts}_k{k}_s{seed}_e{int(10 * qe)}_t{int(10 * qt)}", pts, edges, qe, qt
    verts, seed, chords, quantiles = RING
    pts = KG.points_of(seed, verts)
    ring = [(i, (i + 1) % verts) for i in range(verts)] + chords
    edges = np.array(ring, dtype=np.int64).T.copy()                        # one direction each: no k-nearest-neighbour list
    for qe, qt in quantiles:
        yield f"ring_{verts}_chords_e{int(10 * qe)}_t{int(10 * qt)}", pts, edges, qe, qt


if __name__ == "__main__":
    out = {}
    for name, pts, edges, qe, qt in cases():
        pairs, lengths, triples, areas = graph_values(pts, edges)
        edge_th = 0.5 * float(lengths.min()) if qe == 0.0 else midpoint_at(lengths, qe)
        tri_th = midpoint_at(areas, qt)
        gap = min(relative_gap(edge_th, lengths), relative_gap(tri_th, areas))
        if gap < MIN_GAP:
            raise SystemExit(f"{name}: a threshold lies within {gap:.2e} (relative) of a value of G: refused")
        x_dict, scd = reference_lift(pts, edges, edge_th, tri_th)
        out[f"{name}/points"] = pts
        out[f"{name}/edges"] = edges
        out[f"{name}/edge_th"] = np.array(edge_th, dtype=np.float64)
        out[f"{name}/tri_th"] = np.array(tri_th, dtype=np.float64)
        for d, v in x_dict.items():
            out[f"{name}/x_{d}"] = np.sort(v.numpy().astype(np.int64), axis=1)
        for key in scd.keys:
            if key.startswith("adj_"):
                out[f"{name}/{key}"] = scd[key].numpy()
        out[f"{name}/edge_index"] = scd.edge_index.numpy()
        out[f"{name}/edge_attr"] = scd.edge_attr.numpy()
        out[f"{name}/node_types"] = scd.node_types.numpy()
        x1 = {tuple(r) for r in out[f"{name}/x_1"].tolist()}
        x2 = {tuple(r) for r in out[f"{name}/x_2"].tolist()} if f"{name}/x_2" in out else set()
        hollow = sum(1 for t in itertools.combinations(range(len(pts)), 3)
                     if t not in x2 and all(q in x1 for q in itertools.combinations(t, 2)))
        back = sum(1 for (a, b), length in zip(pairs, lengths) if length > edge_th and (a, b) in x1)
        print(f"{name}: edge_th {edge_th:.6f} tri_th {tri_th:.6f} gap {gap:.1e} rows {[int(x_dict[d].shape[0]) for d in sorted(x_dict)]} "
              f"of G's {len(pairs)} edges / {len(triples)} triangles, hollow {hollow}, brought back {back}, "
              f"adjacencies {scd.edge_index.shape[1]}")
    np.savez_compressed(os.path.join(HERE, "complexes_th_ref.npz"), **out)
