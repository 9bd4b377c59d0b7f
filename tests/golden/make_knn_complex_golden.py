"""Clique-lift fixtures of k-nearest-neighbour graphs from the IMPORTED reference data modules (build container only; exits
cleanly where the reference is absent).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_knn_complex_golden.py

Pins csmpn.data.complexes.knn_clique_complex - lift(..., vertex_block=False) on the cliques of the symmetrised graph - to the
reference's own code for md17's aspirin configuration: `simplicial_lift` (csmpn/data/modules/utils.py:151-207: nx.Graph of
graph.edge_index, its 2- and 3-cliques, generate_adjacencies without a fully connected 0_0 block) and
`SimplicialTransform.add_missing_adj` / `get_num_simplicies` / `get_edge` / `gen_simplicial_type_feat`
(simplicial_data.py:105-175), with the default edge_th / tri_th (10 000: no simplex is thresholded away).

`graph.edge_index` is the directed list of THIS project's knn_edges: the reference takes it from torch_cluster.knn_graph,
which is not installed, so the tie rule of the neighbour search is ours (the seeded points below have pairwise distinct
distances, where the k-nearest-neighbour graph does not depend on a tie rule). networkx is the installed one. `gudhi` and
`torch_geometric.data` / `.transforms` / `.typing` / `torch_scatter` are replaced by in-memory stand-ins that hold no
arithmetic of the path, of the kind make_complex_golden.py documents:

  gudhi.SimplexTree   a set of vertex tuples closed under faces.
                      get_simplices(): lexicographic order of the sorted vertex tuples (the pre-order walk of gudhi's simplex
                      trie), filtration 0.0; get_boundaries(s): the facets of s, removing the LAST vertex first;
                      get_cofaces(s, 1): the simplices with one more vertex that contain s, in get_simplices order.
                      The enumeration order decides the ORDER of the adjacency columns inside one type and nothing else: the
                      test compares adjacency types as sorted multisets and everything else exactly.
  torch_geometric.data.Data   an attribute bag with item access, `keys`, `to_dict` / `from_dict`.

The points live in R^3: the reference takes a cross product for the triangle areas.

Writes complexes_knn_ref.npz: for every case its points, k and, from the reference: x_<d> (the vertices of a row sorted: the
reference fills a row from a frozenset, whose iteration order is not part of the format), adj_<s>_<t> (incl. the flipped
copies), edge_index, edge_attr (type pairs), node_types.
"""
import itertools
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)

import numpy as np
import torch

import pyg_standin

REF = os.environ.get("CSMPN_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    print("reference not present: nothing to do")
    sys.exit(0)

# (name, vertices, k, seed): aspirin's shape and k; a small one; k = 2 (chains, few triangles); k = V - 1 (complete)
CASES = [("aspirin_21_k3", 21, 3, 0), ("nine_k3", 9, 3, 1), ("twelve_k2", 12, 2, 2), ("complete_6_k5", 6, 5, 3)]


def points_of(seed, verts):
    return np.random.default_rng(seed).standard_normal((verts, 3)).astype(np.float32)


# this project's knn_edges, loaded from its file without the package (which would load the native library); the module is
# registered under a private name so that it cannot shadow the reference's `csmpn` package imported below
def load_knn_edges():
    import importlib.util
    pkg = [d for d in os.listdir(ROOT) if os.path.isfile(os.path.join(ROOT, d, "csmpn", "data", "complexes.py"))][0]
    spec = importlib.util.spec_from_file_location("_project_complexes", os.path.join(ROOT, pkg, "csmpn", "data", "complexes.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules["_project_complexes"] = mod
    spec.loader.exec_module(mod)
    return mod.knn_edges


# ----------------------------------------------------------------------------- stand-ins (no arithmetic of the path)
class SimplexTree:
    def __init__(self):
        self._s = set()

    def insert(self, simplex, filtration=0.0):
        verts = tuple(sorted(int(v) for v in simplex))
        for k in range(1, len(verts) + 1):
            for sub in itertools.combinations(verts, k):
                self._s.add(sub)
        return True

    def get_simplices(self):
        for s in sorted(self._s):
            yield list(s), 0.0

    def get_boundaries(self, simplex):
        s = list(simplex)
        if len(s) == 1:
            return
        for drop in range(len(s) - 1, -1, -1):
            yield s[:drop] + s[drop + 1:], 0.0

    def get_cofaces(self, simplex, codim):
        base = set(simplex)
        return [(list(t), 0.0) for t in sorted(self._s) if len(t) == len(simplex) + codim and base.issubset(t)]


class Data:
    def __init__(self, **kw):
        for k, v in kw.items():
            setattr(self, k, v)

    def __getitem__(self, k):
        return getattr(self, k)

    def __setitem__(self, k, v):
        setattr(self, k, v)

    @property
    def keys(self):
        return [k for k in self.__dict__ if not k.startswith("_")]

    def to_dict(self):
        return {k: getattr(self, k) for k in self.keys}

    def from_dict(self, d):
        out = type(self)()
        for k, v in d.items():
            setattr(out, k, v)
        return out


def install_standins():
    pyg_standin.install()
    g = types.ModuleType("gudhi")
    gst = types.ModuleType("gudhi.simplex_tree")
    g.SimplexTree = gst.SimplexTree = SimplexTree
    g.simplex_tree = gst
    sys.modules["gudhi"], sys.modules["gudhi.simplex_tree"] = g, gst
    tg = sys.modules["torch_geometric"]
    for name, attrs in (("torch_geometric.data", {"Data": Data}), ("torch_geometric.typing", {"Adj": object}),
                        ("torch_geometric.transforms", {"BaseTransform": object})):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        setattr(tg, name.split(".")[-1], m)
    ts = types.ModuleType("torch_scatter")
    ts.scatter = None
    sys.modules["torch_scatter"] = ts


knn_edges = load_knn_edges()
install_standins()
sys.path.insert(0, REF)
from csmpn.data.modules import utils as RU  # noqa: E402
from csmpn.data.modules.simplicial_data import SimplicialTransform, SimplicialComplexData  # noqa: E402


def reference_lift(points, k):
    tr = SimplicialTransform(dim=2, label="md17", molecule_type="aspirin")      # default edge_th / tri_th
    graph = Data(pos=torch.from_numpy(points), edge_index=knn_edges(points, k), y=torch.zeros(1))
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


if __name__ == "__main__":
    out = {}
    for name, verts, k, seed in CASES:
        pts = points_of(seed, verts)
        x_dict, scd = reference_lift(pts, k)
        out[f"{name}/points"] = pts
        out[f"{name}/k"] = np.array(k)
        for d, v in x_dict.items():
            out[f"{name}/x_{d}"] = np.sort(v.numpy().astype(np.int64), axis=1)
        for key in scd.keys:
            if key.startswith("adj_"):
                out[f"{name}/{key}"] = scd[key].numpy()
        out[f"{name}/edge_index"] = scd.edge_index.numpy()
        out[f"{name}/edge_attr"] = scd.edge_attr.numpy()
        out[f"{name}/node_types"] = scd.node_types.numpy()
        print(name, {key: tuple(v.shape) for key, v in out.items() if key.startswith(name + "/adj_")}, "rows",
              [int(x_dict[d].shape[0]) for d in sorted(x_dict)], "edges", scd.edge_index.shape[1])
    np.savez_compressed(os.path.join(HERE, "complexes_knn_ref.npz"), **out)
