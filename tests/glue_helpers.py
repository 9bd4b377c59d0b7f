"""Cases and plain references of the kernels either side of the message passing (csrc/glue.hip): csmpn_simplex_rows,
csmpn_readout_mse_*, csmpn_readout_traj_* and csmpn_type_attr_*, for tests/test_glue_reference_cpu.py (validates the
references, no GPU) and tests/test_glue_kernels_gpu.py (holds the kernels to them).

Every reference is torch on the CPU and generic in dtype: the float64 run is the truth, the float32 run of the same code
the yardstick. They are written from the formulas in the comments of glue.hip and from the model statements
those comments cite (hulls_cssmpnn.py:93,155-164, md17_cssmpnn.py:165-176, motion_cssmpnn.py:150-168,
nba_cssmpnn.py:176-191), not from the kernels' loops: no pass, tile or thread-group structure appears below. Gradients
come from autograd (type attributes: a float64 index_add, the adjoint of a gather).

The case tables name, per case, the loop or shape edge it reaches; the inputs of a case follow from its seed alone.
Importing this module needs no GPU and no native library.
"""
import functools

import numpy as np
import torch

from general_helpers import TOL, check, relmax  # noqa: F401  (re-exported: the bound of DESIGN.md §2)
from oracle import ref_path as O

# Seed offsets of cases whose first seed gives an input on which the float32 reference itself misses the bound with
# factor 1 (test_glue_reference_cpu.py measures that); as lane_d32_helpers.RESEED. None was needed.
RESEED = {}


def _gen(tag, base):
    return torch.Generator().manual_seed(base + 7919 * RESEED.get(tag, 0))


def algebra(n, dtype=torch.float64):
    return O.Algebra([1.0] * n, dtype)


# ================================================================================================ trajectory readout
# n, C (channels of x), O (out channels), vertices per graph, rows of x that are no vertex, unscored_last, loc, identity
# rows (vertex_rows = None); kTrajItems = 1024 items (vertex, out channel) per pass -> vper = 1024 // O vertices per pass.
def _traj(n, C, O, sizes, extra, unscored_last, loc, seed, identity=False, seed_tag=None):
    return dict(n=n, C=C, O=O, sizes=tuple(sizes), extra=extra, unscored_last=unscored_last, loc=loc, seed=seed,
                identity=identity, seed_tag=seed_tag)


TRAJ_CASES = {
    # C O = 4096; vper = 16: the graph of 20 takes two passes, the second partial; four vertex groups; an empty graph
    "T1": _traj(3, 64, 64, (3, 0, 20, 1), 7, 0, True, 4101),
    # vper = 25 (1000 of 1024 items): passes of 25/25/10 and 25/1; six vertex groups + idle threads; the NBA ball
    "T2": _traj(2, 40, 40, (60, 11, 26), 5, 1, False, 4102),
    # vper = 1024: two passes, the per-vertex loop strides; 257 = 256 + 1
    "T3": _traj(3, 16, 1, (1500, 31, 0, 257), 9, 0, True, 4103),
    # T3 with identity rows (vertex_rows = None, no row that is no vertex)
    "T3i": _traj(3, 16, 1, (1500, 31, 0, 257), 0, 0, True, 4103, identity=True),
    # O at its limit: one vertex per pass; all five vector blades
    "T4": _traj(5, 4, 1024, (3, 1), 0, 0, False, 4104),
    # vper = 32 divides exactly; the graph of 2 is wholly unscored (cnt = 0); 256 vertex groups
    "T5": _traj(3, 1, 32, (33, 32, 2), 3, 2, True, 4105),
    # vper = 341 (1023 items): graphs of vper + 1, vper, and two passes + a tail
    "T6": _traj(2, 5, 3, (342, 341, 700), 4, 1, True, 4106),
}
TRAJ_ALONE = ("T2", "T5")     # per_graph alone and per_vertex alone: the g_graph / g_vertex null-pointer branches
# the |d| = 0 items of T5: one whole scored vertex (its last out channel is the FDE item) and one further single item
T5_TIES = tuple((5, o) for o in range(32)) + ((40, 7),)


def scored_vertices(sizes, unscored_last):
    """(vertices that are scored, their graphs): the last `unscored_last` vertices of every graph are not scored (NBA: the
    ball, nba_cssmpnn.py:182); the target rows number the scored vertices consecutively."""
    scored, graph, v = [], [], 0
    for b, s in enumerate(sizes):
        for i in range(s):
            if i < s - unscored_last:
                scored.append(v)
                graph.append(b)
            v += 1
    return scored, graph


def traj_tables_loop(sizes, vrows=None, n_rows=None, unscored_last=0):
    """The tables of ops.readout_traj_tables by plain Python loops (int32 tensors, None where the op returns None)."""
    vptr, gov, trow, nxt = [0], [], [], 0
    for b, s in enumerate(sizes):
        vptr.append(vptr[-1] + s)
        for i in range(s):
            gov.append(b)
            if i < s - unscored_last:
                trow.append(nxt)
                nxt += 1
            else:
                trow.append(-1)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32)
    out = {"vptr": i32(vptr), "graph_of_vertex": i32(gov), "trow": i32(trow) if unscored_last else None, "vrows": None,
           "vertex_of_row": None}
    if vrows is not None:
        vof = [-1] * int(n_rows)
        for v, r in enumerate(vrows.tolist()):
            vof[r] = v
        out["vrows"], out["vertex_of_row"] = i32(vrows.tolist()), i32(vof)
    return out


def traj_topology(tag, second=False):
    """(sizes, vrows or None, n_rows) of a case; second = another batch of the same shapes (the sizes rotated by one graph,
    another permutation) for the in-place refill of the tables. The vertex rows are the head of a seeded permutation of
    the rows of x: not monotone."""
    c = TRAJ_CASES[tag]
    sizes = c["sizes"][1:] + c["sizes"][:1] if second else c["sizes"]
    V = sum(sizes)
    if c["identity"]:
        return sizes, None, V
    g = _gen(c["seed_tag"] or tag, c["seed"] + (50000 if second else 0))
    return sizes, torch.randperm(V + c["extra"], generator=g)[:V], V + c["extra"]


@functools.lru_cache(maxsize=None)
def traj_inputs(tag):
    """float32 CPU inputs of a case: N(0,1) x, loc, target and incoming gradients, weight [O, C, n + 1] ~ N(0,1) / sqrt(C)."""
    c = TRAJ_CASES[tag]
    sizes, vrows, S = traj_topology(tag)
    n, C, Oc, V = c["n"], c["C"], c["O"], sum(sizes)
    g = _gen(c["seed_tag"] or tag, c["seed"] + 1)
    rn = lambda *s: torch.randn(*s, generator=g)
    scored, _ = scored_vertices(sizes, c["unscored_last"])
    return dict(n=n, sizes=sizes, vrows=vrows, n_rows=S, unscored_last=c["unscored_last"], x=rn(S, C, 1 << n),
                weight=rn(Oc, C, n + 1) / C ** 0.5, loc=rn(V, Oc, n) if c["loc"] else None, target=rn(len(scored), Oc, n),
                g_graph=rn(len(sizes), 3), g_vertex=rn(V))


def traj_forward(x, weight, loc, target, sizes, vrows, unscored_last, n, ties=()):
    """(pred [V, O, n], per_graph [B, 3] = (MSE, ADE, FDE), per_vertex [V]), differentiable:
        pred[v, o]   = sum_c W[o, c, grade 1] x[row(v), c, vector blades] (+ loc[v, o])
        d[v, o]      = pred[v, o] - target[scored position of v, o]      for the scored vertices only
        per_graph[b] = (sum |d|^2 / (cnt O), sum |d| / (cnt O), sum_v |d[v, O - 1]| / cnt), cnt = max(scored vertices of b, 1)
        per_vertex[v] = sum_{o, a} d^2 / (O n), 0 where v is not scored.
    Norms are taken over scored items only, selected by indexing (a `where` over all vertices differentiates sqrt at the 0
    of the unscored ones: NaN). The project's convention for |d| at d = 0 is the subgradient 0: items with |d|^2 = 0 are
    left out of the square root by indexing as well. `ties` = [(vertex, out channel)]: the target of such an item IS the
    prediction (what a caller gets who feeds a prediction back as the target), so d = 0 exactly in every dtype."""
    xv = x if vrows is None else x.index_select(0, vrows)
    V, Oc, B = xv.shape[0], weight.shape[0], len(sizes)
    pred = torch.einsum("oc,vca->voa", weight[:, :, 1], xv[:, :, 1:1 + n])
    if loc is not None:
        pred = pred + loc.reshape(V, Oc, n).to(pred.dtype)
    scored, graph = scored_vertices(sizes, unscored_last)
    sidx, gidx = torch.tensor(scored, dtype=torch.long), torch.tensor(graph, dtype=torch.long)
    tgt = target.reshape(-1, Oc, n).to(pred.dtype)
    assert tgt.shape[0] == len(scored)
    if ties:
        pos = {v: i for i, v in enumerate(scored)}
        tgt = tgt.clone()
        for v, o in ties:
            tgt[pos[v], o] = pred.detach()[v, o]
    d = pred.index_select(0, sidx) - tgt
    sq = (d * d).sum(-1)                                                      # [scored, O]
    flat = sq.reshape(-1)
    nz = torch.nonzero(flat.detach() > 0).reshape(-1)
    nr = torch.zeros_like(flat).index_put((nz,), flat.index_select(0, nz).sqrt()).reshape(sq.shape)
    cnt = torch.bincount(gidx, minlength=B).clamp(min=1).to(pred.dtype)
    seg = lambda t: torch.zeros(B, dtype=pred.dtype).index_add(0, gidx, t)
    per_graph = torch.stack([seg(sq.sum(1)) / (cnt * Oc), seg(nr.sum(1)) / (cnt * Oc), seg(nr[:, Oc - 1]) / cnt], dim=1)
    per_vertex = torch.zeros(V, dtype=pred.dtype).index_put((sidx,), sq.sum(1) / (Oc * n))
    return pred, per_graph, per_vertex


def traj_reference(inp, dtype, use=("graph", "vertex"), ties=()):
    """{pred, per_graph, per_vertex, gx, gw} of one dtype; gradients of sum(per_graph g_graph) + sum(per_vertex g_vertex)
    restricted to the parts named in `use`."""
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    w = inp["weight"].to(dtype).clone().requires_grad_(True)
    pred, pg, pv = traj_forward(x, w, inp["loc"], inp["target"], inp["sizes"], inp["vrows"], inp["unscored_last"], inp["n"], ties)
    total = 0
    if "graph" in use:
        total = total + (pg * inp["g_graph"].to(dtype)).sum()
    if "vertex" in use:
        total = total + (pv * inp["g_vertex"].to(dtype)).sum()
    gx, gw = torch.autograd.grad(total, [x, w])
    return {"pred": pred.detach(), "per_graph": pg.detach(), "per_vertex": pv.detach(), "gx": gx, "gw": gw}


@functools.lru_cache(maxsize=None)
def traj_truth(tag, use=("graph", "vertex"), ties=()):
    """(float64 truth, float32 yardstick run) of a case, computed once."""
    inp = traj_inputs(tag)
    return traj_reference(inp, torch.float64, use, ties), traj_reference(inp, torch.float32, use, ties)


def traj_exact_zeros(inp, got):
    """The elements no arithmetic reaches must be 0 with ==: d/dx off the vector blades, on rows that are no vertex and on
    rows of unscored vertices; d/d weight outside grade 1; per_vertex of unscored vertices; per_graph of graphs without a
    scored vertex (empty or wholly unscored). `got` holds any of gx, gw, per_vertex, per_graph."""
    n, sizes = inp["n"], inp["sizes"]
    V = sum(sizes)
    scored, graph = scored_vertices(sizes, inp["unscored_last"])
    unscored = sorted(set(range(V)) - set(scored))
    rows = (lambda vs: vs) if inp["vrows"] is None else (lambda vs: inp["vrows"][vs].tolist())
    if "gx" in got:
        gx = got["gx"].cpu()
        assert bool((gx[:, :, 0] == 0).all()) and bool((gx[:, :, 1 + n:] == 0).all()), "d/dx off the vector blades"
        no_vertex = sorted(set(range(inp["n_rows"])) - set(rows(list(range(V)))))
        assert len(no_vertex) == inp["n_rows"] - V
        assert bool((gx[no_vertex] == 0).all()), "d/dx on rows that are no vertex"
        assert bool((gx[rows(unscored)] == 0).all()), "d/dx on rows of unscored vertices"
    if "gw" in got:
        gw = got["gw"].cpu()
        assert bool((gw[:, :, 0] == 0).all()) and bool((gw[:, :, 2:] == 0).all()), "d/d weight outside grade 1"
    if "per_vertex" in got:
        assert bool((got["per_vertex"].cpu()[unscored] == 0).all()), "per_vertex of unscored vertices"
    if "per_graph" in got:
        idle = sorted(set(range(len(sizes))) - set(graph))
        assert bool((got["per_graph"].cpu()[idle] == 0).all()), "per_graph of graphs without a scored vertex"


def compare(name, got, truth, ref32, keys=None, slack=4.0):
    """Every tensor of `got` (or `keys`) within the bound of DESIGN.md §2 of the truth; {tensor: (error, yardstick)}."""
    out = {}
    for k in (keys or sorted(got)):
        t64, t32 = truth[k].double().numpy(), ref32[k].double().numpy()
        g = got[k].detach().double().cpu().numpy()
        assert g.shape == t64.shape, (name, k, g.shape, t64.shape)
        assert np.isfinite(g).all(), f"{name}.{k}: not finite"
        out[k] = (check(f"{name}.{k}", g, t64, t32, slack), relmax(t32, t64))
    return out


# ======================================================================================================= MSE readout
# n, C, weight form ("3d": [1, C, n + 1], "2d": [1, C], weight_stride = 1), rows per graph, filler rows behind the last
# graph (a padded batch), bias
def _mse(n, C, form, sizes, filler, bias, seed):
    return dict(n=n, C=C, form=form, sizes=tuple(sizes), filler=filler, bias=bias, seed=seed)


MSE_CASES = {
    # the 256-stride loop runs 2 and 3 times; empty graphs in the middle and at the end
    "M1": _mse(5, 28, "3d", (84, 0, 257, 1, 600, 0), 5, True, 4201),
    # 2-D weight (stride 1), no bias; one full and one just-short stride
    "M2": _mse(3, 1, "2d", (256, 255), 0, False, 4202),
    # C D = 256: more than one 256-thread block of d/dx lies wholly behind ptr[B]
    "M3": _mse(2, 64, "3d", (1, 1, 1, 0), 300, True, 4203),
}


@functools.lru_cache(maxsize=None)
def mse_inputs(tag):
    c = MSE_CASES[tag]
    g = _gen(tag, c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)
    n, C, B = c["n"], c["C"], len(c["sizes"])
    S = sum(c["sizes"]) + c["filler"]
    weight = rn(1, C, n + 1) / C ** 0.5 if c["form"] == "3d" else rn(1, C) / C ** 0.5
    ptr = [0]
    for s in c["sizes"]:
        ptr.append(ptr[-1] + s)
    return dict(n=n, sizes=c["sizes"], x=rn(S, C, 1 << n), weight=weight, bias=rn(1, 1, 1) if c["bias"] else None,
                target=rn(B), wl=rn(B), ptr=torch.tensor(ptr, dtype=torch.int32))


def mse_forward(x, weight, bias, sizes, target):
    """(loss, pred) per graph: pred_g = mean over the rows s of g of (sum_c w[c] x[s, c, blade 0]) + b, 0 for an empty
    graph (global_mean_pool over no row; the bias is part of the rows' values); loss = (pred - target)^2
    (hulls_cssmpnn.py:93,155-164). The rows of a graph are contiguous from row 0; rows behind the last graph are in no mean."""
    w = weight[0, :, 0] if weight.dim() == 3 else weight[0]
    preds, lo = [], 0
    for s in sizes:
        if s == 0:
            preds.append(x.new_zeros(()))
        else:
            p = (x[lo:lo + s, :, 0] @ w).mean()
            preds.append(p + bias.reshape(()) if bias is not None else p)
        lo += s
    pred = torch.stack(preds)
    return (pred - target.to(pred.dtype)) ** 2, pred


def mse_reference(inp, dtype):
    """{loss, pred, gx, gw, gb (with a bias)} of one dtype; gradients of sum(wl loss)."""
    x = inp["x"].to(dtype).clone().requires_grad_(True)
    w = inp["weight"].to(dtype).clone().requires_grad_(True)
    b = None if inp["bias"] is None else inp["bias"].to(dtype).clone().requires_grad_(True)
    loss, pred = mse_forward(x, w, b, inp["sizes"], inp["target"])
    leaves = [x, w] + ([b] if b is not None else [])
    grads = torch.autograd.grad((loss * inp["wl"].to(dtype)).sum(), leaves)
    out = {"loss": loss.detach(), "pred": pred.detach(), "gx": grads[0], "gw": grads[1]}
    if b is not None:
        out["gb"] = grads[2]
    return out


@functools.lru_cache(maxsize=None)
def mse_truth(tag):
    inp = mse_inputs(tag)
    return mse_reference(inp, torch.float64), mse_reference(inp, torch.float32)


# =================================================================================================== type attributes
# n, T types, K features per type, S node rows, E edges, N entries of the type array (the nodes the edges may name; S
# where there are node rows). kTypeBins = 64 >= T K.
def _attr(n, T, K, S, E, seed, N=None):
    return dict(n=n, T=T, K=K, S=S, E=E, N=N or S, seed=seed)


ATTR_CASES = {
    "A1": _attr(3, 8, 8, 70, 500, 4301),           # 64 bins
    "A2": _attr(3, 64, 1, 300, 0, 4302),           # 64 bins, no edges (src = dst = NULL), 256 rows per pass
    "A3": _attr(2, 1, 64, 100, 1000, 4303),        # 4 rows per pass: 275 passes > 256 workgroups, a chunk spans two passes
    "A4": _attr(5, 9, 7, 0, 777, 4304, N=41),      # edges only; 36 rows per pass + 4 idle threads; 63 bins
    "A5": _attr(2, 3, 5, 52, 0, 4305),             # a row's K entries straddle a 256-thread block
}


@functools.lru_cache(maxsize=None)
def attr_inputs(tag, bad_ids=False):
    """table [T, K], types [N] int32, src / dst [E] int32 (None without edges), incoming gradients g_node [S, K, D] and
    g_edge [E, 2 K, D] (every blade random: only blade 0 may count), `base` = a pre-filled table gradient.
    bad_ids: ids of -2 and T + 4 sprinkled into the types (clamped into [0, T) by the kernels)."""
    c = ATTR_CASES[tag]
    g = _gen(tag, c["seed"])
    rn = lambda *s: torch.randn(*s, generator=g)
    T, K, S, E, N, D = c["T"], c["K"], c["S"], c["E"], c["N"], 1 << c["n"]
    types = torch.randint(0, T, (N,), generator=g, dtype=torch.int32)
    if bad_ids:
        types[torch.randperm(N, generator=g)[:6]] = -2
        types[torch.randperm(N, generator=g)[:6]] = T + 4
    src = torch.randint(0, N, (E,), generator=g, dtype=torch.int32) if E else None
    dst = torch.randint(0, N, (E,), generator=g, dtype=torch.int32) if E else None
    return dict(n=c["n"], T=T, K=K, S=S, E=E, D=D, table=rn(T, K), types=types, src=src, dst=dst, g_node=rn(S, K, D),
                g_edge=rn(E, 2 * K, D), base=rn(T, K))


def attr_forward(inp):
    """(node_attr [S, K, D], edge_attr [E, 2 K, D]): blade 0 = the table row of the node's type / of the types of the
    edge's source (first K) and target (last K); every other blade 0 (md17_cssmpnn.py:122-133). Ids clamped into [0, T)."""
    T, K, S, E, D = inp["T"], inp["K"], inp["S"], inp["E"], inp["D"]
    ty = inp["types"].long().clamp(0, T - 1)
    node, edge = torch.zeros(S, K, D), torch.zeros(E, 2 * K, D)
    node[:, :, 0] = inp["table"][ty[:S]]
    if E:
        edge[:, :K, 0] = inp["table"][ty[inp["src"].long()]]
        edge[:, K:, 0] = inp["table"][ty[inp["dst"].long()]]
    return node, edge


def attr_backward(inp, dtype, use=("node", "edge"), rows=None):
    """g_table [T, K]: index_add of the blade-0 gradients of the rows that read the entry. rows = (lo, hi): only the rows
    lo <= r < hi of the list (node rows, then edges) contribute."""
    T, K, S, E = inp["T"], inp["K"], inp["S"], inp["E"]
    ty = inp["types"].long().clamp(0, T - 1)
    lo, hi = rows if rows is not None else (0, S + E)
    g = torch.zeros(T, K, dtype=dtype)
    if "node" in use and S:
        a, b = min(lo, S), min(hi, S)
        g.index_add_(0, ty[a:b], inp["g_node"][a:b, :, 0].to(dtype))
    if "edge" in use and E:
        a, b = max(lo - S, 0), max(hi - S, 0)
        g.index_add_(0, ty[inp["src"].long()[a:b]], inp["g_edge"][a:b, :K, 0].to(dtype))
        g.index_add_(0, ty[inp["dst"].long()[a:b]], inp["g_edge"][a:b, K:, 0].to(dtype))
    return g


def attr_det_chunk_rows(rows, K):
    """Rows of one workgroup of csmpn_type_attr_backward_det (glue.hip: 256 / K rows per pass, at most 256 partial rows,
    whole passes per workgroup; `chunk size and workgroup count follow from the call's sizes alone`)."""
    rpp = 256 // K
    passes = -(-rows // rpp)
    return -(-passes // min(passes, 256)) * rpp


# ====================================================================================================== simplex rows
# n, feature blocks (channels, grade), vertices per row, rows, feature rows S, ids forced out of range
def _rows(n, blocks, vpr, rows, S, seed, outside=0):
    return dict(n=n, blocks=tuple(blocks), vpr=vpr, rows=rows, S=S, seed=seed, outside=outside)


ROWS_CASES = {
    "R1": _rows(5, ((1, 1), (2, 0), (1, 2), (1, 5)), 3, 37, 11, 4401),     # four blocks (kMaxVertexBlocks), grades 2 and n
    "R2": _rows(3, ((3, 1), (2, 0)), 1, 1, 4, 4402),                       # the smallest call
    "R3": _rows(2, ((5, 2),), 5, 257, 9, 4403, outside=12),                # a few ids of -1 and S: feature row 0
    "R4": _rows(4, ((1, 3), (1, 4)), 2, 64, 6, 4404),                      # n = 4
}


@functools.lru_cache(maxsize=None)
def rows_inputs(tag):
    import math
    c = ROWS_CASES[tag]
    g = _gen(tag, c["seed"])
    feats = [torch.randn(c["S"], k, math.comb(c["n"], gr), generator=g) for k, gr in c["blocks"]]
    verts = torch.randint(0, c["S"], (c["rows"], c["vpr"]), generator=g, dtype=torch.int64)
    if c["outside"]:
        at = torch.randperm(verts.numel(), generator=g)[:c["outside"]]
        verts.view(-1)[at[::2]] = -1
        verts.view(-1)[at[1::2]] = c["S"]
    return dict(n=c["n"], feats=feats, grades=[gr for _, gr in c["blocks"]], verts=verts, S=c["S"])


def rows_reference(inp):
    """out [rows, sum_b vpr K_b, D]: per block the features of the row's vertices, vertex after vertex, embedded at the
    block's grade (algebra.embed_grade), the blocks concatenated along the channels (hulls_cssmpnn.py:96-125,
    md17_cssmpnn.py:85-120). An id outside [0, S) reads feature row 0, as the kernel documents."""
    alg = algebra(inp["n"], torch.float32)
    v = inp["verts"]
    ids = torch.where((v < 0) | (v >= inp["S"]), torch.zeros_like(v), v)
    parts = []
    for f, grade in zip(inp["feats"], inp["grades"]):
        g = f[ids]                                                     # [rows, vpr, K, n_g]
        parts.append(O.embed_grade(alg, g.reshape(g.shape[0], -1, g.shape[-1]), grade))
    return torch.cat(parts, dim=1)
