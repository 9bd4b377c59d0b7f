"""GPU: addressing and tail handling of the (row, channel)-per-lane kernels (cemlp_cl.hpp). They address every array of a
launch through a buffer resource with a 32-bit byte offset, and the rows behind the last one of a partial tile rely on the
hardware's range check: their stores are dropped, their loads read zero. A wrong offset or a wrong array size therefore shows
as a wrong value - or as a store in front of or behind an array.

Layer: Cl(3,0), 8 channels, 6 edge- and 3 node-attribute channels, randomized parameters, mean aggregation, residual; the four
stages (edge forward, node forward, node backward, edge backward) through the C-ABI on buffers of the test's own.
Shapes, the smallest at which addressing or tail handling can go wrong (a tile is 8 rows):
  * edge rows 1, 7, 8, 9 and, with the grid capped to one workgroup (CSMPN_CL_CAP_FWD = CSMPN_CL_CAP_BWD = 1, a child process
    of its own), 67: a wave walks three tiles there and the last one is partial;
  * node rows 1, 5, 8, 9;
  * 5 and 9 nodes under the "hub" adjacency: an isolated node, a self-loop, a duplicated edge and every edge pointing at the
    LAST node - the highest row offset of the node tables and a repeated scatter target in one tile.
Variants: default (atomic scatter) and CSMPN_FLAG_DETERMINISTIC (row tables + segmented sums), each with the save-state and
with the recompute instantiation of the backward.

Checks: (a) layer output, d/dh and every parameter gradient by name against the float64 oracle, `check` of
tests/test_hip_parity.py: max(1e-5, 4 x the float32 oracle's own error); (b) deterministic variants: two runs are torch.equal
in every tensor; (c) a guard row of sentinels in front of and behind every output, row table and saved buffer is untouched.
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_path as O
from test_hip_parity import check, relmax
import test_egcl_layer_backward_gpu as L

pytestmark = pytest.mark.gpu

ROOT, PKG, METRIC = L.ROOT, L.PKG, L.METRIC
C, EA, NA, D = 8, 6, 3, 8
SENTINEL = -12345.0
GUARD = C * D    # floats of one guard row


def hub(n):
    """every edge points at node n - 1: a duplicated edge, a self-loop, node 1 isolated"""
    src = [0, 0, n - 1] + list(range(2, n - 3))
    return torch.tensor([src, [n - 1] * len(src)], dtype=torch.long)


# name -> (nodes, edges or an adjacency, grid cap)
SHAPES = {
    "n5-e1": (5, torch.tensor([[0], [4]]), None),
    "n5-hub": (5, hub(5), None),
    "n9-hub": (9, hub(9), None),
    "n1-e8": (1, torch.zeros(2, 8, dtype=torch.long), None),
    "n8-e9": (8, 9, None),
    "n13-e67-cap1": (13, 67, 1),
}
VARIANTS = {"atomic-state": (False, True), "atomic-recompute": (False, False), "det-state": (True, True), "det-recompute": (True, False)}
PAIRS = [(s, v) for s in SHAPES for v in VARIANTS]
_SWITCHES = ("CSMPN_CL_CAP_FWD", "CSMPN_CL_CAP_BWD", "CSMPN_SAVE_STATE", "CSMPN_NO_CL", "CSMPN_DETERMINISTIC")


def inputs(shape):
    N, adj, _ = SHAPES[shape]
    o32 = O.Algebra(list(METRIC), torch.float32)
    seed = 900 + list(SHAPES).index(shape)
    E = adj if isinstance(adj, int) else adj.shape[1]
    h, ei, _, na = O.synthetic_complex(o32, N, max(E, 1), C, seed=seed)
    if not isinstance(adj, int):
        ei = adj
    ei = ei[:, :E].contiguous()
    ea = torch.cat([na[ei[0]], na[ei[1]]], dim=1).contiguous()
    gen = torch.Generator().manual_seed(seed + 50)
    p = O.init_egcl_params(o32, C, C, C, EA, NA, gen=gen, randomize=True)
    gout = torch.randn(N, C, D, generator=gen)
    return h, ei, ea, na, p, gout


def test_shapes():
    rows = {s: (SHAPES[s][0], inputs(s)[1].shape[1]) for s in SHAPES}
    assert sorted(e for _, e in rows.values()) == [1, 3, 7, 8, 9, 67]
    assert {n for n, _ in rows.values()} >= {1, 5, 8, 9}
    for s in ("n5-hub", "n9-hub"):
        N, ei = SHAPES[s][0], SHAPES[s][1]
        assert bool((ei[1] == N - 1).all()) and 1 not in ei and [0, N - 1] in ei.t().tolist() and [N - 1, N - 1] in ei.t().tolist()
        assert ei.t().tolist().count([0, N - 1]) == 2
    assert (67 + 7) // 8 == 9 and 67 % 8 == 3    # cap 1: four waves, nine tiles: wave 0 walks three, the last has 3 rows


# ------------------------------------------------------------------------------------------------------------ the child
class Guarded:
    """`rows` rows of `row_floats` floats between two guard rows of sentinels"""

    def __init__(self, rows, row_floats, dev, fill=None, total_floats=None):
        n = rows * row_floats if total_floats is None else total_floats
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        self.body = self.full[GUARD:GUARD + n]
        if fill is not None:
            self.body.fill_(fill)
        self.view = self.body.view(rows, -1, D) if total_floats is None else self.body

    def intact(self):
        g = torch.cat([self.full[:GUARD], self.full[GUARD + self.n:]])
        return bool((g == SENTINEL).all())


def run_layer(pkg, shape, det, state):
    """the four stages of one layer through the C-ABI; CPU tensors and the guards' verdicts back"""
    from csmpn_hip import native, ops
    lib = native.lib()
    dev = torch.device("cuda:0")
    h, ei, ea, na, p, gout = inputs(shape)
    N, E = h.shape[0], ei.shape[1]
    layer = pkg.EGCL(pkg.CliffordAlgebra(METRIC), C, C, C, edge_attr_features=EA, node_attr_features=NA, aggr="mean")
    sd = layer.state_dict()
    sd.update(p)
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(dev)
    names = {id(prm): k for k, prm in layer.named_parameters()}
    spec, csr = layer.spec(), ops.get_csr(ei.to(dev), N)
    e, nd = spec.edge, spec.node
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    e.bind(pe)
    nd.bind(pn)
    hh, ead, nad, gd = h.to(dev), ea.to(dev), na.to(dev), gout.to(dev)
    fl_state = native.FLAG_SAVE_STATE if state else 0
    fl_det = native.FLAG_DETERMINISTIC if det else 0
    st = ops._stream(dev)
    guards = {}

    def guarded(name, *a, **k):
        guards[name] = Guarded(*a, **k)
        return guards[name]

    saved_e = guarded("saved_e", 0, 0, dev, total_floats=int(lib.csmpn_cemlp_saved_floats(e.n, e.params, e.nblk, E, fl_state)))
    saved_n = guarded("saved_n", 0, 0, dev, total_floats=int(lib.csmpn_cemlp_saved_floats(nd.n, nd.params, nd.nblk, N, fl_state)))
    ws_e, ws_n = e.workspace(dev), nd.workspace(dev)
    # edge forward
    agg = guarded("agg", N, C * D, dev, fill=0.0)
    msg = guarded("msg_rows", E, C * D, dev) if det else None
    native.check(lib.csmpn_egcl_edge_forward(
        e.metric_arr, e.n, e.params, e.nblk, hh.data_ptr(), spec.C, ead.data_ptr(), spec.A, csr.perm.data_ptr(), csr.src.data_ptr(),
        csr.dst.data_ptr(), E, N, (msg if det else agg).body.data_ptr(), saved_e.body.data_ptr(), ws_e.data_ptr(), ws_e.numel(),
        fl_det | fl_state, st))
    if det:
        ops.segment_reduce(msg.view, agg.view, add=(csr.row_ptr, None))
    # node forward
    out = guarded("out", N, C * D, dev)
    native.check(lib.csmpn_egcl_node_forward(
        nd.metric_arr, nd.n, nd.params, nd.nblk, hh.data_ptr(), spec.C, agg.body.data_ptr(), spec.O, nad.data_ptr(), spec.T,
        csr.deg.data_ptr(), spec.mean, spec.residual, N, out.body.data_ptr(), saved_n.body.data_ptr(), ws_n.data_ptr(), ws_n.numel(),
        fl_det | fl_state, st))
    # node backward
    _, views_n = nd.new_grads(pn, dev)
    gh, g_agg, g_na = guarded("gh", N, C * D, dev), guarded("g_agg", N, C * D, dev), guarded("g_na", N, NA * D, dev)
    native.check(lib.csmpn_egcl_node_backward(
        nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, hh.data_ptr(), spec.C, agg.body.data_ptr(), spec.O, nad.data_ptr(), spec.T,
        csr.deg.data_ptr(), spec.mean, spec.residual, N, gd.data_ptr(), gh.body.data_ptr(), g_agg.body.data_ptr(), g_na.body.data_ptr(),
        saved_n.body.data_ptr(), ws_n.data_ptr(), ws_n.numel(), native.FLAG_WEIGHTS_PACKED | fl_det | fl_state, st))
    # edge backward: gh += the scatter of +- d/d(h_i - h_j)
    _, views_e = e.new_grads(pe, dev)
    g_ea = guarded("g_ea", E, EA * D, dev)
    grow = guarded("gh_rows", E, C * D, dev) if det else None
    native.check(lib.csmpn_egcl_edge_backward(
        e.metric_arr, e.n, e.params, e.grads, e.nblk, hh.data_ptr(), spec.C, ead.data_ptr(), spec.A, csr.perm.data_ptr(),
        csr.src.data_ptr(), csr.dst.data_ptr(), E, N, g_agg.body.data_ptr(), (grow if det else gh).body.data_ptr(), g_ea.body.data_ptr(),
        saved_e.body.data_ptr(), ws_e.data_ptr(), ws_e.numel(), native.FLAG_WEIGHTS_PACKED | fl_det | fl_state, st))
    if det:
        ops.segment_reduce(grow.view, gh.view, add=(csr.row_ptr, None), sub=csr.source_order())
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu().clone()
    res = {"y": cpu(out.view), "gh": cpu(gh.view), "g_ea": cpu(g_ea.view), "g_na": cpu(g_na.view)}
    for prm, v in list(zip(pe, views_e)) + list(zip(pn, views_n)):
        if prm is not None:
            res["g." + names[id(prm)]] = cpu(v)
    return res, {k: g.intact() for k, g in guards.items()}


def child_cases(pkg, shapes):
    out = {}
    for s in shapes:
        for v, (det, state) in VARIANTS.items():
            runs = [run_layer(pkg, s, det, state) for _ in range(2 if det else 1)]
            out[(s, v)] = runs
    return out


_CHILD = r"""
import importlib, os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_cl_addressing_gpu as T
pkg = importlib.import_module(T.PKG)
torch.save(T.child_cases(pkg, sys.argv[3].split(",")), sys.argv[2])
"""
_children = {}
_ended_badly = []    # a child that did not end cleanly: nothing more is started on the GPU after that


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("cl_addressing")


def run_cap(cap, workdir):
    """{(shape, variant): runs} of the shapes with this grid cap, from one child process (the library reads its switches once)"""
    if cap in _children:
        return _children[cap]
    assert not _ended_badly, f"not started: the child of cap {_ended_badly[0]} did not end cleanly"
    f = str(workdir / f"cap{cap}.pt")
    shapes = [s for s in SHAPES if SHAPES[s][2] == cap]
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    if cap is not None:
        env.update(CSMPN_CL_CAP_FWD=str(cap), CSMPN_CL_CAP_BWD=str(cap))
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, f, ",".join(shapes)], env=dict(env, CSMPN_DEBUG="1"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    if r.returncode != 0:
        _ended_badly.append(cap)
    assert r.returncode == 0, f"child of cap {cap} ended with {r.returncode}:\n{r.stderr[-4000:]}"
    # the kernels the test is about served every stage (no other family, no general kernel)
    lines = [l for l in r.stderr.splitlines() if l.startswith("[csmpn] ") and " mode=" in l]
    assert lines and all(l.startswith("[csmpn] cl mode=") for l in lines), lines[:8]
    if cap is not None:
        assert all(f" grid={cap} " in l for l in lines), lines[:8]
    _children[cap] = torch.load(f)
    return _children[cap]


# -------------------------------------------------------------------------------------------------------- the reference
_oracle = {}


def oracle(shape):
    """(float64 truth, float32 yardstick run), computed once per shape"""
    if shape not in _oracle:
        h, ei, ea, na, p, gout = inputs(shape)
        runs = []
        for dtype in (torch.float64, torch.float32):
            q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
            hh = h.detach().to(dtype).clone().requires_grad_(True)
            ee, nn_ = ea.to(dtype).clone().requires_grad_(True), na.to(dtype).clone().requires_grad_(True)
            y = O.egcl(O.Algebra(list(METRIC), dtype), hh, ei, ee, nn_, q, aggr="mean", residual=True)
            (y * gout.to(dtype)).sum().backward()
            out = {"y": y.detach(), "gh": hh.grad, "g_ea": ee.grad, "g_na": nn_.grad}
            out.update({"g." + k: v.grad for k, v in q.items()})
            runs.append({k: v.numpy() for k, v in out.items()})
        _oracle[shape] = tuple(runs)
    return _oracle[shape]


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("shape,variant", PAIRS)
def test_against_the_float64_oracle(shape, variant, workdir):
    res, _ = run_cap(SHAPES[shape][2], workdir)[(shape, variant)][0]
    t64, t32 = oracle(shape)
    assert set(res) == set(t64) and len([k for k in res if k.startswith("g.")]) == 40
    for k in sorted(res):
        print(f"{shape} {variant} {k}: err {relmax(res[k].numpy(), t64[k]):.2e}, float32 yardstick {relmax(t32[k], t64[k]):.2e}")
    for k in sorted(res):
        check(f"{shape} {variant} {k}", res[k].numpy(), t64[k], t32[k], slack=4.0)


@pytest.mark.parametrize("shape,variant", PAIRS)
def test_nothing_stored_outside_the_arrays(shape, variant, workdir):
    for _, intact in run_cap(SHAPES[shape][2], workdir)[(shape, variant)]:
        assert all(intact.values()), (shape, variant, [k for k, ok in intact.items() if not ok])


@pytest.mark.parametrize("shape,variant", [(s, v) for s, v in PAIRS if VARIANTS[v][0]])
def test_deterministic_runs_are_bit_equal(shape, variant, workdir):
    (a, _), (b, _) = run_cap(SHAPES[shape][2], workdir)[(shape, variant)]
    assert set(a) == set(b)
    for k in sorted(a):
        assert torch.equal(a[k], b[k]), (shape, variant, k, relmax(a[k].numpy(), b[k].numpy()))
