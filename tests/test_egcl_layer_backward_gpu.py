"""GPU: csmpn_egcl_backward, the one C-ABI call for both backwards of an EGCL layer (HipBackend.layer_backward, taken by
_EgclFn.backward whenever the adjacency is whole and no deterministic request is active). On the Cl(3,0) 8-channel kernels the
node program's slice sum is deferred into one launch behind the edge backward that sums both programs' slices.

Shape: Cl(3,0), 8 channels, 6 edge- and 3 node-attribute channels, 37 nodes and 203 edges - neither a multiple of the 8 rows
of a wave tile, so the last tile of both programs is masked; node 36 has no incoming edge, node 11 more than 16, so its target
segment spans row tiles. aggr mean and sum, with and without attribute gradients.

The library reads its environment switches once per process, so every environment has ONE child process (as
tests/general_helpers.py) that runs all its cases and saves their tensors; the comparisons are made here:
  * default: one tile per wave (the hand-over between the blocks stays in registers);
  * CSMPN_CL_CAP_FWD=2 CSMPN_CL_CAP_BWD=2: two workgroups, every wave of the edge program walks several tiles (26 tiles on 8
    waves), the hand-over between its blocks goes through memory;
  * CSMPN_SAVE_STATE=0: the recomputing backward.
The default child also runs Cl(3,0) at 5 channels, which no lane family serves: the entry then runs the two stages on the
general kernels.

Per case: (a) the layer through autograd against the float64 oracle, bound max(1e-5, 4 x the float32 oracle's own error), the
`check` of tests/test_hip_parity.py; (b) the new entry against the two separate entries on the SAME forward state: parameter
gradients and attribute gradients torch.equal on the lane kernels; d/dh torch.equal on the rows that receive at most one
float atomic and within 1e-5 on the others (below); (c) fused accumulation into p.grad: two backward passes through one
forward leave exactly twice what one leaves (x + x is exact in binary floating point).

d/dh and bit equality. The edge backward adds its +-d/d(h_i - h_j) rows into gh with float atomics, in an order that differs
from launch to launch, so the rows of gh that take two or more atomics are not bit-reproducible between ANY two runs, the two
separate entry points run twice included (measured on this shape: merged against separate 1.13e-07 of max|gh|; the child
also runs the separate entries a second time and the test prints that difference beside it). What can be bit-equal is: the
node stage's part of gh, and what one atomic adds to it (a + x has one order). Node 36 has no edge at all and node 35
exactly one (incoming): on those rows d/dh must be torch.equal; on the others the two results are two float32 evaluations
of the same sum in another order, held to the suite's floor of 1e-5 of max|gh|.
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_path as O
from test_hip_parity import TOL, check, relmax

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "clifford-group-equivariant-simplicial-message-passing-networks_amd"
METRIC = (1.0, 1.0, 1.0)
N, E, EA, NA = 37, 203, 6, 3
HUB, ISOLATED, LEAF = 11, N - 1, N - 2

#  case: (channels, aggr, attribute gradients)
CASES = {
    "mean": (8, "mean", False), "mean-attr": (8, "mean", True), "sum": (8, "sum", False), "sum-attr": (8, "sum", True),
    "general5": (5, "mean", True),
}
LANE = ["mean", "mean-attr", "sum", "sum-attr"]
#  environment: (switches beside CSMPN_DEBUG=1, its cases)
ENVS = {
    "one-tile": ({}, LANE + ["general5"]),
    "capped": ({"CSMPN_CL_CAP_FWD": "2", "CSMPN_CL_CAP_BWD": "2"}, LANE),
    "recompute": ({"CSMPN_SAVE_STATE": "0"}, ["mean-attr", "sum"]),
}
PAIRS = [(env, case) for env, (_, cases) in ENVS.items() for case in cases]


def inputs(case):
    C = CASES[case][0]
    o32 = O.Algebra(list(METRIC), torch.float32)
    h, ei, ea, na = O.synthetic_complex(o32, N, E, C, seed=71)
    ei = ei.clone()
    ei[1][ei[1] == ISOLATED] = 3       # the last node: no edge at all
    ei[0][ei[0] == ISOLATED] = 2
    ei[1][ei[1] == LEAF] = 4           # the one in front of it: one incoming edge, none going out
    ei[0][ei[0] == LEAF] = 5
    ei[1, 0] = LEAF
    ei[1, 40:60] = HUB                 # ... and 20 more edges at the hub: more than two 8-row tiles of one target
    gen = torch.Generator().manual_seed(72)
    p = O.init_egcl_params(o32, C, C, C, EA, NA, gen=gen, randomize=True)
    gout = torch.randn(N, C, 8, generator=gen)
    return h, ei, ea, na, p, gout


def test_inputs_have_an_isolated_node_and_a_hub():
    _, ei, _, _, _, _ = inputs("mean")
    deg = torch.bincount(ei[1], minlength=N)
    assert deg[ISOLATED] == 0 and deg[HUB] > 16 and N % 8 and E % 8
    assert one_atomic_rows(ei).tolist() == [LEAF, ISOLATED]


def one_atomic_rows(ei):
    """Nodes whose d/dh row takes at most one atomic add of the edge backward (one per edge end at the most)."""
    return torch.nonzero(torch.bincount(ei[0], minlength=N) + torch.bincount(ei[1], minlength=N) <= 1).flatten()


# ------------------------------------------------------------------------------------------------------------ the child
def _layer(pkg, case, p, dev):
    C, aggr, _ = CASES[case]
    layer = pkg.EGCL(pkg.CliffordAlgebra(METRIC), C, C, C, edge_attr_features=EA, node_attr_features=NA, aggr=aggr)
    sd = layer.state_dict()
    sd.update(p)
    layer.load_state_dict(sd, strict=True)
    return layer.to(dev)


def child_case(pkg, case):
    """Everything of one case that needs the GPU; CPU tensors back."""
    from csmpn_hip import ops
    dev = torch.device("cuda:0")
    _, aggr, attr_grad = CASES[case]
    h, ei, ea, na, p, gout = inputs(case)
    cpu = lambda t: None if t is None else t.detach().cpu()
    res = {}
    # (a) the layer through autograd
    layer = _layer(pkg, case, p, dev)
    hd = h.to(dev).requires_grad_(True)
    ead, nad = ea.to(dev).requires_grad_(attr_grad), na.to(dev).requires_grad_(attr_grad)
    y = layer(hd, ei.to(dev), ead, nad)
    (y * gout.to(dev)).sum().backward()
    auto = {"y": cpu(y), "gh": cpu(hd.grad)}
    if attr_grad:
        auto["g_edge_attr"], auto["g_node_attr"] = cpu(ead.grad), cpu(nad.grad)
    auto.update({"g." + k: cpu(v.grad) for k, v in layer.named_parameters()})
    res["auto"] = auto
    # (b) one forward state, both ways through the backward
    be, spec = ops.HipBackend, layer.spec()
    csr = ops.get_csr(ei.to(dev), N)
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    hh, gd = h.to(dev), gout.to(dev)
    agg, st_e = be.edge_forward(spec, csr, hh, ead.detach(), pe)
    _, st_n = be.node_forward(spec, csr.deg, hh, agg, nad.detach(), pn)
    gh, g_agg, g_na, views_n = be.node_backward(spec, csr.deg, hh, agg, nad.detach(), pn, gd, attr_grad, st_n)
    g_ea, views_e = be.edge_backward(spec, csr, hh, ead.detach(), pe, g_agg, gh, attr_grad, st_e)
    res["separate"] = dict(gh=cpu(gh), g_edge_attr=cpu(g_ea), g_node_attr=cpu(g_na),
                           params=[cpu(v) for v in list(views_e) + list(views_n)])
    gh2, g_agg, _, _ = be.node_backward(spec, csr.deg, hh, agg, nad.detach(), pn, gd, attr_grad, st_n)
    be.edge_backward(spec, csr, hh, ead.detach(), pe, g_agg, gh2, attr_grad, st_e)
    res["separate_again_gh"] = cpu(gh2)
    gh, g_ea, g_na, views_e, views_n = be.layer_backward(spec, csr, hh, agg, ead.detach(), nad.detach(), pe, pn, gd, attr_grad,
                                                         attr_grad, st_e, st_n)
    res["merged"] = dict(gh=cpu(gh), g_edge_attr=cpu(g_ea), g_node_attr=cpu(g_na),
                         params=[cpu(v) for v in list(views_e) + list(views_n)])
    # (c) fused accumulation: one forward, two backward passes into the zeroed p.grad
    ops.set_fused_grad_accumulation(True)
    try:
        for prm in layer.parameters():
            prm.grad.zero_()
        y = layer(h.to(dev).requires_grad_(True), ei.to(dev), ea.to(dev), na.to(dev))
        y.backward(gout.to(dev), retain_graph=True)
        res["fused1"] = [cpu(prm.grad).clone() for prm in layer.parameters()]
        y.backward(gout.to(dev))
        res["fused2"] = [cpu(prm.grad) for prm in layer.parameters()]
    finally:
        ops.set_fused_grad_accumulation(False)
    torch.cuda.synchronize()
    return res


_BEGIN, _END = "[case] begin ", "[case] end "
_CHILD = r"""
import importlib, os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_egcl_layer_backward_gpu as T
pkg = importlib.import_module(T.PKG)
out = {}
for case in sys.argv[3:]:
    os.write(2, (T._BEGIN + case + "\n").encode())
    out[case] = T.child_case(pkg, case)
    os.write(2, (T._END + case + "\n").encode())
torch.save(out, sys.argv[2])
"""
_children = {}
_ended_badly = []    # an environment whose child did not end cleanly: nothing more is started on the GPU after that


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("layer_backward")


def run_env(env, workdir):
    """{case: (tensors, the library's dispatch lines)} of one environment, from one child process."""
    if env in _children:
        return _children[env]
    assert not _ended_badly, f"not started: the child of {_ended_badly[0]} did not end cleanly"
    switches, cases = ENVS[env]
    f = str(workdir / f"{env}.pt")
    clean = {k: v for k, v in os.environ.items() if k not in ("CSMPN_CL_CAP_FWD", "CSMPN_CL_CAP_BWD", "CSMPN_SAVE_STATE")}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, f] + cases, env=dict(clean, CSMPN_DEBUG="1", **switches),
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    if r.returncode != 0:
        _ended_badly.append(env)
    assert r.returncode == 0, f"child of {env} ended with {r.returncode}:\n{r.stderr[-4000:]}"
    logs, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith(_BEGIN):
            cur = line[len(_BEGIN):].strip()
            logs[cur] = []
        elif line.startswith(_END):
            cur = None
        elif cur is not None and line.startswith("[csmpn]"):
            logs[cur].append(line)
    tensors = torch.load(f)
    _children[env] = {case: (tensors[case], logs[case]) for case in cases}
    return _children[env]


# -------------------------------------------------------------------------------------------------------- the reference
_oracle = {}


def oracle(case):
    """(float64 truth, float32 yardstick run) of a case, computed once."""
    if case not in _oracle:
        _, aggr, attr_grad = CASES[case]
        h, ei, ea, na, p, gout = inputs(case)
        runs = []
        for dtype in (torch.float64, torch.float32):
            leaf = lambda t, rg=True: t.detach().to(dtype).clone().requires_grad_(rg)
            q = {k: leaf(v) for k, v in p.items()}
            hh, ee, nn = leaf(h), leaf(ea, attr_grad), leaf(na, attr_grad)
            y = O.egcl(O.Algebra(list(METRIC), dtype), hh, ei, ee, nn, q, aggr=aggr, residual=True)
            (y * gout.to(dtype)).sum().backward()
            out = {"y": y.detach(), "gh": hh.grad}
            if attr_grad:
                out["g_edge_attr"], out["g_node_attr"] = ee.grad, nn.grad
            out.update({"g." + k: v.grad for k, v in q.items()})
            runs.append({k: v.numpy() for k, v in out.items()})
        _oracle[case] = tuple(runs)
    return _oracle[case]


# ------------------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("env,case", PAIRS)
def test_layer_against_the_float64_oracle(env, case, workdir):
    (res, log) = run_env(env, workdir)[case]
    t64, t32 = oracle(case)
    got = res["auto"]
    assert set(got) == set(t64) and len([k for k in got if k.startswith("g.")]) == 40
    worst = 0.0
    for k in sorted(got):
        err, yard = relmax(got[k].numpy(), t64[k]), relmax(t32[k], t64[k])
        print(f"{env} {case} {k}: err {err:.2e}, float32 yardstick {yard:.2e}")
        worst = max(worst, err / max(TOL, 4.0 * yard))
    print(f"{env} {case}: worst err / bound {worst:.2f}")
    for k in sorted(got):
        check(f"{env} {case} {k}", got[k].numpy(), t64[k], t32[k], slack=4.0)
    # the kernels the case is about ran, at the grid the environment asks for
    lane = CASES[case][0] == 8
    for mode, rows in ((2, N), (1, E)):
        lines = [l for l in log if l.startswith(f"[csmpn] cl mode={mode} bwd=1 ")]
        assert bool(lines) == lane, log
        if lane:
            grid = 2 if env == "capped" else (rows + 31) // 32
            assert all(f" grid={grid} rows={rows}" in l for l in lines), lines


@pytest.mark.parametrize("env,case", PAIRS)
def test_one_call_equals_the_two_stage_calls(env, case, workdir):
    (res, _) = run_env(env, workdir)[case]
    sep, new = res["separate"], res["merged"]
    attr_grad = CASES[case][2]
    assert (sep["g_edge_attr"] is not None) == (new["g_edge_attr"] is not None) == attr_grad
    assert (sep["g_node_attr"] is not None) == (new["g_node_attr"] is not None) == attr_grad
    assert len(sep["params"]) == len(new["params"]) == 40
    named = [(f"param {i}", a, b) for i, (a, b) in enumerate(zip(new["params"], sep["params"]))]
    named += [(k, new[k], sep[k]) for k in ("g_edge_attr", "g_node_attr") if sep[k] is not None]
    exact = one_atomic_rows(inputs(case)[1])
    print(f"{env} {case} gh: merged against separate {relmax(new['gh'].numpy(), sep['gh'].numpy()):.2e}, separate against "
          f"separate run again {relmax(res['separate_again_gh'].numpy(), sep['gh'].numpy()):.2e}")
    named.append(("gh, rows of at most one atomic", new["gh"][exact], sep["gh"][exact]))
    for name, a, b in named:
        diff = relmax(a.numpy(), b.numpy()) if float(b.abs().max()) > 0 else float(a.abs().max())
        print(f"{env} {case} {name}: merged against separate {diff:.2e}")
    for name, a, b in named:
        if CASES[case][0] == 8:
            assert torch.equal(a, b), (env, case, name)
        else:
            # the general kernels: the same launches in the same order either way, what may differ is the order of float
            # atomics - the suite's floor for one float32 evaluation against another
            assert relmax(a.numpy(), b.numpy()) <= TOL, (env, case, name)
    assert relmax(new["gh"].numpy(), sep["gh"].numpy()) <= TOL, (env, case)


@pytest.mark.parametrize("env,case", PAIRS)
def test_fused_accumulation_twice_is_twice(env, case, workdir):
    (res, _) = run_env(env, workdir)[case]
    t64, t32 = oracle(case)
    names = [k for k in res["auto"] if k.startswith("g.")]   # named_parameters order, as layer.parameters()
    assert len(names) == len(res["fused1"]) == len(res["fused2"]) == 40
    for k, g1, g2 in zip(names, res["fused1"], res["fused2"]):
        check(f"{env} {case} fused {k}", g1.numpy(), t64[k], t32[k], slack=4.0)
        if CASES[case][0] == 8:
            assert torch.equal(g2, 2.0 * g1), (env, case, k)
        else:
            assert relmax(g2.numpy(), (2.0 * g1).numpy()) <= TOL, (env, case, k)
