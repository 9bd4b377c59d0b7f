"""GPU: the end phase of the (row, channel)-per-lane backward (cemlp_cl.hpp, cl_bwd_block). Once per block a workgroup turns
what its waves summed over their tiles into one slice of partial sums: the weight-gradient MFMA tiles through per-wave images
that are added in wave order, the per-channel parameter gradients (0.bias, 1.a, 1.b, 2.weight, 2.normalization.a,
2.linear_left.bias, 3.a) by owner threads that add the 32 lane-private LDS sums of a channel - 4 waves x 8 rows - whoever
wrote them. So a wave without a tile and the rows behind the last valid one must have left exact zeros there, in both blocks.

Layer: Cl(3,0), 8 channels, 6 edge- and 3 node-attribute channels, randomized parameters, aggr mean and sum. Sizes:
  * "small": 13 nodes, 37 edges. The node launch has two tiles: waves 2 and 3 of its only workgroup have none, the last tile
    has 5 valid rows. The edge launch has 5 tiles: its second workgroup has one busy wave, with a 5-row tile.
  * "hub": the 37 nodes and 203 edges of tests/test_egcl_layer_backward_gpu.py, with its hub and its isolated node.
Environments (one child process each: the library reads its switches once per process): default (one tile per wave),
CSMPN_CL_CAP_FWD = CSMPN_CL_CAP_BWD = 1 (one workgroup walks every tile), the same with 2, CSMPN_SAVE_STATE=0.

Checks: (a) layer output, d/dh and every parameter gradient by name against the float64 oracle, `check` of
tests/test_hip_parity.py, bound max(1e-5, 4 x the float32 oracle's own error); (b) two backward passes on one forward state give
torch.equal parameter gradients; (c) d/d(out) all zero: every parameter gradient is exactly 0.0; (d) d/d(out) non-zero only on
the rows of the last, partial node tile: parameter gradients still meet (a); (e) cap 1, cap 2 and default agree on every
parameter gradient within the bound of (a) (not bit-equal: the slice count differs).
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_path as O
from test_hip_parity import TOL, check, relmax
import test_egcl_layer_backward_gpu as L

pytestmark = pytest.mark.gpu

ROOT, PKG, METRIC = L.ROOT, L.PKG, L.METRIC
C, EA, NA = 8, 6, 3
SIZES = {"small": (13, 37), "hub": (L.N, L.E)}
CASES = [(size, aggr) for size in SIZES for aggr in ("mean", "sum")]
CASE_IDS = [f"{s}-{a}" for s, a in CASES]
_SWITCHES = ("CSMPN_CL_CAP_FWD", "CSMPN_CL_CAP_BWD", "CSMPN_SAVE_STATE")
ENVS = {
    "one-tile": {},
    "cap1": {"CSMPN_CL_CAP_FWD": "1", "CSMPN_CL_CAP_BWD": "1"},
    "cap2": {"CSMPN_CL_CAP_FWD": "2", "CSMPN_CL_CAP_BWD": "2"},
    "recompute": {"CSMPN_SAVE_STATE": "0"},
}
PAIRS = [(env, cid) for env in ENVS for cid in CASE_IDS]
PER_CHANNEL = ("0.bias", "1.a", "1.b", "2.weight", "2.normalization.a", "2.linear_left.bias", "3.a")


def inputs(size):
    """h, edge_index, edge_attr, node_attr, parameters, d/d(out), and d/d(out) confined to the last (partial) node tile."""
    N, E = SIZES[size]
    if size == "hub":
        h, ei, ea, na, p, gout = L.inputs("mean")
    else:
        o32 = O.Algebra(list(METRIC), torch.float32)
        h, ei, ea, na = O.synthetic_complex(o32, N, E, C, seed=81)
        gen = torch.Generator().manual_seed(82)
        p = O.init_egcl_params(o32, C, C, C, EA, NA, gen=gen, randomize=True)
        gout = torch.randn(N, C, 8, generator=gen)
    assert h.shape[0] == N and ei.shape[1] == E and N % 8 == 5 and E % 8
    tail = gout.clone()
    tail[: N - N % 8] = 0.0
    return h, ei, ea, na, p, gout, tail


# ------------------------------------------------------------------------------------------------------------ the child
def child_case(pkg, size, aggr):
    """Everything of one case that needs the GPU; CPU tensors back."""
    from csmpn_hip import ops
    dev = torch.device("cuda:0")
    N, _ = SIZES[size]
    h, ei, ea, na, p, gout, tail = inputs(size)
    cpu = lambda t: t.detach().cpu().clone()
    layer = pkg.EGCL(pkg.CliffordAlgebra(METRIC), C, C, C, edge_attr_features=EA, node_attr_features=NA, aggr=aggr)
    sd = layer.state_dict()
    sd.update(p)
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(dev)
    res = {}
    # (a), (d) the layer through autograd
    for key, g in (("auto", gout), ("tail", tail)):
        for prm in layer.parameters():
            prm.grad = None
        hd = h.to(dev).requires_grad_(True)
        y = layer(hd, ei.to(dev), ea.to(dev), na.to(dev))
        (y * g.to(dev)).sum().backward()
        res[key] = {"y": cpu(y), "gh": cpu(hd.grad)}
        res[key].update({"g." + k: cpu(v.grad) for k, v in layer.named_parameters()})
    # (b), (c) one forward state, the backward of the whole layer on it: twice with d/d(out), once with zeros
    be, spec = ops.HipBackend, layer.spec()
    csr = ops.get_csr(ei.to(dev), N)
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    hh, ead, nad = h.to(dev), ea.to(dev), na.to(dev)
    agg, st_e = be.edge_forward(spec, csr, hh, ead, pe)
    _, st_n = be.node_forward(spec, csr.deg, hh, agg, nad, pn)
    for key, g in (("first", gout), ("second", gout), ("zero", torch.zeros_like(gout))):
        _, _, _, views_e, views_n = be.layer_backward(spec, csr, hh, agg, ead, nad, pe, pn, g.to(dev), False, False, st_e, st_n)
        torch.cuda.synchronize()
        res[key] = [cpu(v) for v in list(views_e) + list(views_n)]
    return res


_BEGIN, _END = "[case] begin ", "[case] end "
_CHILD = r"""
import importlib, os, sys, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_cl_end_phase_gpu as T
pkg = importlib.import_module(T.PKG)
out = {}
for (size, aggr), cid in zip(T.CASES, T.CASE_IDS):
    os.write(2, (T._BEGIN + cid + "\n").encode())
    out[cid] = T.child_case(pkg, size, aggr)
    os.write(2, (T._END + cid + "\n").encode())
torch.save(out, sys.argv[2])
"""
_children = {}
_ended_badly = []    # an environment whose child did not end cleanly: nothing more is started on the GPU after that


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("cl_end_phase")


def run_env(env, workdir):
    """{case id: (tensors, the library's dispatch lines)} of one environment, from one child process."""
    if env in _children:
        return _children[env]
    assert not _ended_badly, f"not started: the child of {_ended_badly[0]} did not end cleanly"
    f = str(workdir / f"{env}.pt")
    clean = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, f], env=dict(clean, CSMPN_DEBUG="1", **ENVS[env]),
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
    _children[env] = {cid: (tensors[cid], logs[cid]) for cid in CASE_IDS}
    return _children[env]


# -------------------------------------------------------------------------------------------------------- the reference
_oracle = {}


def oracle(cid, which):
    """(float64 truth, float32 yardstick run) of a case with d/d(out) = `which` ("auto": all rows, "tail": the last tile's),
    computed once."""
    if (cid, which) not in _oracle:
        size, aggr = CASES[CASE_IDS.index(cid)]
        h, ei, ea, na, p, gout, tail = inputs(size)
        g = gout if which == "auto" else tail
        runs = []
        for dtype in (torch.float64, torch.float32):
            q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
            hh = h.detach().to(dtype).clone().requires_grad_(True)
            y = O.egcl(O.Algebra(list(METRIC), dtype), hh, ei, ea.to(dtype), na.to(dtype), q, aggr=aggr, residual=True)
            (y * g.to(dtype)).sum().backward()
            out = {"y": y.detach(), "gh": hh.grad}
            out.update({"g." + k: v.grad for k, v in q.items()})
            runs.append({k: v.numpy() for k, v in out.items()})
        _oracle[(cid, which)] = tuple(runs)
    return _oracle[(cid, which)]


def grad_names(t64):
    names = sorted(k for k in t64 if k.startswith("g."))
    assert len(names) == 40
    for model in ("edge_model", "node_model"):
        for blk in (0, 1):
            for tail in PER_CHANNEL:
                assert f"g.{model}.layers.{blk}.{tail}" in names
    return names


# ------------------------------------------------------------------------------------------------------------ the tests
def test_shapes_leave_idle_waves_and_partial_tiles():
    for size, (N, E) in SIZES.items():
        assert N % 8 == 5 and E % 8, size                 # the last tile of both programs is partial
    N, E = SIZES["small"]
    assert (N + 7) // 8 == 2 and (N + 31) // 32 == 1      # node launch: two tiles, one workgroup of four waves
    assert (E + 7) // 8 == 5 and (E + 31) // 32 == 2      # edge launch: the second workgroup has one tile ...
    assert E % 8 == 5                                     # ... of 5 valid rows


@pytest.mark.parametrize("env,cid", PAIRS)
def test_layer_against_the_float64_oracle(env, cid, workdir):
    (res, log) = run_env(env, workdir)[cid]
    t64, t32 = oracle(cid, "auto")
    got = res["auto"]
    assert set(got) == set(t64)
    grad_names(t64)
    for k in sorted(got):
        print(f"{env} {cid} {k}: err {relmax(got[k].numpy(), t64[k]):.2e}, float32 yardstick {relmax(t32[k], t64[k]):.2e}")
    for k in sorted(got):
        check(f"{env} {cid} {k}", got[k].numpy(), t64[k], t32[k], slack=4.0)
    # the kernels the case is about ran, at the grid the environment asks for
    N, E = SIZES[CASES[CASE_IDS.index(cid)][0]]
    cap = {"cap1": 1, "cap2": 2}.get(env, 1 << 30)
    for mode, rows in ((2, N), (1, E)):
        lines = [l for l in log if l.startswith(f"[csmpn] cl mode={mode} bwd=1 ")]
        assert lines, log
        grid = min(cap, (rows + 31) // 32)
        assert all(f" grid={grid} rows={rows}" in l for l in lines), lines


@pytest.mark.parametrize("env,cid", PAIRS)
def test_two_backward_passes_are_bit_equal(env, cid, workdir):
    (res, _) = run_env(env, workdir)[cid]
    assert len(res["first"]) == len(res["second"]) == 40
    assert any(float(a.abs().max()) > 0 for a in res["first"])
    for i, (a, b) in enumerate(zip(res["first"], res["second"])):
        assert torch.equal(a, b), (env, cid, f"param {i}", relmax(a.numpy(), b.numpy()))


@pytest.mark.parametrize("env,cid", PAIRS)
def test_zero_gradient_in_gives_exact_zeros(env, cid, workdir):
    (res, _) = run_env(env, workdir)[cid]
    assert len(res["zero"]) == 40
    for i, a in enumerate(res["zero"]):
        assert torch.equal(a, torch.zeros_like(a)), (env, cid, f"param {i}", float(a.abs().max()))


@pytest.mark.parametrize("env,cid", PAIRS)
def test_gradient_on_the_last_partial_tile_only(env, cid, workdir):
    (res, _) = run_env(env, workdir)[cid]
    t64, t32 = oracle(cid, "tail")
    for k in grad_names(t64):
        print(f"{env} {cid} tail {k}: err {relmax(res['tail'][k].numpy(), t64[k]):.2e}, "
              f"float32 yardstick {relmax(t32[k], t64[k]):.2e}")
    for k in grad_names(t64):
        check(f"{env} {cid} tail {k}", res["tail"][k].numpy(), t64[k], t32[k], slack=4.0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_grid_caps_agree(cid, workdir):
    t64, t32 = oracle(cid, "auto")
    got = {env: run_env(env, workdir)[cid][0]["auto"] for env in ("one-tile", "cap1", "cap2")}
    for k in grad_names(t64):
        bound = max(TOL, 4.0 * relmax(t32[k], t64[k]))
        for a, b in (("cap1", "cap2"), ("cap1", "one-tile"), ("cap2", "one-tile")):
            diff = relmax(got[a][k].numpy(), got[b][k].numpy())
            print(f"{cid} {k}: {a} against {b} {diff:.2e}, bound {bound:.2e}")
            assert diff <= bound, (cid, k, a, b, diff, bound)
