"""The (row, channel)-per-lane backward where a wave owns ONE tile - and where it does not.

cemlp_cl_bwd_kernel runs two instantiations of its blocks inside one kernel: with at most one tile per wave (S1's node
launch, every small layer) the rows of every block are requested ahead, d/d(block input) stays in registers and no store
is waited for between the blocks; with several tiles per wave the hand-over goes through L2 behind a `vmcnt(0)`. Both are
run here on the Cl(3,0) 8-channel EGCL layer, at sizes chosen for the tile bookkeeping:

    N = 37,  E = 101    one tile per wave; 5 node tiles, the last with 5 valid rows of 8
    N = 600, E = 9000   one tile per wave; 75 node tiles on 19 workgroups = 76 waves: the last wave owns no tile and still
                        takes part in the images, the barriers and the slice sums
    N = 8,   E = 0      no adjacency at all: the edge stages have no rows, the node stages one tile
    N = 600, E = 9000   CSMPN_CL_CAP_BWD = CSMPN_CL_CAP_FWD = 2 in a child process (the switches are read once): two
                        workgroups = eight waves walk 75 node tiles and 1 125 edge tiles

y, d/dh and every parameter gradient of both models against the float64 C++ twin, bound = the rule of
tests/test_full_size_twin.py: max(1e-5, 4 x the float32 twin's own error), per tensor and element-wise. Every case also
reads csmpn_last_kernel behind each stage (called on this thread) and compares it with the dispatch snapshot: the cl
kernels ran, not another family. The parameter gradients are sums of per-workgroup slices added in a fixed order: two
runs in one process must agree bit for bit.
"""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_path as O
from test_full_size_twin import _twin
from test_hip_parity import check, deterministic_aggregation, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "clifford-group-equivariant-simplicial-message-passing-networks_amd"
METRIC, C = (1.0, 1.0, 1.0), 8
SMALL, LARGE, EMPTY = (37, 101), (600, 9000), (8, 0)
SNAPSHOT_KEY = {SMALL: "egcl-cl30-8@small", LARGE: "egcl-cl30-8@large"}
_cache = {}


def cl_grid(rows, bwd, cap=None):
    """cl_grid of csrc/dispatch.hip: ceil(tiles / 4) workgroups of four waves, tiles = ceil(rows / 8), below the caps
    (512 backward, 1024 forward: neither is reached here)."""
    tiles = (rows + 7) // 8
    grid = (tiles + 3) // 4
    return min(grid, cap) if cap else grid


def _case(size):
    """inputs, parameters and the twin's float64 / float32 results of one size (computed once per session)"""
    if size in _cache:
        return _cache[size]
    N, E = size
    o32 = O.Algebra(list(METRIC), torch.float32)
    h, ei, ea, na = O.synthetic_complex(o32, N, E, C, seed=21 + N)
    gen = torch.Generator().manual_seed(22 + N)
    p = O.init_egcl_params(o32, C, C, C, 6, 3, gen=gen, randomize=True)
    gout = torch.randn(N, C, 8, generator=gen)
    args = (np.asarray(METRIC, np.float32), {k: v.numpy() for k, v in p.items()}, h.numpy(), ei.numpy(), ea.numpy(), na.numpy())
    t64 = _twin().egcl_layer(*args, aggr="mean", gout=gout.numpy(), real64=True)
    t32 = _twin().egcl_layer(*args, aggr="mean", gout=gout.numpy(), real64=False)
    _cache[size] = (h, ei, ea, na, p, gout, t64, t32)
    return _cache[size]


def _layer(p):
    pkg = importlib.import_module(PKG)
    layer = pkg.EGCL(pkg.CliffordAlgebra(METRIC), C, C, C, edge_attr_features=6, node_attr_features=3, aggr="mean")
    sd = layer.state_dict()
    sd.update(p)
    layer.load_state_dict(sd, strict=True)
    return layer.to(dev())


def _run(size):
    """The layer through autograd: y, d/dh, {parameter: gradient}."""
    h, ei, ea, na, p, gout, _, _ = _case(size)
    layer = _layer(p)
    hd = h.to(dev()).requires_grad_(True)
    y = layer(hd, ei.to(dev()), ea.to(dev()), na.to(dev()))
    (y * gout.to(dev())).sum().backward()
    torch.cuda.synchronize()
    return y.detach().cpu().numpy(), hd.grad.cpu().numpy(), {k: v.grad.cpu().numpy() for k, v in layer.named_parameters()}


def _stage_kernels(size):
    """csmpn_last_kernel behind each of the four stages, called on this thread (the name is kept per thread)."""
    from csmpn_hip import native, ops
    h, ei, ea, na, p, gout, _, _ = _case(size)
    layer = _layer(p)
    last = lambda: native.lib().csmpn_last_kernel().decode()
    hd, ead, nad = h.to(dev()), ea.to(dev()), na.to(dev())
    be, spec = ops.HipBackend, layer.spec()
    csr = ops.get_csr(ei.to(dev()), hd.shape[0])
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    names = {}
    agg, st_e = be.edge_forward(spec, csr, hd, ead, pe)
    names["edge_fwd"] = last()
    out, st_n = be.node_forward(spec, csr.deg, hd, agg, nad, pn)
    names["node_fwd"] = last()
    gh, g_agg, _, _ = be.node_backward(spec, csr.deg, hd, agg, nad, pn, gout.to(dev()), False, st_n)
    names["node_bwd"] = last()
    be.edge_backward(spec, csr, hd, ead, pe, g_agg, gh, False, st_e)
    names["edge_bwd"] = last()
    torch.cuda.synchronize()
    return names


def _recorded_kernels(size):
    """the snapshot's kernel names at the size that was run (the size without adjacency is not recorded: the small one's)"""
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_snapshot.json")) as f:
        return json.load(f)["default"][SNAPSHOT_KEY.get(size, SNAPSHOT_KEY[SMALL])]["kernels"]


def compare(size):
    """One size against the twin and the snapshot's kernel names; returns the worst error and its tensor's yardstick."""
    *_, t64, t32 = _case(size)
    y, gh, grads = _run(size)
    report = {"y": (check("y", y, t64["out"], t32["out"], slack=4.0), t32["out"], t64["out"]),
              "gh": (check("gh", gh, t64["gh"], t32["gh"], slack=4.0), t32["gh"], t64["gh"])}
    assert set(grads) == set(t64["grads"])
    for k, g in grads.items():
        report[k] = (check("g." + k, g, t64["grads"][k], t32["grads"][k], slack=4.0), t32["grads"][k], t64["grads"][k])
    want = _recorded_kernels(size)
    got = _stage_kernels(size)
    stages = ("node_fwd", "node_bwd") if size[1] == 0 else tuple(want)   # no adjacency: the edge stages launch nothing
    for st in stages:
        assert got[st] == want[st], (st, got[st])
    worst = max(report, key=lambda k: report[k][0])
    return f"{size}: worst tensor {worst}: HIP err {report[worst][0]:.2e}"


def test_spare_wave_owns_no_tile():
    """600 nodes = 75 tiles on 19 workgroups = 76 waves; 37 nodes = 5 tiles (the last with 5 rows) on 2 workgroups; the
    grids are the ones the dispatch snapshot records for these sizes."""
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_snapshot.json")) as f:
        snap = json.load(f)["default"]
    for (N, E), key in SNAPSHOT_KEY.items():
        for mode, rows, i0 in ((2, N, 19), (1, E, 14)):
            line = f"[csmpn] cl mode={mode} bwd=1 channels=8 i0={i0} grid={cl_grid(rows, True)} rows={rows}"
            assert line in snap[key]["log"], line
    tiles, waves = (600 + 7) // 8, 4 * cl_grid(600, True)
    assert (tiles, waves) == (75, 76)
    assert 75 * 8 >= 600 > 74 * 8        # tile 74 is the last one, wave 75 (the 76th) has none
    assert (37 + 7) // 8 == 5 and 37 - 4 * 8 == 5 and 4 * cl_grid(37, True) == 8
    # one tile per wave at both sizes, node and edge launch alike
    for rows in (37, 101, 600, 9000):
        assert (rows + 7) // 8 <= 4 * cl_grid(rows, True)


@pytest.mark.parametrize("size", [SMALL, LARGE, EMPTY], ids=["tail-tile-masked", "one-spare-wave", "no-adjacency"])
def test_one_tile_per_wave_against_the_float64_twin(pkg, size):
    print(compare(size))


def test_parameter_gradients_do_not_depend_on_the_run(pkg):
    """The slices are added in index order: two runs in one process give the same bits in every parameter gradient (under
    deterministic aggregation: the atomic scatter of the edge forward has no fixed order of its own)."""
    with deterministic_aggregation():
        _, _, first = _run(LARGE)
        _, _, second = _run(LARGE)
    assert set(first) == set(second)
    for k in first:
        assert np.array_equal(first[k].view(np.uint32), second[k].view(np.uint32)), k


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import test_cl_single_tile_gpu as T
print(T.compare(T.LARGE))
"""


def test_several_tiles_per_wave_at_small_size(pkg):
    """Two workgroups walk every tile: the hand-over rows go through L2, every block has its own end phase."""
    env = dict(os.environ, CSMPN_DEBUG="1", CSMPN_CL_CAP_BWD="2", CSMPN_CL_CAP_FWD="2")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout.strip())
    log = [l for l in r.stderr.splitlines() if l.startswith("[csmpn] cl ")]
    for mode, rows, i0 in ((2, 600, 19), (1, 9000, 14)):
        for bwd in (0, 1):
            assert f"[csmpn] cl mode={mode} bwd={bwd} channels=8 i0={i0} grid=2 rows={rows}" in log, (mode, bwd, log)
    # eight waves, 75 and 1 125 tiles: several tiles per wave in all four launches
    assert 75 > 4 * cl_grid(600, True, cap=2) and 1125 > 4 * cl_grid(9000, True, cap=2)
