"""Float64 CEMLP, EGCL and task models on the device (csrc/cemlp_f64.hpp) against float64 truths: the reference's own
float64 fixtures, oracle/ref_path.py in float64 elsewhere. One comparison rule, stated in tests/f64_helpers.py:
bound = max(1e-5 * 2^-29, 4 x yardstick), the yardstick being a second float64 implementation on the host against the same
truth. Every case that reaches a module with a float64 tensor fails without the float64 family with 'must be float32'."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import f64_helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _compare(tag, res, truth, yard):
    """Every tensor under the rule; all figures are printed before the first miss is raised."""
    assert set(res) == set(truth), set(res) ^ set(truth)
    missed = []
    for k in sorted(truth):
        try:
            H.assert_close(f"{tag}.{k}", res[k], truth[k], yard[k])
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, "; ".join(missed)


# ----------------------------------------------------------------------------------------------- layer against the fixtures

@pytest.mark.parametrize("variant", H.EGCL_TAGS)
@pytest.mark.parametrize("kind,name", H.EGCL_FIXTURES)
def test_egcl_against_the_reference_float64_fixture(pkg, kind, name, variant):
    """y, gh, the attribute gradients and every parameter gradient of EGCL(...).double() with the fixture's parameters; the
    fixture graph has a duplicate and a triplicate edge, a self loop, an isolated node and a node of in-degree 8."""
    c = H.egcl_case(kind, name, variant)
    _compare(f"{kind}_{name}.{variant}", H.run_egcl(c, DEV), c["truth"], H.egcl_yardsticks(kind, name, variant))


# ----------------------------------------------------------------------------------------------- standalone CEMLP

@pytest.mark.parametrize("case", H.CEMLP_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_cemlp_against_ref_path_float64(pkg, case):
    """1, 2 and 4 blocks; widths 1 -> 1, 5 -> 4, the task widths (28 at D = 32, 32 at D = 8, 40 at D = 4) and the limit 64;
    rows 1, a tile - 1, a tile, a tile + 1 and one tile more than the grid holds (a workgroup's second tile)."""
    ref = H.cemlp_reference(*case)
    _compare("cemlp." + "-".join(str(v) for v in case), H.run_cemlp(*case[:5], ref, DEV), ref["truth"], ref["yard"])


def test_cemlp_no_rows(pkg):
    m = H.cemlp_module("cl30", 5, 4, 4, 2, H.cemlp_reference("cl30", 5, 4, 4, 2, 1)["params"], DEV)
    x = torch.zeros(0, 5, 8, dtype=torch.float64, device=DEV, requires_grad=True)
    y = m(x)
    assert tuple(y.shape) == (0, 4, 8) and y.dtype == torch.float64
    y.sum().backward()
    assert tuple(x.grad.shape) == (0, 5, 8)
    assert all(p.grad is not None and float(p.grad.abs().max()) == 0.0 for p in m.parameters())


def test_egcl_no_edges(pkg):
    """E = 0 with N > 0: the aggregate is zero, the node stage runs, the edge model's gradients are zero."""
    from oracle import ref_path as O
    c = H.egcl_case("egcl", "cl30", "mean_res1_ag1")
    layer = H.egcl_module(c, DEV)
    h = torch.from_numpy(c["h"]).to(DEV).requires_grad_(True)
    ei = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    ea = torch.zeros(0, 6, 8, dtype=torch.float64, device=DEV)
    na = torch.from_numpy(c["na"]).to(DEV)
    y = layer(h, ei, ea, na)
    (y * torch.from_numpy(c["gout"]).to(DEV)).sum().backward()
    o = O.Algebra(list(c["metric"]), torch.float64)
    q = {k: torch.from_numpy(v).clone().requires_grad_(True) for k, v in c["params"].items()}
    hc = torch.from_numpy(c["h"]).clone().requires_grad_(True)
    yo = O.egcl(o, hc, ei.cpu(), ea.cpu(), na.cpu(), q, aggr="mean", residual=True)
    (yo * torch.from_numpy(c["gout"])).sum().backward()
    yard = H.egcl_yardsticks("egcl", "cl30", "mean_res1_ag1")     # the same layer with its edges: the conditioning of the node stage
    H.assert_close("noedges.y", y.detach().cpu().numpy(), yo.detach().numpy(), yard["y"])
    H.assert_close("noedges.gh", h.grad.cpu().numpy(), hc.grad.numpy(), yard["gh"])
    for k, p in layer.named_parameters():
        if k.startswith("edge_model."):
            assert float(p.grad.abs().max()) == 0.0, k
        else:
            H.assert_close("noedges.g/" + k, p.grad.cpu().numpy(), q[k].grad.numpy(), yard["g/" + k])


def test_width_65_raises_with_the_limit(pkg):
    alg = pkg.CliffordAlgebra((1.0, 1.0, 1.0))
    m = pkg.CEMLP(alg, 3, 65, 65, n_layers=1).double().to(DEV)
    with pytest.raises(RuntimeError, match="limit of 64 channels"):
        m(torch.zeros(2, 3, 8, dtype=torch.float64, device=DEV))
    layer = pkg.EGCL(alg, 65, 65, 65).double().to(DEV)
    with pytest.raises(RuntimeError, match="limit of 64 channels"):
        layer(torch.zeros(3, 65, 8, dtype=torch.float64, device=DEV), torch.tensor([[0, 1], [1, 2]], device=DEV))


def test_mixed_dtypes_raise_and_launch_nothing(pkg):
    from csmpn_hip import native
    alg = pkg.CliffordAlgebra((1.0, 1.0, 1.0))
    ei = torch.tensor([[0, 1], [1, 2]], device=DEV)
    m32, m64 = pkg.CEMLP(alg, 2, 2, 2).to(DEV), pkg.CEMLP(alg, 2, 2, 2).double().to(DEV)
    m32(torch.zeros(1, 2, 8, device=DEV))                       # stamps csmpn_last_kernel with a float32 launch
    before = native.lib().csmpn_last_kernel()
    with pytest.raises(RuntimeError, match=r"torch\.float64.*torch\.float32"):
        m32(torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match=r"torch\.float32.*torch\.float64"):
        m64(torch.zeros(3, 2, 8, device=DEV))
    l64 = pkg.EGCL(alg, 2, 2, 2, edge_attr_features=1).double().to(DEV)
    with pytest.raises(RuntimeError, match=r"torch\.float64.*edge_attr is torch\.float32"):
        l64(torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV), ei, torch.zeros(2, 1, 8, device=DEV))
    l32 = pkg.EGCL(alg, 2, 2, 2).to(DEV)
    with pytest.raises(RuntimeError, match=r"torch\.float64.*torch\.float32"):
        l32(torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV), ei)
    # attribute tensors left on the host, float64 like the rest: the float32 path's error, never a host pointer in a kernel
    l64a = pkg.EGCL(alg, 2, 2, 2, edge_attr_features=1, node_attr_features=1).double().to(DEV)
    h64 = torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV)
    ea_d, na_d = torch.zeros(2, 1, 8, dtype=torch.float64, device=DEV), torch.zeros(3, 1, 8, dtype=torch.float64, device=DEV)
    with pytest.raises(RuntimeError, match="edge_attr is on cpu.*no CPU fallback"):
        l64a(h64, ei, ea_d.cpu(), na_d)
    with pytest.raises(RuntimeError, match="node_attr is on cpu.*no CPU fallback"):
        l64a(h64, ei, ea_d, na_d.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        l64a(h64, ei, ea_d.cpu(), na_d.cpu().float())          # host AND another dtype: still an error, whichever comes first
    # a module with only some parameters cast: every parameter is looked at
    half = pkg.CEMLP(alg, 2, 2, 2).double().to(DEV)
    half.layers[1][3].a.data = half.layers[1][3].a.data.float()
    with pytest.raises(RuntimeError, match=r"torch\.float64.*ln_a of block 1 is torch\.float32"):
        half(torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV))
    lhalf = pkg.EGCL(alg, 2, 2, 2).double().to(DEV)
    lhalf.node_model.layers[0][2].weight.data = lhalf.node_model.layers[0][2].weight.data.float()
    with pytest.raises(RuntimeError, match=r"gp_w of block 0 of the node model is torch\.float32"):
        lhalf(torch.zeros(3, 2, 8, dtype=torch.float64, device=DEV), ei)
    assert native.lib().csmpn_last_kernel() == before
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m64.cpu()(torch.zeros(3, 2, 8, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------- buffer discipline

GUARD, SENTINEL = 64, -7.25


def _guarded(n, dtype=torch.float64):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[GUARD + n:] == SENTINEL).all())


def test_buffers_guards_accumulation_and_identical_bits(pkg):
    """The C-ABI itself: y, gx, the gradient tensors and a workspace of exactly the queried size between guard regions;
    pre-filled gradients come back as pre-fill + gradient; a second call gives the same bits."""
    from csmpn_hip import native, ops
    case = ("cl30", 5, 4, 4, 2, "R+1")
    ref = H.cemlp_reference(*case)
    rows, D = ref["rows"], 8
    m = H.cemlp_module(*case[:5], ref["params"], DEV)
    b = m.binding()
    params = m.flat_params()
    b.bind(params)
    L, st = native.lib(), torch.cuda.current_stream(DEV).cuda_stream
    x, gy = ref["x"].to(DEV).contiguous(), ref["gy"].to(DEV).contiguous()
    nbytes = int(L.csmpn_cemlp_f64_workspace_bytes(b.n, b.params, b.nblk, rows))
    assert nbytes == H.plan(3, H.widths_of(*case[1:5]), rows)[3] and nbytes % 8 == 0
    PRE = 0.5

    def call():
        wsb, ws = _guarded(nbytes // 8)
        yb, y = _guarded(rows * 4 * D)
        gxb, gx = _guarded(rows * 5 * D)
        total = b.grad_floats(params)
        gb, flat = _guarded(total)
        flat.fill_(PRE)
        _f, views = b.new_grads(params, DEV, flat=flat, dtype=torch.float64)
        native.check(L.csmpn_cemlp_forward_f64(b.metric_arr, b.n, b.params, b.nblk, x.data_ptr(), rows, y.data_ptr(), ws.data_ptr(),
                                               nbytes, st))
        native.check(L.csmpn_cemlp_backward_f64(b.metric_arr, b.n, b.params, b.grads, b.nblk, x.data_ptr(), gy.data_ptr(), rows,
                                                gx.data_ptr(), ws.data_ptr(), nbytes, st))
        torch.cuda.synchronize()
        assert _intact(wsb, nbytes // 8) and _intact(yb, rows * 4 * D) and _intact(gxb, rows * 5 * D) and _intact(gb, total)
        # a workspace one byte short is rejected and nothing is written
        y.fill_(SENTINEL)
        assert L.csmpn_cemlp_forward_f64(b.metric_arr, b.n, b.params, b.nblk, x.data_ptr(), rows, y.data_ptr(), ws.data_ptr(),
                                         nbytes - 1, st) == native.ERR_INVALID
        torch.cuda.synchronize()
        assert bool((y == SENTINEL).all())
        native.check(L.csmpn_cemlp_forward_f64(b.metric_arr, b.n, b.params, b.nblk, x.data_ptr(), rows, y.data_ptr(), ws.data_ptr(),
                                               nbytes, st))
        torch.cuda.synchronize()
        return y.clone(), gx.clone(), [v.clone() for v in views if v is not None]

    y1, gx1, g1 = call()
    y2, gx2, g2 = call()
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    H.assert_close("abi.y", y1.reshape(rows, 4, D).cpu().numpy(), ref["truth"]["y"], ref["yard"]["y"])
    H.assert_close("abi.gx", gx1.reshape(rows, 5, D).cpu().numpy(), ref["truth"]["gx"], ref["yard"]["gx"])
    names = [k for k, _ in m.named_parameters()]
    by_ptr = {p.data_ptr(): k for k, p in m.named_parameters()}
    order = [by_ptr[p.data_ptr()] for p in params if p is not None]
    assert sorted(order) == sorted(names)
    for k, g in zip(order, g1):
        truth = ref["truth"]["g/" + k]
        # pre-fill + gradient is rounded once more, at the size of the sum: one ulp of (|pre-fill| + |gradient|) on the rule's scale
        extra = 2.0 ** -52 * (PRE + np.abs(truth).max()) / max(np.abs(truth).max(), 1e-300)
        H.assert_close("abi.prefilled.g/" + k, (g.cpu().numpy() - PRE), truth, ref["yard"]["g/" + k] + extra)


def test_stage_entry_points_between_guards(pkg):
    """The four EGCL stage entry points and the two segment sums called directly on the 8-channel Cl(3,0) fixture graph
    (duplicate and triplicate edges, a self loop, an isolated node; perm is no identity): the message table [E, O, D], agg,
    out, gh, g_agg, g_node_attr, the per-edge table [E, C, D], g_edge_attr, both flat gradient buffers and both workspaces of
    exactly the queried sizes sit between guard regions that stay intact, and the results are the fixture's."""
    from csmpn_hip import native, ops
    kind, name, variant = "egcl8", "cl30", "mean_res1_ag1"
    c = H.egcl_case(kind, name, variant)
    yard = H.egcl_yardsticks(kind, name, variant)
    layer = H.egcl_module(c, DEV)
    spec = layer.spec()
    e, nd = spec.edge, spec.node
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    e.bind(pe); nd.bind(pn)
    t = lambda a: torch.from_numpy(a).to(DEV).contiguous()
    h, ea, na, gout = t(c["h"]), t(c["ea"]), t(c["na"]), t(c["gout"])
    csr = ops.Csr(t(c["ei"]), h.shape[0])
    assert not torch.equal(csr.perm[:csr.n_edges].cpu(), torch.arange(csr.n_edges, dtype=torch.int32))
    N, E, C, O, D, A, T = h.shape[0], csr.n_edges, spec.C, spec.O, 8, spec.A, spec.T
    L, st = native.lib(), torch.cuda.current_stream(DEV).cuda_stream
    be = int(L.csmpn_cemlp_f64_workspace_bytes(e.n, e.params, e.nblk, E))
    bn = int(L.csmpn_cemlp_f64_workspace_bytes(nd.n, nd.params, nd.nblk, N))
    bufs = {}

    def g(key, n):
        bufs[key] = _guarded(n)
        return bufs[key][1]

    wse, wsn = g("wse", be // 8), g("wsn", bn // 8)
    msg, agg, out = g("msg", E * O * D), g("agg", N * O * D), g("out", N * O * D)
    gh, g_agg, g_na = g("gh", N * C * D), g("g_agg", N * O * D), g("g_na", N * T * D)
    rows, g_ea = g("rows", E * C * D), g("g_ea", E * A * D)
    fe, fn = g("fe", e.grad_floats(pe)), g("fn", nd.grad_floats(pn))
    fe.zero_(); fn.zero_()
    _x, ve = e.new_grads(pe, DEV, flat=fe, dtype=torch.float64)
    _x, vn = nd.new_grads(pn, DEV, flat=fn, dtype=torch.float64)
    chk = native.check
    chk(L.csmpn_egcl_edge_forward_f64(e.metric_arr, e.n, e.params, e.nblk, h.data_ptr(), C, ea.data_ptr(), A, csr.perm.data_ptr(),
                                      csr.src.data_ptr(), csr.dst.data_ptr(), E, N, msg.data_ptr(), wse.data_ptr(), be, st))
    ops.segment_reduce_f64(msg.view(E, O, D), agg.view(N, O, D), add=(csr.row_ptr, None), accumulate=False)
    chk(L.csmpn_egcl_node_forward_f64(nd.metric_arr, nd.n, nd.params, nd.nblk, h.data_ptr(), C, agg.data_ptr(), O, na.data_ptr(), T,
                                      csr.deg.data_ptr(), spec.mean, spec.residual, N, out.data_ptr(), wsn.data_ptr(), bn, st))
    chk(L.csmpn_egcl_node_backward_f64(nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, h.data_ptr(), C, agg.data_ptr(), O,
                                       na.data_ptr(), T, csr.deg.data_ptr(), spec.mean, spec.residual, N, gout.data_ptr(), gh.data_ptr(),
                                       g_agg.data_ptr(), g_na.data_ptr(), wsn.data_ptr(), bn, st))
    chk(L.csmpn_egcl_edge_backward_f64(e.metric_arr, e.n, e.params, e.grads, e.nblk, h.data_ptr(), C, ea.data_ptr(), A,
                                       csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), E, N, g_agg.data_ptr(),
                                       rows.data_ptr(), g_ea.data_ptr(), wse.data_ptr(), be, st))
    ops.segment_reduce_f64(rows.view(E, C, D), gh.view(N, C, D), add=(csr.row_ptr, None), sub=csr.source_order())
    torch.cuda.synchronize()
    for key, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), key
    H.assert_close("stages.y", out.view(N, O, D).cpu().numpy(), c["truth"]["y"], yard["y"])
    H.assert_close("stages.gh", gh.view(N, C, D).cpu().numpy(), c["truth"]["gh"], yard["gh"])
    H.assert_close("stages.g_edge_attr", g_ea.view(E, A, D).cpu().numpy(), c["truth"]["g_edge_attr"], yard["g_edge_attr"])
    H.assert_close("stages.g_node_attr", g_na.view(N, T, D).cpu().numpy(), c["truth"]["g_node_attr"], yard["g_node_attr"])
    for model, params, views in (("edge_model", pe, ve), ("node_model", pn, vn)):
        by_ptr = {p.data_ptr(): k for k, p in layer.named_parameters()}
        for p_, v in zip(params, views):
            k = by_ptr[p_.data_ptr()]
            assert k.startswith(model)
            H.assert_close("stages.g/" + k, v.cpu().numpy(), c["truth"]["g/" + k], yard["g/" + k])


def test_segment_sum_float64(pkg):
    from csmpn_hip import ops
    g = torch.Generator().manual_seed(3)
    N, E, W = 7, 23, 12
    ei = torch.randint(0, N - 1, (2, E), generator=g).to(DEV)       # node N - 1 stays isolated
    csr = ops.Csr(ei, N)
    rows = torch.randn(E, 3, 4, generator=g, dtype=torch.float64).to(DEV)
    ob, o = _guarded(N * W)
    out = o.view(N, 3, 4)
    out.fill_(2.0)
    ops.segment_reduce_f64(rows, out, add=(csr.row_ptr, None), sub=csr.source_order())
    torch.cuda.synchronize()
    assert _intact(ob, N * W)
    want = torch.full((N, 3, 4), 2.0, dtype=torch.float64)
    want.index_add_(0, csr.dst[:E].cpu().long(), rows.cpu())
    want.index_add_(0, csr.src[:E].cpu().long(), -rows.cpu())
    assert H.err(out.cpu().numpy(), want.numpy()) <= 16 * 2.0 ** -52       # up to E signed terms per node, each rounded once
    again = torch.full_like(out, 2.0)
    ops.segment_reduce_f64(rows, again, add=(csr.row_ptr, None), sub=csr.source_order())
    assert torch.equal(again, out)
    ops.segment_reduce_f64(rows, again, add=(csr.row_ptr, None), accumulate=False)
    assert float(again[N - 1].abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------- child process: bits, tiles

def _child(scenario):
    env = dict(os.environ, CSMPN_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "f64_helpers.py"), scenario], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def test_fresh_process_same_bits_and_second_tile(pkg):
    """Two calls here and one in a fresh child process give identical bits (the path ignores set_deterministic); the child's
    dispatch log shows that the 16385-row case gives a workgroup a second tile."""
    here = H.scenario_layer()
    assert here == H.scenario_layer()
    child, log = _child("layer")
    assert child == here
    lines = [l for l in log.split("[f64-child] second-tile case")[1].splitlines() if l.startswith("[csmpn] f64 ")]
    assert lines, log[-2000:]
    for l in lines:
        f = {k: int(v) for k, v in re.findall(r"(\w+)=(-?\d+)", l)}
        assert f["mode"] == 0 and f["tile_rows"] == 32 and f["rows"] == 16385 and f["tiles"] == 513 and f["grid"] == 512, l
    assert {int(re.search(r"bwd=(\d)", l).group(1)) for l in lines} == {0, 1}
    fam = [l.split()[1] for l in log.splitlines() if l.startswith("[csmpn] ") and " mode=" in l]
    assert set(fam) == {"f64"}, set(fam)


# ----------------------------------------------------------------------------------------------- gradcheck

def _host_cemlp_fn(metric, keys):
    from oracle import ref_path as O
    o = O.Algebra(list(metric), torch.float64)
    return lambda x, *ps: O.cemlp(o, x, dict(zip(keys, ps)))


def test_gradcheck_cemlp(pkg):
    """torch.autograd.gradcheck with torch's float64 defaults on CEMLP.double(): Cl(2,0), 2 -> 2 channels, 2 blocks, 3 rows; the
    inputs are the first seed for which the same call passes on the host through oracle/ref_path.py."""
    from csmpn_hip import ops
    from oracle import ref_path as O
    o = O.Algebra([1.0, 1.0], torch.float64)
    for seed in range(8):
        gen = torch.Generator().manual_seed(seed)
        p = O.init_cemlp_params(o, 2, 2, 2, 2, gen=gen, randomize=True, dtype=torch.float64)
        x = torch.randn(3, 2, 4, generator=gen, dtype=torch.float64)
        keys = list(p)
        host_in = [x.clone().requires_grad_(True)] + [p[k].clone().requires_grad_(True) for k in keys]
        if torch.autograd.gradcheck(_host_cemlp_fn((1.0, 1.0), keys), host_in, raise_exception=False):
            break
    else:
        pytest.fail("no seed passes gradcheck on the host")
    m = H.cemlp_module("cl20", 2, 2, 2, 2, p, DEV)
    flat = m.flat_params()
    dev_in = [x.to(DEV).requires_grad_(True)] + [q.detach().clone().requires_grad_(True) for q in flat]
    assert torch.autograd.gradcheck(lambda xx, *ps: ops.cemlp_apply(xx, m.binding(), list(ps)), dev_in)


def test_gradcheck_egcl(pkg):
    """... and on EGCL.double(): Cl(3,0), 2 channels, 4 nodes, 6 edges (a duplicate, a self loop), with attributes."""
    from csmpn_hip import ops
    from oracle import ref_path as O
    o = O.Algebra([1.0, 1.0, 1.0], torch.float64)
    ei = torch.tensor([[0, 1, 1, 2, 3, 0], [1, 2, 2, 2, 0, 3]])
    alg = pkg.CliffordAlgebra((1.0, 1.0, 1.0))
    for seed in range(8):
        gen = torch.Generator().manual_seed(seed)
        p = O.init_egcl_params(o, 2, 2, 2, edge_attr_f=2, node_attr_f=1, gen=gen, randomize=True, dtype=torch.float64)
        h, ea, na = (torch.randn(*s, generator=gen, dtype=torch.float64) for s in ((4, 2, 8), (6, 2, 8), (4, 1, 8)))
        keys = list(p)
        host_in = [t.clone().requires_grad_(True) for t in (h, ea, na)] + [p[k].clone().requires_grad_(True) for k in keys]
        if torch.autograd.gradcheck(lambda hh, e, n_, *ps: O.egcl(o, hh, ei, e, n_, dict(zip(keys, ps)), aggr="mean"), host_in,
                                    raise_exception=False):
            break
    else:
        pytest.fail("no seed passes gradcheck on the host")
    layer = pkg.EGCL(alg, 2, 2, 2, edge_attr_features=2, node_attr_features=1, aggr="mean").double()
    layer.load_state_dict({**layer.state_dict(), **p}, strict=True)
    layer = layer.to(DEV)
    flat = layer.edge_model.flat_params() + layer.node_model.flat_params()
    csr = ops.get_csr(ei.to(DEV), 4)
    dev_in = [t.to(DEV).requires_grad_(True) for t in (h, ea, na)] + [q.detach().clone().requires_grad_(True) for q in flat]
    assert torch.autograd.gradcheck(lambda hh, e, n_, *ps: ops.egcl_apply(hh, e, n_, layer.spec(), csr, list(ps)), dev_in)


# ----------------------------------------------------------------------------------------------- O(3) equivariance

def _compounds(Q):
    """Outermorphism of Q on Cl(3,0) in the blade order 'by grade, then lexicographic': block k = k-th compound matrix."""
    import itertools
    M = torch.zeros(8, 8, dtype=torch.float64)
    pos = 0
    for k in range(4):
        sub = list(itertools.combinations(range(3), k))
        for a, I in enumerate(sub):
            for b, J in enumerate(sub):
                M[pos + a, pos + b] = torch.linalg.det(Q[list(I)][:, list(J)]) if k else 1.0
        pos += len(sub)
    return M


@pytest.mark.parametrize("reflect", [False, True], ids=["rotation", "reflection"])
def test_egcl_o3_equivariance(pkg, reflect):
    """layer(rho(Q) x) against rho(Q) layer(x) for a random orthogonal Q, on the 4-channel Cl(3,0) fixture graph with random full
    multivector inputs; the yardstick is the same check on the host through oracle/ref_path.py."""
    from oracle import ref_path as O
    c = H.egcl_case("egcl", "cl30", "mean_res1_ag0")
    gen = torch.Generator().manual_seed(11)
    Q, _ = torch.linalg.qr(torch.randn(3, 3, generator=gen, dtype=torch.float64))
    if (torch.linalg.det(Q) < 0) != reflect:
        Q = Q * torch.tensor([1.0, 1.0, -1.0], dtype=torch.float64)
    assert (float(torch.linalg.det(Q)) < 0) == reflect
    M = _compounds(Q)
    rho = lambda t: t @ M.T
    h, ea, na = (torch.randn(*c[k].shape, generator=gen, dtype=torch.float64) for k in ("h", "ea", "na"))
    ei = torch.from_numpy(c["ei"])
    o = O.Algebra(list(c["metric"]), torch.float64)
    p = {k: torch.from_numpy(v) for k, v in c["params"].items()}
    host = lambda a, b_, d: O.egcl(o, a, ei, b_, d, p, aggr="mean", residual=True)
    yard = H.err(host(rho(h), rho(ea), rho(na)).numpy(), rho(host(h, ea, na)).numpy())
    layer = H.egcl_module(c, DEV)
    with torch.no_grad():
        dev = lambda a, b_, d: layer(a.to(DEV), ei.to(DEV), b_.to(DEV), d.to(DEV)).cpu()
        H.assert_close("equivariance." + ("reflection" if reflect else "rotation"), dev(rho(h), rho(ea), rho(na)).numpy(),
                       rho(dev(h, ea, na)).numpy(), yard)


# ----------------------------------------------------------------------------------------------- task models

@pytest.fixture(scope="module")
def model_child():
    return _child("models")


@pytest.mark.parametrize("kind", H.MODELS)
def test_model_float64_step(pkg, monkeypatch, model_child, kind):
    """model.double() on batch.to(device, dtype=torch.float64): the loss and every f64/gn/* (norm, directional dot) of the
    reference's float64 fixture; yardstick: the same model in float64 on the host with the layers computed by the oracle.
    From the child's dispatch log: every CEMLP / EGCL launch of the step is of family f64, no float32 glue kernel ran."""
    loss, gn, _ = H.model_step(kind, torch.float64, DEV)
    got = H.model_errors(kind, loss, gn)
    with monkeypatch.context() as mp:
        H.host_oracle_injection(mp.setattr)
        hl, hgn, _ = H.model_step(kind, torch.float64)
    yard = H.model_errors(kind, hl, hgn)
    worst = max(got, key=lambda k: got[k] / H.bound(yard[k]))
    print(f"[f64] model {kind}: loss err {got['backprop_loss']:.3e} (yardstick {yard['backprop_loss']:.3e}); worst {worst} "
          f"err {got[worst]:.3e} yardstick {yard[worst]:.3e}")
    missed = {k: (got[k], yard[k]) for k in got if got[k] > H.bound(yard[k])}
    assert not missed, missed
    res, log = model_child
    part = log.split(f"[f64-child] model {kind}\n")[1].split("[f64-child]")[0]
    fam = [l.split()[1] for l in part.splitlines() if l.startswith("[csmpn] ") and " mode=" in l]
    assert fam and set(fam) == {"f64"}, sorted(set(fam))
    # (the child's figures are not compared bit for bit: the models' composed float64 glue uses torch's index_add_, whose
    # float atomics are outside this kernel family; test_fresh_process_same_bits_and_second_tile holds the kernels to it)
    assert abs(res[kind]["loss"] - float(loss)) <= 1e-12 * abs(float(loss))


GLUE = ["simplex_rows", "embed_cemlp_apply", "type_attr_apply", "readout_mse", "readout_traj", "mvlinear_apply", "mvsilu_apply",
        "mvnorm_apply", "mvlayernorm_apply", "wgp_apply", "geometric_product_apply"]


def test_no_float32_glue_in_a_float64_step(pkg, monkeypatch):
    """The float32-only entry points behind the gates of the models - simplex rows, the fused embedding, the type
    attributes, both read-outs, the standalone small layers and the geometric product - are each called in a float32 step of
    some model and in no float64 step (every one of them is counted at its function in csmpn_hip.ops, which the models
    look up at call time; the dispatch log does not name these kernels)."""
    from csmpn_hip import ops
    calls = {k: 0 for k in GLUE}

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return wrapped

    for k in GLUE:
        monkeypatch.setattr(ops, k, spy(k, getattr(ops, k)))
    for kind in H.MODELS:
        H.model_step(kind, torch.float32, DEV)
    seen32 = dict(calls)
    for k in ("simplex_rows", "embed_cemlp_apply", "type_attr_apply", "readout_mse", "readout_traj", "mvlinear_apply"):
        assert seen32[k] > 0, (k, seen32)             # the spies do sit where the models call
    for kind in H.MODELS:
        H.model_step(kind, torch.float64, DEV)
    assert calls == seen32, {k: calls[k] - seen32[k] for k in GLUE if calls[k] != seen32[k]}


def test_float32_steps_unchanged_bit_for_bit(pkg, monkeypatch):
    """The float32 loss and gradients of the four model steps under CSMPN_DETERMINISTIC=1 equal the recording made by the
    same helper on the commit in front of the float64 family (tools/record_f32_steps.py)."""
    monkeypatch.setenv("CSMPN_DETERMINISTIC", "1")
    rec = np.load(H.F32_RECORDING)
    got = H.f32_step_record()
    assert set(got) == set(rec.files)
    for k in rec.files:
        assert got[k].dtype == rec[k].dtype and np.array_equal(got[k], rec[k]), k
