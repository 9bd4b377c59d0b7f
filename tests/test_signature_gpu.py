"""CEMLP / EGCL on every signature Cl(p,q), p + q = 2..5, on the device (csrc/cemlp_sig.hpp): the five fixtures of the reference
in float64 and float32, the sweep over all 60 signatures with the kernel of every launch, bit identity of the sig kernel
with the compiled float64 kernels, the tile walk, buffers and repeatability at the C-ABI, gradcheck, Lorentz equivariance,
the refusals and the routing. Rules, cases and child-process scenarios: tests/signature_helpers.py."""
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

import signature_helpers as H

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32
SIG_KERNEL = r"csmpn::sig::cemlp_sig_kernel<%d, %s, (fwd|bwd)>"


def _child(scenario, **env):
    e = {k: v for k, v in os.environ.items() if k != "CSMPN_FORCE_SIG"}
    e.update(CSMPN_DEBUG="1", **env)
    r = subprocess.run([sys.executable, os.path.join(H.ROOT, "tests", "signature_helpers.py"), scenario], capture_output=True, text=True,
                       env=e, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def _dispatch(log):
    """[(family, {field: int})] of the row-kernel lines of a CSMPN_DEBUG log."""
    out = []
    for l in log.splitlines():
        if l.startswith("[csmpn] ") and " mode=" in l:
            out.append((l.split()[1], {k: int(v, 0) for k, v in re.findall(r"(\w+)=(-?(?:0x[0-9a-f]+|\d+))", l)}, l))
    return out


# ----------------------------------------------------------------------------------------------- 1. fixture variants

@pytest.mark.parametrize("variant", H.TAGS)
@pytest.mark.parametrize("name", list(H.SIGNATURES))
def test_fixture_variant_float64(pkg, name, variant):
    from csmpn_hip import native
    c = H.egcl_case(name, variant)
    y64, _, _ = H.yardsticks(name, variant)
    res = H.run_egcl(c, DEV, F64)
    assert re.match(SIG_KERNEL % (len(c["metric"]), "double"), native.lib().csmpn_last_kernel().decode())
    for k, t in c["truth"].items():
        H.assert_close(f"{name}/{variant}/f64/{k}", res[k], t, y64[k])


@pytest.mark.parametrize("variant", H.TAGS)
@pytest.mark.parametrize("name", list(H.SIGNATURES))
def test_fixture_variant_float32(pkg, name, variant):
    from csmpn_hip import native
    if H.excluded(name, variant):
        # float32 itself is off by more than 1e-2 here (tests/test_signature_cpu.py asserts that this is cl23 / noattr alone):
        # the layer still has to run and give finite results
        res = H.run_egcl(H.egcl_case(name, variant), DEV, F32)
        assert all(np.isfinite(v).all() for v in res.values())
        return
    c = H.egcl_case(name, variant)
    _, y32, _ = H.yardsticks(name, variant)
    res = H.run_egcl(c, DEV, F32)
    assert re.match(SIG_KERNEL % (len(c["metric"]), "float"), native.lib().csmpn_last_kernel().decode())
    for k, t in c["truth"].items():
        H.assert_close(f"{name}/{variant}/f32/{k}", res[k], t, y32[k], f32=True)


# ----------------------------------------------------------------------------------------------- 2. the sweep

def test_sweep_of_all_60_signatures_float64_and_their_kernels(pkg):
    res, log = _child("sweep")
    sigs = H.all_signatures()
    assert len(res) == 120
    for n, neg, _ in sigs:
        for what in ("cemlp", "egcl"):
            for k, (e, yard) in res[f"{n}/{neg}/{what}"].items():
                assert np.isfinite(e) and e <= H.F.bound(yard), (n, neg, what, k, e, yard)
    parts = log.split("[sig-child] signature ")[1:]
    assert len(parts) == 60
    for part in parts:
        n, neg = (int(v) for v in re.match(r"n=(\d+) neg=(\d+)", part).groups())
        lines = _dispatch(part)
        # CEMLP forward + backward, EGCL edge + node forward and backward: six row-kernel launches
        assert len(lines) == 6, part[:2000]
        want = "f64" if (n, neg) in H.COMPILED else "sig"
        assert {f for f, _, _ in lines} == {want}, (n, neg, [l for _, _, l in lines])
        if want == "sig":
            assert all(f["n"] == n and f["neg"] == neg and "dtype=f64" in l for _, f, l in lines), part[:2000]
        assert sorted(f["bwd"] for _, f, _ in lines) == [0, 0, 0, 1, 1, 1]
        assert sorted(f["mode"] for _, f, _ in lines) == [0, 0, 1, 1, 2, 2]


# ----------------------------------------------------------------------------------------------- 3. bit identity

def test_force_sig_gives_the_bits_of_the_compiled_float64_kernels(pkg):
    """CSMPN_FORCE_SIG=1 sends the six compiled algebras to the sig kernel too: same arithmetic, same order, only the source of
    the sign differs - the float64 results on three fixtures are the default process's, bit for bit; and a fresh process
    repeats the bits of a sig-only layer in both dtypes."""
    default, log0 = _child("bits")
    forced, log1 = _child("bits", CSMPN_FORCE_SIG="1")
    here = H.scenario_bits()
    for kind, name in H.BIT_FIXTURES:
        key = f"{kind}_{name}"
        assert default[key] == forced[key] == here[key], key
        assert "cemlp_f64_kernel" in default[key + "/kernel"] and "cemlp_sig_kernel" in forced[key + "/kernel"], key
    for key in ("cl13/f32", "cl13/f64"):
        assert default[key] == forced[key] == here[key], key
    assert {f for f, _, _ in _dispatch(log1)} == {"sig"}
    assert {f for f, _, _ in _dispatch(log0.split("[sig-child] cl13")[0])} == {"f64"}


@pytest.mark.parametrize("kind,name", [("egcl", "cl30"), ("egcl", "cl41"), ("egcl8", "cl41")])
def test_float_sig_entry_points_on_compiled_algebras(pkg, kind, name, monkeypatch):
    """The float *_sig entry points accept the compiled algebras too: Cl(3,0) and Cl(4,1) fixtures through them (the module
    routes a compiled algebra to its own kernels, so the routing predicate is overridden here), held to the float32 rule."""
    from csmpn_hip import native, ops
    monkeypatch.setattr(ops.CemlpBinding, "sig_only", lambda self: True)
    for variant in ("sum_res1_ag1", "mean_res0_ag0"):
        c = H.compiled_case(kind, name, variant)
        _, y32, _ = H.compiled_yardsticks(kind, name, variant)
        res = H.run_egcl(c, DEV, F32)
        assert re.match(SIG_KERNEL % (len(c["metric"]), "float"), native.lib().csmpn_last_kernel().decode())
        for k, t in c["truth"].items():
            H.assert_close(f"{kind}_{name}/{variant}/sig32/{k}", res[k], t, y32[k], f32=True)


# ----------------------------------------------------------------------------------------------- 4. tile walk

def test_tile_walk_second_tile_both_dtypes(pkg):
    res, log = _child("tiles")
    for tag, plan, dt in (("f64", H.plan64, "f64"), ("f32", H.plan32, "f32")):
        rows = H.tile_rows(plan)
        R, tiles, grid = plan(2, [(2, 2)], rows)[:3]
        assert res[tag + "/rows"] == rows and tiles == grid + 1
        for k, (e, yard) in res[tag].items():
            b = H.bound32(yard) if tag == "f32" else H.F.bound(yard)
            print(f"[sig] tiles/{tag}/{k}: err {e:.3e} yardstick {yard:.3e} bound {b:.3e}")
            assert np.isfinite(e) and e <= b, (tag, k, e, yard)
        lines = [(f, l) for fam, f, l in _dispatch(log.split(f"[sig-child] tiles {tag}")[1].split("[sig-child]")[0]) if fam == "sig"]
        assert len(lines) == 2 and {f["bwd"] for f, _ in lines} == {0, 1}, log[-2000:]
        for f, l in lines:
            assert f"dtype={dt}" in l and f["rows"] == rows and f["tile_rows"] == R and f["tiles"] == tiles and f["grid"] == grid, l


# ----------------------------------------------------------------------------------------------- 5. buffers, repeatability

GUARD = 64
PRE = 0.75


def _guarded(n, dtype=F32):
    buf = torch.full((n + 2 * GUARD,), -7.5, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, n):
    return bool((buf[:GUARD] == -7.5).all()) and bool((buf[GUARD + n:] == -7.5).all())


def test_plain_entry_points_between_guards_accumulate_and_repeat(pkg):
    """csmpn_cemlp_forward_sig / _backward_sig on cl13, 5 -> 4 -> 4 channels, R + 1 rows: outputs, gradients and a workspace of
    exactly the queried size between guard regions; parameter gradients are added to a pre-fill; two calls give the same bits."""
    from csmpn_hip import native
    metric, widths = H.SIGNATURES["cl13"], [(5, 4), (4, 4)]
    R = H.plan32(4, widths, 1)[0]
    rows, D = R + 1, 16
    ref = H.cemlp_reference(metric, 5, 4, 4, 2, rows)
    truth = H.oracle_cemlp(metric, ref)
    yard = {k: H.err(ref["twin32"][k], v) for k, v in truth.items()}
    P = H.F.pkg()
    m = P.CEMLP(P.CliffordAlgebra(metric), 5, 4, 4, n_layers=2)
    sd = m.state_dict()
    for k, v in ref["params"].items():
        sd[k] = v.float()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    b, params = m.binding(), m.flat_params()
    b.bind(params)
    L, st = native.lib(), torch.cuda.current_stream(DEV).cuda_stream
    need = int(L.csmpn_cemlp_sig_workspace_bytes(4, b.params, b.nblk, rows))
    assert need == H.plan32(4, widths, rows)[3] and need % 4 == 0
    x, gy = ref["x"].float().to(DEV).contiguous(), ref["gy"].float().to(DEV).contiguous()

    def once():
        bufs = {k: _guarded(n) for k, n in (("ws", need // 4), ("y", rows * 4 * D), ("gx", rows * 5 * D), ("flat", b.grad_floats(params)))}
        bufs["flat"][1].fill_(PRE)
        _x, views = b.new_grads(params, DEV, flat=bufs["flat"][1])
        native.check(L.csmpn_cemlp_forward_sig(b.metric_arr, 4, b.params, b.nblk, x.data_ptr(), rows, bufs["y"][1].data_ptr(),
                                               bufs["ws"][1].data_ptr(), need, st))
        native.check(L.csmpn_cemlp_backward_sig(b.metric_arr, 4, b.params, b.grads, b.nblk, x.data_ptr(), gy.data_ptr(), rows,
                                                bufs["gx"][1].data_ptr(), bufs["ws"][1].data_ptr(), need, st))
        torch.cuda.synchronize()
        for key, (buf, view) in bufs.items():
            assert _intact(buf, view.numel()), key
        return bufs["y"][1].view(rows, 4, D).clone(), bufs["gx"][1].view(rows, 5, D).clone(), [v.clone() for v in views if v is not None]

    y1, gx1, g1 = once()
    y2, gx2, g2 = once()
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    assert "cemlp_sig_kernel<4, float, bwd>" in L.csmpn_last_kernel().decode()
    H.assert_close("abi.y", y1.cpu().numpy(), truth["y"], yard["y"], f32=True)
    H.assert_close("abi.gx", gx1.cpu().numpy(), truth["gx"], yard["gx"], f32=True)
    by_ptr = {p.data_ptr(): k for k, p in m.named_parameters()}
    order = [by_ptr[p.data_ptr()] for p in params if p is not None]
    assert sorted(order) == sorted(by_ptr.values())
    for k, g in zip(order, g1):
        t = truth["g/" + k]
        # pre-fill + gradient is rounded once more, at the size of the sum: one ulp of (|pre-fill| + |gradient|) on the rule's scale
        extra = 2.0 ** -23 * (PRE + np.abs(t).max()) / max(np.abs(t).max(), 1e-300)
        H.assert_close("abi.prefilled.g/" + k, g.cpu().numpy().astype(np.float64) - PRE, t, yard["g/" + k] + extra, f32=True)
    # one byte short: rejected, nothing written
    yb, yv = _guarded(rows * 4 * D)
    rc = L.csmpn_cemlp_forward_sig(b.metric_arr, 4, b.params, b.nblk, x.data_ptr(), rows, yv.data_ptr(), x.data_ptr(), need - 1, st)
    torch.cuda.synchronize()
    assert rc == native.ERR_INVALID and bool((yb == -7.5).all())


def test_stage_entry_points_between_guards(pkg):
    """The four float EGCL stage entry points and csmpn_segment_reduce called directly on the cl13 fixture graph (duplicate and
    triplicate edges, a self loop, an isolated node, in-degree 8; perm is no identity): every table, gradient and workspace of
    exactly the queried size between guard regions that stay intact, and the results are the fixture's by the float32 rule."""
    from csmpn_hip import native, ops
    name, variant = "cl13", "mean_res1_ag1"
    c = H.egcl_case(name, variant)
    _, yard, _ = H.yardsticks(name, variant)
    layer = H.egcl_module(c, DEV, F32)
    spec = layer.spec()
    e, nd = spec.edge, spec.node
    pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
    e.bind(pe); nd.bind(pn)
    t = lambda a: torch.from_numpy(a).float().to(DEV).contiguous()
    h, ea, na, gout = t(c["h"]), t(c["ea"]), t(c["na"]), t(c["gout"])
    csr = ops.Csr(torch.from_numpy(c["ei"]).to(DEV), h.shape[0])
    assert not torch.equal(csr.perm[:csr.n_edges].cpu(), torch.arange(csr.n_edges, dtype=torch.int32))
    N, E, C, O, D, A, T = h.shape[0], csr.n_edges, spec.C, spec.O, 16, spec.A, spec.T
    L, st = native.lib(), torch.cuda.current_stream(DEV).cuda_stream
    be = int(L.csmpn_cemlp_sig_workspace_bytes(e.n, e.params, e.nblk, E))
    bn = int(L.csmpn_cemlp_sig_workspace_bytes(nd.n, nd.params, nd.nblk, N))
    bufs = {}

    def g(key, n):
        bufs[key] = _guarded(n)
        return bufs[key][1]

    wse, wsn = g("wse", be // 4), g("wsn", bn // 4)
    msg, agg, out = g("msg", E * O * D), g("agg", N * O * D), g("out", N * O * D)
    gh, g_agg, g_na = g("gh", N * C * D), g("g_agg", N * O * D), g("g_na", N * T * D)
    rows, g_ea = g("rows", E * C * D), g("g_ea", E * A * D)
    fe, fn = g("fe", e.grad_floats(pe)), g("fn", nd.grad_floats(pn))
    fe.zero_(); fn.zero_()
    _x, ve = e.new_grads(pe, DEV, flat=fe)
    _x, vn = nd.new_grads(pn, DEV, flat=fn)
    chk = native.check
    chk(L.csmpn_egcl_edge_forward_sig(e.metric_arr, e.n, e.params, e.nblk, h.data_ptr(), C, ea.data_ptr(), A, csr.perm.data_ptr(),
                                      csr.src.data_ptr(), csr.dst.data_ptr(), E, N, msg.data_ptr(), wse.data_ptr(), be, st))
    ops.segment_reduce(msg.view(E, O, D), agg.view(N, O, D), add=(csr.row_ptr, None), accumulate=False)
    chk(L.csmpn_egcl_node_forward_sig(nd.metric_arr, nd.n, nd.params, nd.nblk, h.data_ptr(), C, agg.data_ptr(), O, na.data_ptr(), T,
                                      csr.deg.data_ptr(), spec.mean, spec.residual, N, out.data_ptr(), wsn.data_ptr(), bn, st))
    chk(L.csmpn_egcl_node_backward_sig(nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, h.data_ptr(), C, agg.data_ptr(), O,
                                       na.data_ptr(), T, csr.deg.data_ptr(), spec.mean, spec.residual, N, gout.data_ptr(), gh.data_ptr(),
                                       g_agg.data_ptr(), g_na.data_ptr(), wsn.data_ptr(), bn, st))
    chk(L.csmpn_egcl_edge_backward_sig(e.metric_arr, e.n, e.params, e.grads, e.nblk, h.data_ptr(), C, ea.data_ptr(), A,
                                       csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), E, N, g_agg.data_ptr(),
                                       rows.data_ptr(), g_ea.data_ptr(), wse.data_ptr(), be, st))
    ops.segment_reduce(rows.view(E, C, D), gh.view(N, C, D), add=(csr.row_ptr, None), sub=csr.source_order())
    torch.cuda.synchronize()
    for key, (buf, view) in bufs.items():
        assert _intact(buf, view.numel()), key
    f = dict(f32=True)
    H.assert_close("stages.y", out.view(N, O, D).cpu().numpy(), c["truth"]["y"], yard["y"], **f)
    H.assert_close("stages.gh", gh.view(N, C, D).cpu().numpy(), c["truth"]["gh"], yard["gh"], **f)
    H.assert_close("stages.g_edge_attr", g_ea.view(E, A, D).cpu().numpy(), c["truth"]["g_edge_attr"], yard["g_edge_attr"], **f)
    H.assert_close("stages.g_node_attr", g_na.view(N, T, D).cpu().numpy(), c["truth"]["g_node_attr"], yard["g_node_attr"], **f)
    by_ptr = {p.data_ptr(): k for k, p in layer.named_parameters()}
    for model, params, views in (("edge_model", pe, ve), ("node_model", pn, vn)):
        for p_, v in zip(params, views):
            k = by_ptr[p_.data_ptr()]
            assert k.startswith(model)
            H.assert_close("stages.g/" + k, v.cpu().numpy(), c["truth"]["g/" + k], yard["g/" + k], **f)
    # the module gives the very bits of the direct calls (one call sequence)
    res = H.run_egcl(c, DEV, F32)
    assert np.array_equal(res["y"], out.view(N, O, D).cpu().numpy()) and np.array_equal(res["gh"], gh.view(N, C, D).cpu().numpy())


# ----------------------------------------------------------------------------------------------- 6. gradcheck

CL13 = H.SIGNATURES["cl13"]


def _first_host_passing_seed(make, host_fn):
    for seed in range(20):
        inputs = make(seed)
        try:
            if torch.autograd.gradcheck(host_fn, inputs, raise_exception=False):
                return seed, inputs
        except Exception:
            pass
    raise AssertionError("no seed passes gradcheck on the host formulation")


def test_gradcheck_cemlp_cl13(pkg):
    """torch.autograd.gradcheck at torch's float64 defaults on a Cl(1,3) CEMLP.double(), 2 -> 2 channels, 2 blocks, 3 rows; the
    inputs are the first seed for which the same call passes on the host through oracle/ref_path.py."""
    from csmpn_hip import ops
    from oracle import ref_path as O
    o = O.Algebra(list(CL13), F64)
    m = pkg.CEMLP(pkg.CliffordAlgebra(CL13), 2, 2, 2, n_layers=2).double()
    keys = [k for k, _ in m.named_parameters()]

    def make(seed):
        gen = torch.Generator().manual_seed(seed)
        p = O.init_cemlp_params(o, 2, 2, 2, 2, gen=gen, randomize=True, dtype=F64)
        return (torch.randn(3, 2, o.D, generator=gen, dtype=F64).requires_grad_(True), *[p[k].clone().requires_grad_(True) for k in keys])

    _seed, inputs = _first_host_passing_seed(make, lambda x, *ps: O.cemlp(o, x, dict(zip(keys, ps))))
    sd = m.state_dict()
    for k, v in zip(keys, inputs[1:]):
        sd[k] = v.detach().clone()
    m.load_state_dict(sd, strict=True)
    m = m.to(DEV)
    binding, flat = m.binding(), m.flat_params()
    order = [keys.index({p.data_ptr(): k for k, p in m.named_parameters()}[p.data_ptr()]) for p in flat]
    dev_in = [t.detach().to(DEV).requires_grad_(True) for t in inputs]

    def fn(x, *ps):
        return ops.cemlp_apply(x, binding, [ps[i] for i in order])

    assert torch.autograd.gradcheck(fn, dev_in)


def test_gradcheck_egcl_cl13(pkg):
    """gradcheck at torch's float64 defaults on a Cl(1,3) EGCL.double() at N = 5, E = 7, 2 channels (the graph of the sweep)."""
    from csmpn_hip import ops
    from oracle import ref_path as O
    o = O.Algebra(list(CL13), F64)
    c0 = H.small_egcl_case(CL13)
    ei = torch.from_numpy(c0["ei"])
    layer = pkg.EGCL(pkg.CliffordAlgebra(CL13), 2, 2, 2, aggr="mean").double()
    keys = [k for k, _ in layer.named_parameters()]
    assert sorted(keys) == sorted(c0["params"])

    def make(seed):
        gen = torch.Generator().manual_seed(seed)
        p = O.init_egcl_params(o, 2, 2, 2, gen=gen, randomize=True, dtype=F64)
        return (torch.randn(5, 2, o.D, generator=gen, dtype=F64).requires_grad_(True), *[p[k].clone().requires_grad_(True) for k in keys])

    _seed, inputs = _first_host_passing_seed(make, lambda h, *ps: O.egcl(o, h, ei, None, None, dict(zip(keys, ps)), aggr="mean"))
    sd = layer.state_dict()
    for k, v in zip(keys, inputs[1:]):
        sd[k] = v.detach().clone()
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(DEV)
    spec, csr = layer.spec(), ops.get_csr(ei.to(DEV), 5)
    flat = layer.edge_model.flat_params() + layer.node_model.flat_params()
    by_ptr = {p.data_ptr(): k for k, p in layer.named_parameters()}
    order = [keys.index(by_ptr[p.data_ptr()]) for p in flat]
    dev_in = [t.detach().to(DEV).requires_grad_(True) for t in inputs]

    def fn(h, *ps):
        return ops.egcl_apply(h, None, None, spec, csr, [ps[i] for i in order])

    assert torch.autograd.gradcheck(fn, dev_in)


# ----------------------------------------------------------------------------------------------- 7. equivariance on Cl(1,3)

def _compound(Q, n):
    """The action of the linear map Q (columns = images of the generators) on the blades, in blade order: the matrix of
    minors (compound matrices) of Q, grade by grade."""
    bm = H.blade_bitmaps(n)
    idx = [[b for b in range(n) if m >> b & 1] for m in bm]
    M = np.zeros((1 << n, 1 << n))
    for i, ri in enumerate(idx):
        for k, ck in enumerate(idx):
            if len(ri) == len(ck):
                M[i, k] = 1.0 if not ri else np.linalg.det(Q[np.ix_(ri, ck)])
    return M


def _lorentz_maps():
    ch, sh, a = np.cosh(0.5), np.sinh(0.5), 0.7
    boost = np.eye(4); boost[0, 0] = boost[1, 1] = ch; boost[0, 1] = boost[1, 0] = sh
    rot = np.eye(4); rot[2, 2] = rot[3, 3] = np.cos(a); rot[2, 3] = -np.sin(a); rot[3, 2] = np.sin(a)
    rot2 = np.eye(4); rot2[1, 1] = rot2[2, 2] = np.cos(0.4); rot2[1, 2] = -np.sin(0.4); rot2[2, 1] = np.sin(0.4)
    Q = boost @ rot @ rot2
    Tr = np.diag([-1.0, 1.0, 1.0, 1.0])
    eta = np.diag(CL13)
    for q in (Q, Tr @ Q):
        assert np.abs(q.T @ eta @ q - eta).max() < 1e-14
    return [("boost x rotation", Q), ("time reversal", Tr @ Q)]


def test_lorentz_equivariance_float64(pkg):
    """layer(rho(Q) x) against rho(Q) layer(x) on a Cl(1,3) EGCL in float64, Q a boost of rapidity 0.5 composed with rotations
    (Q^T eta Q = eta), then with a time reversal; rho(Q) acts on blades by the compound matrices of Q. The yardstick is the
    same measure for the host formulation (oracle/ref_path.py in float64); the rule is the float64 rule."""
    from oracle import ref_path as O
    o = O.Algebra(list(CL13), F64)
    c = H.small_egcl_case(CL13)
    P = H.F.pkg()
    layer = P.EGCL(P.CliffordAlgebra(CL13), 2, 2, 2, aggr="mean").double()
    sd = layer.state_dict()
    for k, v in c["params"].items():
        sd[k] = torch.from_numpy(v)
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(DEV)
    p = {k: torch.from_numpy(v) for k, v in c["params"].items()}
    h, ei = torch.from_numpy(c["h"]), torch.from_numpy(c["ei"])
    for tag, Q in _lorentz_maps():
        M = torch.from_numpy(_compound(Q, 4))
        rho = lambda x: torch.einsum("ik,...k->...i", M.to(x.device), x)
        with torch.no_grad():
            dev_a, dev_b = layer(rho(h).to(DEV), ei.to(DEV)).cpu(), rho(layer(h.to(DEV), ei.to(DEV)).cpu())
            host_a, host_b = O.egcl(o, rho(h), ei, None, None, p, aggr="mean"), rho(O.egcl(o, h, ei, None, None, p, aggr="mean"))
        assert float((dev_b - h).abs().max()) > 1e-2            # the layer and the map do something
        H.assert_close(f"equivariance/{tag}", dev_a.numpy(), dev_b.numpy(), H.err(host_a.numpy(), host_b.numpy()))
    # the guard: the compound matrix of a map that is NOT in O(1,3) does not commute with the layer
    Rbad = np.eye(4); Rbad[0, 0] = Rbad[1, 1] = np.cos(0.5); Rbad[0, 1] = -np.sin(0.5); Rbad[1, 0] = np.sin(0.5)
    M = torch.from_numpy(_compound(Rbad, 4))
    with torch.no_grad():
        a = layer(torch.einsum("ik,...k->...i", M, h).to(DEV), ei.to(DEV)).cpu()
        b = torch.einsum("ik,...k->...i", M, layer(h.to(DEV), ei.to(DEV)).cpu())
    assert H.err(a.numpy(), b.numpy()) > 1e-3


# ----------------------------------------------------------------------------------------------- 8. refusals

def test_refusals_on_the_device_launch_nothing(pkg):
    from csmpn_hip import native, ops
    alg = pkg.CliffordAlgebra(CL13)
    D = 16
    kernel_before = native.lib().csmpn_last_kernel()
    x = torch.zeros(3, 2, D, device=DEV)
    with pytest.raises(native.CsmpnError, match="above the limit of 64 channels of the run-time-signature kernels"):
        pkg.CEMLP(alg, 2, 65, 65).to(DEV)(x)
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        pkg.CEMLP(alg, 2, 2, 2).double().to(DEV)(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.CEMLP(alg, 2, 2, 2)(torch.zeros(3, 2, D))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.CEMLP(alg, 2, 2, 2).to(DEV)(torch.zeros(3, 2, D))
    layer = pkg.EGCL(alg, 2, 2, 2, edge_attr_features=1, aggr="mean").to(DEV)
    h, ei = torch.zeros(5, 2, D, device=DEV), torch.tensor([[0, 1, 2], [1, 2, 3]], device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        layer(h, ei, torch.zeros(3, 1, D))
    with pytest.raises(RuntimeError, match="mixed dtypes"):
        layer(h, ei, torch.zeros(3, 1, D, device=DEV, dtype=F64))
    spec, csr = layer.spec(), ops.get_csr(ei, 5)
    flat = layer.edge_model.flat_params() + layer.node_model.flat_params()
    with pytest.raises(native.CsmpnError, match="whole adjacency"):
        ops.egcl_apply(h, torch.zeros(2, 1, D, device=DEV), None, spec, ops.CsrSlice(csr, 0, 2), flat)
    for metric in [(1.0,) * 6, (1.0, -1.0, 0.5), (1.0, 0.0)]:
        a = pkg.CliffordAlgebra(metric)
        with pytest.raises(native.CsmpnError, match="metric not supported by the HIP path"):
            pkg.CEMLP(a, 2, 2, 2).to(DEV)(torch.zeros(3, 2, 1 << len(metric), device=DEV))
        with pytest.raises(native.CsmpnError, match="metric not supported by the HIP path"):
            pkg.CEMLP(a, 2, 2, 2).double().to(DEV)(torch.zeros(3, 2, 1 << len(metric), device=DEV, dtype=F64))
    torch.cuda.synchronize()
    assert native.lib().csmpn_last_kernel() == kernel_before


# ----------------------------------------------------------------------------------------------- 9. determinism, routing

def test_deterministic_requests_raise_no_warning_and_change_no_bit(pkg):
    from csmpn_hip import ops
    c = H.egcl_case("cl13", "sum_res1_ag1")
    base = H.run_egcl(c, DEV, F32)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ops.set_deterministic(True)
            hard = H.run_egcl(c, DEV, F32)
            ops.set_deterministic(None)
            torch.use_deterministic_algorithms(True)
            soft = H.run_egcl(c, DEV, F32)
    finally:
        torch.use_deterministic_algorithms(False)
        ops.set_deterministic(None)
    for k in base:
        assert np.array_equal(base[k], hard[k]) and np.array_equal(base[k], soft[k]), k


def test_compiled_algebras_keep_their_kernels(pkg):
    """A Cl(3,0) 8-channel float32 layer and a Cl(4,1) float64 layer name the kernels they named before this family existed."""
    from csmpn_hip import native
    H.run_egcl(H.compiled_case("egcl8", "cl30", "mean_res1_ag0"), DEV, F32)
    k32 = native.lib().csmpn_last_kernel().decode()
    assert "cemlp_cl" in k32 and "Alg<3, 0u>" in k32 and "sig" not in k32 and "f64" not in k32, k32
    H.run_egcl(H.compiled_case("egcl", "cl41", "mean_res1_ag0"), DEV, F64)
    k64 = native.lib().csmpn_last_kernel().decode()
    # (the name is kept per thread: autograd runs the backward on a thread of its own, this one saw the node forward last)
    assert k64 == "csmpn::f64::cemlp_f64_kernel<Cl(4,1), fwd> (mode 2, 2 blocks, 4 channels)", k64
