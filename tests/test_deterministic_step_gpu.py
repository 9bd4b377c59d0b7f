"""Bit-reproducible training steps: the deterministic forms of the standalone MVLinear backward and of the
type-attribute backward (csmpn_mvlinear_backward_det / csmpn_type_attr_backward_det: per-workgroup partial sums in scratch +
a fixed-order sum, no float atomics) against the float64 truth, their C-ABI contracts (NULL outputs, accumulation into
the gradient buffers, scratch that needs no initialisation), bit-identical repeated runs, and whole training steps of
the four task models under torch.use_deterministic_algorithms(True) + ops.set_deterministic(True): same bits run after
run, and still the reference's numbers."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_path as O

from det_step_helpers import KINDS, build, deterministic, fixture, load_batch
from test_hip_parity import check, dev
from test_model_harness import _check_against_fixture

pytestmark = pytest.mark.gpu

# (metric, in_features, out_features, subspaces): md17's feature_embedding, a head with per-grade weights, the first module
# of the hulls simplex embedding, NBA's feature_embedding; all with a bias
MV_SHAPES = {"md17": ((1.0, 1.0, 1.0), 35, 32, False), "head": ((1.0, 1.0, 1.0), 32, 10, True),
             "hulls": ((1.0,) * 5, 1, 28, False), "nba": ((1.0, 1.0), 43, 40, False)}
# one row; below the smallest slab (8 rows); an md17 batch; many slabs (64 rows each) with a partial last one
MV_ROWS = [1, 7, 940, 20_000]


@functools.lru_cache(maxsize=None)
def mv_case(name, rows):
    """Seeded inputs of one MVLinear backward (host, float32) and the float64 truth of d/dx, d/dW, d/dbias: computed
    once, shared by the tests below, never written."""
    metric, I, O_, sub = MV_SHAPES[name]
    n = len(metric)
    D, G = 1 << n, n + 1
    gen = torch.Generator().manual_seed(1000 * len(name) + rows)
    x = torch.randn(rows, I, D, generator=gen)
    w = torch.randn((O_, I, G) if sub else (O_, I), generator=gen)
    gy = torch.randn(rows, O_, D, generator=gen)
    alg = O.Algebra(list(metric), torch.float64)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    b64 = torch.zeros(1, O_, 1, dtype=torch.float64, requires_grad=True)
    (O.mv_linear(alg, x64, w64, b64) * gy.double()).sum().backward()
    truth = {"gx": x64.grad.numpy(), "gw": w64.grad.numpy(), "gb": b64.grad.reshape(-1).numpy()}
    return {"n": n, "I": I, "O": O_, "sub": 1 if sub else 0, "rows": rows, "x": x, "w": w, "gy": gy, "truth": truth}


class MvDevice:
    """The device side of one case: inputs uploaded once, csmpn_mvlinear_backward_det called straight through the C-ABI."""

    def __init__(self, case):
        from csmpn_hip import native
        self.c, self.lib = case, native.lib()
        self.x, self.w, self.gy = (case[k].to(dev()) for k in ("x", "w", "gy"))
        self.bytes = int(self.lib.csmpn_mvlinear_backward_det_bytes(case["n"], case["rows"], case["I"], case["O"], case["sub"]))
        assert self.bytes > 0 and self.bytes % 4 == 0

    def run(self, want_gx=True, want_gw=True, want_gb=True, pre_w=None, pre_b=None, fill=0.0):
        from csmpn_hip import native
        c = self.c
        ws = torch.full((self.bytes // 4,), fill, dtype=torch.float32, device=dev())
        gx = torch.full_like(self.x, float("nan")) if want_gx else None        # overwritten, whatever it held
        gw = (pre_w.clone() if pre_w is not None else torch.zeros_like(self.w)) if want_gw else None
        gb = (pre_b.clone() if pre_b is not None else torch.zeros(c["O"], device=dev())) if want_gb else None
        ptr = lambda t: None if t is None else t.data_ptr()
        native.check(self.lib.csmpn_mvlinear_backward_det(
            c["n"], self.x.data_ptr(), self.w.data_ptr(), self.gy.data_ptr(), c["rows"], c["I"], c["O"], c["sub"], ptr(gx), ptr(gw),
            ptr(gb), ws.data_ptr(), self.bytes, torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return gx, gw, gb


@pytest.mark.parametrize("rows", MV_ROWS)
@pytest.mark.parametrize("name", list(MV_SHAPES))
def test_mvlinear_det_backward_against_truth(pkg, name, rows):
    """d/dx, d/dW and d/dbias of csmpn_mvlinear_backward_det against the float64 oracle, at the yardstick and bound of the
    atomic path's test_mvlinear_standalone_large (check(): 1e-5 of the tensor's largest entry); then the contracts of the
    entry point, each held to the bits of that first run: bias only (g_weight = NULL), no d/dx (gx = NULL), accumulation
    into pre-filled gradient buffers, and a workspace full of NaN."""
    case = mv_case(name, rows)
    m = MvDevice(case)
    gx, gw, gb = m.run()
    tag = f"{name}.{rows}"
    check(tag + ".gx", gx.cpu().numpy(), case["truth"]["gx"])
    check(tag + ".gW", gw.cpu().numpy(), case["truth"]["gw"])
    check(tag + ".gb", gb.cpu().numpy(), case["truth"]["gb"])
    # stale scratch never reaches the result
    gx_n, gw_n, gb_n = m.run(fill=float("nan"))
    assert bool(torch.isfinite(gw_n).all()) and bool(torch.isfinite(gb_n).all()) and bool(torch.isfinite(gx_n).all())
    assert torch.equal(gw_n, gw) and torch.equal(gb_n, gb) and torch.equal(gx_n, gx)
    # a frozen weight: the bias still gets its gradient
    gx_b, none_w, gb_b = m.run(want_gw=False, fill=float("nan"))
    assert none_w is None and torch.equal(gb_b, gb) and torch.equal(gx_b, gx)
    check(tag + ".gb (g_weight = NULL)", gb_b.cpu().numpy(), case["truth"]["gb"])
    # no d/dx
    none_x, gw_x, gb_x = m.run(want_gx=False)
    assert none_x is None and torch.equal(gw_x, gw) and torch.equal(gb_x, gb)
    # the += contract: the fixed-order sum is added to what the buffers hold (one float32 add per element)
    gen = torch.Generator().manual_seed(5)
    pre_w, pre_b = torch.randn(gw.shape, generator=gen).to(dev()), torch.randn(gb.shape, generator=gen).to(dev())
    _, gw_p, gb_p = m.run(want_gx=False, pre_w=pre_w, pre_b=pre_b)
    assert torch.equal(gw_p, pre_w + gw) and torch.equal(gb_p, pre_b + gb)


def test_mvlinear_det_rejects_a_missing_or_small_workspace(pkg):
    from csmpn_hip import native
    m = MvDevice(mv_case("md17", 7))
    c, lib = m.c, native.lib()
    gw = torch.zeros_like(m.w)
    ws = torch.zeros(m.bytes // 4, device=dev())
    args = (c["n"], m.x.data_ptr(), m.w.data_ptr(), m.gy.data_ptr(), c["rows"], c["I"], c["O"], c["sub"], None, gw.data_ptr(), None)
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.csmpn_mvlinear_backward_det(*args, None, m.bytes, stream) == native.ERR_INVALID
    assert lib.csmpn_mvlinear_backward_det(*args, ws.data_ptr(), m.bytes - 4, stream) == native.ERR_INVALID
    assert b"workspace" in lib.csmpn_last_error()
    # rows == 0: nothing touched, no workspace needed
    assert lib.csmpn_mvlinear_backward_det(c["n"], None, None, None, 0, c["I"], c["O"], c["sub"], None, gw.data_ptr(), None, None, 0,
                                           stream) == 0
    torch.cuda.synchronize()
    assert float(gw.abs().max()) == 0.0


# ----------------------------------------------------------------------------- type attributes

TYPE_CASES = {"several-groups": (300, 2999), "one-node": (1, 0)}   # K = 3, 3 types: 85 rows per pass -> 39 workgroups, the last short


@functools.lru_cache(maxsize=None)
def type_case(name, bad_ids=False):
    """Seeded type ids, edges and incoming gradients; float64 truth of the table gradient from the composed torch ops
    (row gather of the table -> scalar blade -> gathers by source / target, md17_cssmpnn.py:122-133) for both gradients,
    the node gradient alone and the edge gradient alone."""
    S, E = TYPE_CASES[name]
    T, K, n = 3, 3, 3
    D = 1 << n
    gen = torch.Generator().manual_seed(17 + S)
    types = torch.randint(0, T, (S,), generator=gen)
    if bad_ids:   # out-of-range ids land in the first / last row of the table, as in the forward
        types[::7] = -2
        types[3::11] = T + 4
    ei = torch.randint(0, S, (2, E), generator=gen)
    g_node, g_edge = torch.randn(S, K, D, generator=gen), torch.randn(E, 2 * K, D, generator=gen)
    table = torch.randn(T, K, generator=gen).double().requires_grad_(True)
    feats = table.index_select(0, types.clamp(0, T - 1))
    node_attr = torch.cat((feats.unsqueeze(-1), torch.zeros(S, K, D - 1, dtype=torch.float64)), dim=-1)   # blade 0 = the feature
    edge_attr = torch.cat((node_attr.index_select(0, ei[0]), node_attr.index_select(0, ei[1])), dim=1)
    ln, le = (node_attr * g_node.double()).sum(), (edge_attr * g_edge.double()).sum()
    truth = {"both": torch.autograd.grad(ln + le, table, retain_graph=True)[0].numpy(),
             "node": torch.autograd.grad(ln, table, retain_graph=True)[0].numpy()}
    truth["edge"] = torch.autograd.grad(le, table)[0].numpy() if E else np.zeros((T, K))
    return {"T": T, "K": K, "n": n, "S": S, "E": E, "types": types.to(torch.int32), "src": ei[0].to(torch.int32).contiguous(),
            "dst": ei[1].to(torch.int32).contiguous(), "g_node": g_node, "g_edge": g_edge, "truth": truth}


class TypeDevice:
    def __init__(self, case):
        from csmpn_hip import native
        self.c, self.lib = case, native.lib()
        self.types, self.src, self.dst, self.g_node, self.g_edge = (case[k].to(dev()) for k in ("types", "src", "dst", "g_node", "g_edge"))
        self.bytes = int(self.lib.csmpn_type_attr_backward_det_bytes(case["T"], case["K"], case["S"], case["E"]))
        assert self.bytes > 0 and self.bytes % 4 == 0

    def run(self, which="both", pre=None, fill=0.0):
        from csmpn_hip import native
        c = self.c
        ws = torch.full((self.bytes // 4,), fill, dtype=torch.float32, device=dev())
        g_tab = pre.clone() if pre is not None else torch.zeros(c["T"], c["K"], device=dev())
        gn = self.g_node.data_ptr() if which in ("both", "node") else None
        ge = self.g_edge.data_ptr() if (which in ("both", "edge") and c["E"]) else None
        native.check(self.lib.csmpn_type_attr_backward_det(
            c["n"], c["T"], c["K"], self.types.data_ptr(), c["S"], self.src.data_ptr() if c["E"] else None,
            self.dst.data_ptr() if c["E"] else None, c["E"], gn, ge, g_tab.data_ptr(), ws.data_ptr(), self.bytes,
            torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return g_tab


def _type_close(got, truth):
    """The bound of test_type_attr_kernel_matches_composed_ops: 1e-5 of the largest entry of the table gradient."""
    err, scale = float(np.abs(got.double().cpu().numpy() - truth).max()), float(np.abs(truth).max())
    assert err <= 1e-5 * scale, (err, scale)


@pytest.mark.parametrize("bad_ids", [False, True], ids=["ids-in-range", "ids-clamped"])
@pytest.mark.parametrize("name", list(TYPE_CASES))
def test_type_attr_det_backward_against_truth(pkg, name, bad_ids):
    case = type_case(name, bad_ids)
    m = TypeDevice(case)
    which = ["both", "node", "edge"] if case["E"] else ["node"]
    for w in which:
        g = m.run(w)
        _type_close(g, case["truth"][w])
        g_nan = m.run(w, fill=float("nan"))          # stale scratch never reaches the result
        assert bool(torch.isfinite(g_nan).all()) and torch.equal(g_nan, g)
    pre = torch.arange(9, dtype=torch.float32, device=dev()).reshape(3, 3) - 4.0
    assert torch.equal(m.run(which[0], pre=pre), pre + m.run(which[0]))        # accumulated into g_table
    # the plain form on the same inputs: the same sums up to the order of the float32 additions
    from csmpn_hip import native
    g_atomic = torch.zeros(3, 3, device=dev())
    native.check(m.lib.csmpn_type_attr_backward(case["n"], 3, 3, m.types.data_ptr(), case["S"], m.src.data_ptr() if case["E"] else None,
                                                m.dst.data_ptr() if case["E"] else None, case["E"], m.g_node.data_ptr(),
                                                m.g_edge.data_ptr() if case["E"] else None, g_atomic.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    _type_close(g_atomic, case["truth"]["both" if case["E"] else "node"])


def test_type_attr_det_rejects_a_missing_or_small_workspace(pkg):
    from csmpn_hip import native
    m = TypeDevice(type_case("several-groups"))
    c, lib = m.c, native.lib()
    g_tab = torch.zeros(3, 3, device=dev())
    ws = torch.zeros(m.bytes // 4, device=dev())
    stream = torch.cuda.current_stream().cuda_stream
    args = (c["n"], 3, 3, m.types.data_ptr(), c["S"], m.src.data_ptr(), m.dst.data_ptr(), c["E"], m.g_node.data_ptr(), m.g_edge.data_ptr(),
            g_tab.data_ptr())
    assert lib.csmpn_type_attr_backward_det(*args, None, m.bytes, stream) == native.ERR_INVALID
    assert lib.csmpn_type_attr_backward_det(*args, ws.data_ptr(), m.bytes - 4, stream) == native.ERR_INVALID
    # no nodes and no edges: nothing touched, no workspace needed
    assert lib.csmpn_type_attr_backward_det(c["n"], 3, 3, None, 0, None, None, 0, m.g_node.data_ptr(), None, g_tab.data_ptr(), None, 0,
                                            stream) == 0
    torch.cuda.synchronize()
    assert float(g_tab.abs().max()) == 0.0


# ----------------------------------------------------------------------------- same bits, run after run

@pytest.mark.parametrize("name", list(MV_SHAPES))
def test_mvlinear_det_bit_reproducible(pkg, name):
    m = MvDevice(mv_case(name, MV_ROWS[-1]))
    first = m.run()
    for _ in range(4):
        again = m.run(fill=float("nan"))
        assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("which", ["both", "node", "edge"])
def test_type_attr_det_bit_reproducible(pkg, which):
    m = TypeDevice(type_case("several-groups"))
    first = m.run(which)
    for _ in range(4):
        assert torch.equal(first, m.run(which, fill=float("nan")))


def test_mvlinear_module_takes_the_deterministic_form_under_a_request(pkg):
    """Through the nn.Module and autograd: under ops.set_deterministic(True) the backward of a standalone MVLinear calls
    csmpn_mvlinear_backward_det (ops.det_launches() counts it) and repeats its bits; its numbers are the truth's."""
    case = mv_case("md17", MV_ROWS[-1])
    lin = pkg.MVLinear(pkg.CliffordAlgebra((1.0, 1.0, 1.0)), case["I"], case["O"], subspaces=False).to(dev())
    with torch.no_grad():
        lin.weight.copy_(case["w"])
    x, gy = case["x"].to(dev()).requires_grad_(True), case["gy"].to(dev())
    with deterministic(torch_flag=False, request=True) as ops:
        runs = []
        for _ in range(5):
            n0 = ops.det_launches()
            lin.weight.grad = lin.bias.grad = x.grad = None
            (lin(x) * gy).sum().backward()
            assert ops.det_launches() == n0 + 1
            runs.append((x.grad.clone(), lin.weight.grad.clone(), lin.bias.grad.clone()))
    for r in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], r))
    check("module.gW", runs[0][1].cpu().numpy(), case["truth"]["gw"])
    check("module.gb", runs[0][2].reshape(-1).cpu().numpy(), case["truth"]["gb"])


def test_standalone_cemlp_request_on_a_shape_without_deterministic_kernels(pkg, monkeypatch):
    """A standalone CEMLP now carries the request to csmpn_cemlp_forward / _backward. Cl(5,0) at 12 channels runs on the
    general kernels, which have no deterministic form for n >= 4: a hard request raises, a soft one (inherited from
    torch.use_deterministic_algorithms) warns once and repeats the call without the flag - the numbers of no request."""
    from csmpn_hip import native
    torch.manual_seed(2)
    m = pkg.CEMLP(pkg.CliffordAlgebra((1.0,) * 5), 12, 12, 12, n_layers=1).to(dev())
    gen = torch.Generator().manual_seed(4)
    x, gy = torch.randn(50, 12, 32, generator=gen).to(dev()), torch.randn(50, 12, 32, generator=gen).to(dev())

    def once():
        m.zero_grad(set_to_none=True)
        xx = x.clone().requires_grad_(True)
        y = m(xx)
        (y * gy).sum().backward()
        return [y.detach().clone(), xx.grad.clone()] + [p.grad.clone() for p in m.parameters()]

    with deterministic(torch_flag=False, request=None):
        want = once()
    with deterministic(torch_flag=False, request=True):
        with pytest.raises(native.CsmpnError, match="DETERMINISTIC"):
            once()
    with deterministic(torch_flag=True, request=None) as ops:
        monkeypatch.delenv("CSMPN_DETERMINISTIC", raising=False)
        monkeypatch.setattr(ops, "_warned_soft_det", False)
        assert ops.deterministic_request() == "soft"
        with pytest.warns(UserWarning, match="deterministic aggregation is not available"):
            got = once()
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12


# ----------------------------------------------------------------------------- whole training steps

def _step(model, batch):
    loss, parts = model(batch)
    loss.backward()
    grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
    return loss.detach().clone(), {k: v.detach().clone() for k, v in parts.items()}, grads


def _same_bits(a, b, what):
    (la, pa, ga), (lb, pb, gb) = a, b
    assert torch.equal(la, lb), f"{what}: loss"
    assert sorted(pa) == sorted(pb) and all(torch.equal(pa[k], pb[k]) for k in pa), f"{what}: parts"
    assert sorted(ga) == sorted(gb)
    for k in ga:
        assert (ga[k] is None) == (gb[k] is None), k
        assert ga[k] is None or torch.equal(ga[k], gb[k]), f"{what}: gradient of {k}"


@pytest.mark.parametrize("kind", KINDS)
def test_model_step_bit_reproducible(pkg, kind):
    """Forward + backward of a task model on the parameters and batch of tests/golden/model_<kind>.npz, five times from the
    same state under torch.use_deterministic_algorithms(True) and ops.set_deterministic(True) (a hard request: an op
    without a deterministic form raises): loss, every loss part and every parameter gradient identical bit for bit; the
    models with type attributes / standalone MVLinears take the _det entry points; and the step still passes the fixture
    comparison of test_model_fixture_gpu at that test's tolerances."""
    g = fixture(kind)
    with deterministic(torch_flag=True, request=True) as ops:
        model = build(pkg, kind, g, dev())
        batch = load_batch(pkg, g, device=dev())
        runs = []
        for _ in range(5):
            model.zero_grad(set_to_none=True)
            n0 = ops.det_launches()
            runs.append(_step(model, batch))
            if kind != "hulls":
                assert ops.det_launches() >= n0 + 1, "the deterministic entry points did not run"
        torch.cuda.synchronize()
    for i, r in enumerate(runs[1:]):
        _same_bits(runs[0], r, f"{kind}, run {i + 1}")
    loss, parts, _ = runs[-1]
    _check_against_fixture(g, loss, parts, model, tol=3e-5 if kind == "nba" else 1e-5)


def test_md17_step_bit_reproducible_with_fused_grad_accumulation(pkg):
    """The same through ops.set_fused_grad_accumulation(True): the fixed-order sums are added into p.grad in place."""
    g = fixture("md17")
    with deterministic(torch_flag=True, request=True) as ops:
        model = build(pkg, "md17", g, dev())
        batch = load_batch(pkg, g, device=dev())
        for p in model.parameters():
            p.grad = torch.zeros_like(p)
        ops.set_fused_grad_accumulation(True)
        try:
            runs = []
            for _ in range(2):
                model.zero_grad(set_to_none=False)
                n0 = ops.det_launches()
                runs.append(_step(model, batch))
                assert ops.det_launches() >= n0 + 1
        finally:
            ops.set_fused_grad_accumulation(False)
        torch.cuda.synchronize()
    _same_bits(runs[0], runs[1], "md17, fused accumulation")
    _check_against_fixture(g, runs[1][0], runs[1][1], model, tol=1e-5)


def test_replayed_hulls_steps_bit_reproducible(pkg):
    """Two GraphedTrainStep instances of the hulls model from the same initial state, three replayed steps each (forward,
    backward, fused Adam over one flat parameter) under the request: same losses, same final parameters, bit for bit."""
    from csmpn_hip.graphed import GraphedTrainStep, flatten_parameters
    g = fixture("hulls")

    def advance():
        model = build(pkg, "hulls", g, dev())
        batch = load_batch(pkg, g, device=dev())
        flat = flatten_parameters(model)
        opt = torch.optim.Adam([flat], lr=1e-3, capturable=True, fused=True)
        gs = GraphedTrainStep(model, opt, batch, ["input", "target"])
        losses = [gs.step().detach().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in model.parameters()]

    with deterministic(torch_flag=True, request=True):
        (la, pa), (lb, pb) = advance(), advance()
    assert all(torch.equal(a, b) for a, b in zip(la, lb)), (la, lb)
    assert len(pa) == len(pb) and all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert not torch.equal(la[0], la[2])            # the steps did move the parameters


def test_default_path_takes_no_deterministic_entry_point(pkg, monkeypatch):
    """No request, torch's flag off: an md17 step makes the calls it made before (the plain backward forms)."""
    monkeypatch.delenv("CSMPN_DETERMINISTIC", raising=False)
    g = fixture("md17")
    with deterministic(torch_flag=False, request=None) as ops:
        assert ops.deterministic_request() is None
        model = build(pkg, "md17", g, dev())
        n0 = ops.det_launches()
        loss, parts, _ = _step(model, load_batch(pkg, g, device=dev()))
        torch.cuda.synchronize()
        assert ops.det_launches() == n0
    _check_against_fixture(g, loss, parts, model, tol=1e-5)
