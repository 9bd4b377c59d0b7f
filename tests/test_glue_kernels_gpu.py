"""The kernels either side of the message passing (csrc/glue.hip: csmpn_simplex_rows, csmpn_readout_mse_*,
csmpn_readout_traj_*, csmpn_type_attr_*) against the float64 references of tests/glue_helpers.py at their loop and shape
edges - the cases and what each reaches are listed there; tests/test_glue_reference_cpu.py validates the references against
the fixtures of the imported reference models first.

Bound: per tensor relmax(got, truth) <= max(1e-5, 4 x the float32 run of the same reference), every element
within 10 x that bound of |truth| + 0.1 max|truth|; equality where an operation only moves data (simplex rows, the
type-attribute forward) and for every element no arithmetic reaches (`glue_helpers.traj_exact_zeros`, the filler rows and
the blades >= 1 of the MSE readout). Each forward and backward of the readouts runs twice and must repeat its bits (fixed
order sums, no atomics); so must csmpn_type_attr_backward_det, also on scratch full of NaN.

Everything runs in-process: through csmpn_hip.ops, and through the C-ABI where ops cannot express an argument (a null
incoming gradient, edges without node rows, invalid sizes) and to see what the kernels write: every output of a C-ABI call
is a view into a larger allocation, the words either side hold a sentinel and the interior NaN (buffers the kernels ADD
into - the weight and table gradients - hold finite numbers); afterwards the sentinels are intact and no NaN is left.
No call passes an index table the kernels do not validate (vrows, trow, vptr, graph_ptr) with an entry out of range.

test_*_can_fail: a COPY of a stored kernel result is mutated the way an index bug would leave it and the comparison it
belongs to must reject it.

Every test prints `glue <case> <tensor> err=<relmax to float64> yard=<float32 reference>` (pytest -s).
"""
import numpy as np
import pytest
import torch

import glue_helpers as G

pytestmark = pytest.mark.gpu
GUARD, PAD = -77.0, 64
BOTH = ("graph", "vertex")


def dev():
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """A float32 tensor of `shape` inside a larger allocation of sentinels; the interior starts as `fill`."""

    def __init__(self, shape, fill=float("nan")):
        n = int(np.prod(shape))
        self.whole = torch.full((n + 2 * PAD,), GUARD, dtype=torch.float32, device=dev())
        self.t = self.whole[PAD:PAD + n].view(shape)
        self.t.copy_(fill) if isinstance(fill, torch.Tensor) else self.t.fill_(fill)
        self.n = n

    def ok(self, written=True):
        torch.cuda.synchronize()
        intact = bool((self.whole[:PAD] == GUARD).all()) and bool((self.whole[PAD + self.n:] == GUARD).all())
        return intact and (not written or not bool(torch.isnan(self.t).any()))


def report(case, figures):
    for k, (err, yard) in figures.items():
        print(f"glue {case} {k} err={err:.2e} yard={yard:.2e}")


def same_bits(a, b):
    return a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


# ================================================================================================ trajectory readout
class Traj:
    def __init__(self, tag, target=None):
        from csmpn_hip import ops
        self.tag, self.inp = tag, G.traj_inputs(tag)
        i = self.inp
        d = lambda t: None if t is None else t.to(dev())
        self.x, self.w, self.loc, self.gg, self.gv = d(i["x"]), d(i["weight"]), d(i["loc"]), d(i["g_graph"]), d(i["g_vertex"])
        self.target = d(i["target"]) if target is None else target
        self.want = G.traj_tables_loop(i["sizes"], i["vrows"], i["n_rows"], i["unscored_last"])
        kw = dict(unscored_last=i["unscored_last"])
        if i["vrows"] is not None:
            kw.update(vertex_rows=d(i["vrows"]), n_rows=i["n_rows"])
        self.tables = ops.readout_traj_tables(d(self.want["graph_of_vertex"].long()), len(i["sizes"]), **kw)
        for k, w in self.want.items():     # the tables the kernels index with are the loop construction's: all in range
            assert (w is None) == (self.tables[k] is None) and (w is None or torch.equal(self.tables[k].cpu(), w)), (tag, k)

    def ops(self, use=BOTH):
        from csmpn_hip import ops
        x, w = self.x.clone().requires_grad_(True), self.w.clone().requires_grad_(True)
        pg, pv, pred = ops.readout_traj(x, w, self.loc, self.target, self.tables, self.inp["n"])
        total = ((pg * self.gg).sum() if "graph" in use else 0) + ((pv * self.gv).sum() if "vertex" in use else 0)
        gx, gw = torch.autograd.grad(total, [x, w])
        torch.cuda.synchronize()
        return {"pred": pred.detach(), "per_graph": pg.detach(), "per_vertex": pv.detach(), "gx": gx, "gw": gw}

    def cabi(self, use=BOTH):
        """Forward and backward through the C-ABI into guarded buffers; a part of the loss that is not in `use` passes a
        null incoming gradient."""
        from csmpn_hip import native
        lib, i, t = native.lib(), self.inp, self.tables
        S, C, D = self.x.shape
        O, n, V, B = self.w.shape[0], i["n"], sum(i["sizes"]), len(i["sizes"])
        pred, pg, pv = Guarded((V, O, n)), Guarded((B, 3)), Guarded((V,))
        native.check(lib.csmpn_readout_traj_forward(n, self.x.data_ptr(), C, ptr(t["vrows"]), V, self.w.data_ptr(), O, self.w.shape[2],
                                                    ptr(self.loc), self.target.data_ptr(), ptr(t["trow"]), t["vptr"].data_ptr(), B,
                                                    pred.t.data_ptr(), pg.t.data_ptr(), pv.t.data_ptr(), stream()))
        assert pred.ok() and pg.ok() and pv.ok(), (self.tag, "forward wrote outside its outputs or left an element unwritten")
        scratch, gx, gw = Guarded((V, O, n)), Guarded((S, C, D)), Guarded(tuple(self.w.shape), 0.0)
        native.check(lib.csmpn_readout_traj_backward(
            n, self.x.data_ptr(), C, S, ptr(t["vrows"]), ptr(t["vertex_of_row"]), V, self.w.data_ptr(), O, self.w.shape[2],
            pred.t.data_ptr(), self.target.data_ptr(), ptr(t["trow"]), t["graph_of_vertex"].data_ptr(), t["vptr"].data_ptr(),
            ptr(self.gg) if "graph" in use else None, ptr(self.gv) if "vertex" in use else None, scratch.t.data_ptr(),
            gx.t.data_ptr(), gw.t.data_ptr(), stream()))
        assert scratch.ok() and gx.ok() and gw.ok(), (self.tag, "backward wrote outside its outputs or left an element unwritten")
        return {"pred": pred.t.clone(), "per_graph": pg.t.clone(), "per_vertex": pv.t.clone(), "gx": gx.t.clone(), "gw": gw.t.clone()}


def check_traj(name, inp, got, truth, ref32):
    figures = G.compare(name, got, truth, ref32)
    G.traj_exact_zeros(inp, got)
    report(name, figures)
    return figures


@pytest.mark.parametrize("tag", sorted(G.TRAJ_CASES))
def test_traj_readout_against_float64(pkg, tag):
    """pred, per_graph, per_vertex, d/dx and d/d weight under incoming gradients on per_graph and per_vertex together,
    through ops (autograd) and through the C-ABI (guarded buffers): the same bits both ways and run after run."""
    m = Traj(tag)
    truth, ref32 = G.traj_truth(tag)
    first = m.ops()
    check_traj(tag, m.inp, first, truth, ref32)
    assert same_bits(first, m.ops()), "a second run through ops differs"
    raw = m.cabi()
    assert same_bits(first, raw), "the C-ABI call differs from the call through ops"
    assert same_bits(raw, m.cabi())


@pytest.mark.parametrize("use", ["graph", "vertex"])
@pytest.mark.parametrize("tag", G.TRAJ_ALONE)
def test_traj_readout_one_incoming_gradient(pkg, tag, use):
    """per_graph alone and per_vertex alone: the other incoming gradient is a null pointer (C-ABI)."""
    m = Traj(tag)
    truth, ref32 = G.traj_truth(tag, (use,))
    got = m.cabi((use,))
    check_traj(f"{tag}-{use}", m.inp, got, truth, ref32)
    assert same_bits(got, m.cabi((use,)))
    through_ops = m.ops((use,))        # autograd hands the unused part a gradient of zeros: the same numbers, not the same branch
    check_traj(f"{tag}-{use}-ops", m.inp, through_ops, truth, ref32)


def test_traj_readout_zero_distance(pkg):
    """|d| = 0 (the `inv = nr > 0 ? 1 / nr : 0` branch of the ADE / FDE gradient): the targets of one whole scored vertex
    of T5 and of one further (vertex, out channel) are the float32 predictions of a first run; the kernel recomputes them
    in the same order, so d = 0 exactly there. Everything finite, and the float64 reference under the subgradient-0
    convention (glue_helpers.traj_forward) is met."""
    first = Traj("T5")
    pred = first.ops()["pred"]
    scored, _ = G.scored_vertices(first.inp["sizes"], first.inp["unscored_last"])
    pos = {v: k for k, v in enumerate(scored)}
    target = first.target.clone()
    for v, o in G.T5_TIES:
        target[pos[v], o] = pred[v, o]
    m = Traj("T5", target=target)
    truth, ref32 = G.traj_truth("T5", BOTH, G.T5_TIES)
    got = m.ops()
    assert torch.equal(got["pred"], pred)
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    check_traj("T5-ties", m.inp, got, truth, ref32)
    v = G.T5_TIES[0][0]
    assert float(got["per_vertex"][v]) == 0.0 and bool((got["gx"][int(m.inp["vrows"][v])] == 0).all()), "d is not exactly 0"
    assert same_bits(got, m.cabi())
    for use in ("graph", "vertex"):
        t64, t32 = G.traj_truth("T5", (use,), G.T5_TIES)
        check_traj(f"T5-ties-{use}", m.inp, m.cabi((use,)), t64, t32)


def test_traj_readout_invalid_arguments(pkg):
    """Sizes outside the kernels' limits and inconsistent row tables are refused before any launch: nothing is written."""
    from csmpn_hip import native
    lib = native.lib()
    m = Traj("T5")
    i, t = m.inp, m.tables
    S, V, B = i["n_rows"], sum(i["sizes"]), len(i["sizes"])
    outs = [Guarded((V * 32 * 3,)) for _ in range(6)]
    o = [g.t.data_ptr() for g in outs]

    def fwd(C, O, stride, n_graphs=B):
        return lib.csmpn_readout_traj_forward(3, m.x.data_ptr(), C, ptr(t["vrows"]), V, m.w.data_ptr(), O, stride, ptr(m.loc),
                                              m.target.data_ptr(), ptr(t["trow"]), t["vptr"].data_ptr(), n_graphs, o[0], o[1], o[2], stream())

    def bwd(C, O, stride, vrows=t["vrows"], vof=t["vertex_of_row"], n_rows=S):
        return lib.csmpn_readout_traj_backward(3, m.x.data_ptr(), C, n_rows, ptr(vrows), ptr(vof), V, m.w.data_ptr(), O, stride, o[0],
                                               m.target.data_ptr(), ptr(t["trow"]), t["graph_of_vertex"].data_ptr(), t["vptr"].data_ptr(),
                                               ptr(m.gg), ptr(m.gv), o[3], o[4], o[5], stream())

    for C, O, stride in ((65, 32, 4), (1, 1025, 4), (17, 241, 4), (1, 32, 1)):
        assert fwd(C, O, stride) == native.ERR_UNSUPPORTED, (C, O, stride)
        assert bwd(C, O, stride) == native.ERR_UNSUPPORTED, (C, O, stride)
    assert bwd(1, 32, 4, vof=None) == native.ERR_INVALID             # vertex_rows without vertex_of_row
    assert bwd(1, 32, 4, vrows=None) == native.ERR_INVALID           # ... and the other way round
    assert bwd(1, 32, 4, vrows=None, vof=None) == native.ERR_INVALID   # identity rows with n_rows != n_vertices
    assert S != V and fwd(1, 32, 4, n_graphs=0) == 0                 # no graph: OK, nothing written
    for g in outs:
        assert g.ok(written=False) and bool(torch.isnan(g.t).all())


def test_traj_comparisons_can_fail(pkg):
    """Mutations of copies of stored results, each of the kind an index bug of the named path would leave."""
    m = Traj("T2")
    truth, ref32 = G.traj_truth("T2")
    got = m.ops()
    G.compare("T2", got, truth, ref32)

    def rejected(key, mutate, by=G.compare):
        bad = {key: got[key].clone()}
        mutate(bad[key])
        with pytest.raises(AssertionError):
            by("T2", bad, truth, ref32) if by is G.compare else by(m.inp, bad)

    def second_pass_from_first(pv):          # vper = 25: the vertices 25..49 of graph 0 are its second pass
        pv[25:50] = got["per_vertex"][0:25]
    rejected("per_vertex", second_pass_from_first)

    def swap_ade_fde(pg):
        pg[:, 1], pg[:, 2] = got["per_graph"][:, 2], got["per_graph"][:, 1]
    rejected("per_graph", swap_ade_fde)

    def drop_out_channel(gw):
        gw[17] = 0
    rejected("gw", drop_out_channel)
    no_vertex = sorted(set(range(m.inp["n_rows"])) - set(m.inp["vrows"].tolist()))

    def touch_a_row_that_is_no_vertex(gx):
        gx[no_vertex[2], 3, 1] = 1e-3
    rejected("gx", touch_a_row_that_is_no_vertex, by=G.traj_exact_zeros)


# ======================================================================================================= MSE readout
def mse_cabi(tag, wl):
    """csmpn_readout_mse_forward / _backward into guarded buffers; coef as ops forms it (glue.hip: g_loss 2 (pred - target)
    / max(cnt, 1))."""
    from csmpn_hip import native
    lib, i = native.lib(), G.mse_inputs(tag)
    x, w, ptr32, tgt = i["x"].to(dev()), i["weight"].to(dev()), i["ptr"].to(dev()), i["target"].to(dev())
    b = None if i["bias"] is None else i["bias"].to(dev())
    S, C, D = x.shape
    B = len(i["sizes"])
    stride = w.shape[2] if w.dim() == 3 else 1
    pred, loss, xs = Guarded((B,)), Guarded((B,)), Guarded((B, C))
    native.check(lib.csmpn_readout_mse_forward(i["n"], x.data_ptr(), w.data_ptr(), stride, ptr(b), S, C, ptr32.data_ptr(), B,
                                               tgt.data_ptr(), pred.t.data_ptr(), loss.t.data_ptr(), xs.t.data_ptr(), stream()))
    assert pred.ok() and loss.ok() and xs.ok(), tag
    cnt = (ptr32[1:] - ptr32[:-1]).clamp(min=1).float()
    coef = (wl * 2.0 * (pred.t - tgt) / cnt).contiguous()
    gx = Guarded((S, C, D))
    native.check(lib.csmpn_readout_mse_backward(i["n"], w.data_ptr(), stride, S, C, ptr32.data_ptr(), B, coef.data_ptr(),
                                                gx.t.data_ptr(), stream()))
    assert gx.ok(), tag
    return {"pred": pred.t.clone(), "loss": loss.t.clone(), "gx": gx.t.clone()}


def mse_ops(tag):
    from csmpn_hip import ops
    i = G.mse_inputs(tag)
    x, w = i["x"].to(dev()).requires_grad_(True), i["weight"].to(dev()).requires_grad_(True)
    b = None if i["bias"] is None else i["bias"].to(dev()).requires_grad_(True)
    loss, pred = ops.readout_mse(x, w, b, i["ptr"].to(dev()), i["target"].to(dev()), i["n"])
    grads = torch.autograd.grad((loss * i["wl"].to(dev())).sum(), [x, w] + ([b] if b is not None else []))
    torch.cuda.synchronize()
    out = {"loss": loss.detach(), "pred": pred.detach(), "gx": grads[0], "gw": grads[1]}
    if b is not None:
        out["gb"] = grads[2]
    return out


@pytest.mark.parametrize("tag", sorted(G.MSE_CASES))
def test_mse_readout_against_float64(pkg, tag):
    """loss, pred, d/dx, d/d weight, d/d bias under a random loss weight per graph."""
    i = G.mse_inputs(tag)
    truth, ref32 = G.mse_truth(tag)
    got = mse_ops(tag)
    assert got.keys() == truth.keys()
    report(tag, G.compare(tag, got, truth, ref32))
    gx, rows = got["gx"].cpu(), sum(i["sizes"])
    assert gx.shape[0] - rows == G.MSE_CASES[tag]["filler"]
    assert bool((gx[:, :, 1:] == 0).all()) and bool((gx[rows:] == 0).all()), "d/dx off blade 0 or on the filler rows"
    gw = got["gw"].cpu()
    assert gw.dim() == 2 or bool((gw[:, :, 1:] == 0).all())
    for b, s in enumerate(i["sizes"]):
        if s == 0:     # an empty graph: pred exactly 0, loss exactly target^2 (one float32 product)
            assert float(got["pred"][b]) == 0.0 and float(got["loss"][b]) == float(i["target"][b] * i["target"][b]), (tag, b)
    assert same_bits(got, mse_ops(tag))
    raw = mse_cabi(tag, i["wl"].to(dev()))
    assert same_bits(raw, {k: got[k] for k in raw}), "the C-ABI calls differ from the calls through ops"
    assert same_bits(raw, mse_cabi(tag, i["wl"].to(dev())))


def test_mse_comparison_can_fail(pkg):
    """The third stride of M1's largest graph (rows 512.. of 600) missing from its mean; a filler row touched."""
    i = G.mse_inputs("M1")
    truth, ref32 = G.mse_truth("M1")
    got = mse_ops("M1")
    w, lo = i["weight"][0, :, 0].double(), 84 + 257 + 1
    bad = got["pred"].detach().clone()
    bad[4] -= float((i["x"][lo + 512:lo + 600, :, 0].double() @ w).sum() / 600)
    with pytest.raises(AssertionError):
        G.compare("M1", {"pred": bad}, truth, ref32)
    gx = got["gx"].clone()
    gx[sum(i["sizes"]) + 1, 2, 0] = 1e-3
    assert not bool((gx[sum(i["sizes"]):] == 0).all())


# =================================================================================================== type attributes
class Attr:
    def __init__(self, tag, bad_ids=False):
        from csmpn_hip import native
        self.tag, self.inp, self.lib = tag, G.attr_inputs(tag, bad_ids), native.lib()
        i = self.inp
        d = lambda t: None if t is None else t.to(dev())
        self.table, self.types, self.src, self.dst = d(i["table"]), d(i["types"]), d(i["src"]), d(i["dst"])
        self.g_node = d(i["g_node"]) if i["S"] else None
        self.g_edge = d(i["g_edge"]) if i["E"] else None
        self.base = d(i["base"])
        self.bytes = int(self.lib.csmpn_type_attr_backward_det_bytes(i["T"], i["K"], i["S"], i["E"]))
        assert self.bytes > 0 and self.bytes % 4 == 0

    def forward(self):
        from csmpn_hip import native
        i = self.inp
        node = Guarded((i["S"], i["K"], i["D"])) if i["S"] else None
        edge = Guarded((i["E"], 2 * i["K"], i["D"])) if i["E"] else None
        native.check(self.lib.csmpn_type_attr_forward(i["n"], self.table.data_ptr(), i["T"], i["K"], self.types.data_ptr(), i["S"],
                                                      ptr(self.src), ptr(self.dst), i["E"], node.t.data_ptr() if node else None,
                                                      edge.t.data_ptr() if edge else None, stream()))
        assert (node is None or node.ok()) and (edge is None or edge.ok()), self.tag
        return node.t if node else torch.zeros(0, i["K"], i["D"]), edge.t if edge else torch.zeros(0, 2 * i["K"], i["D"])

    def backward(self, use, det, pre=None, fill=0.0):
        """g_table (accumulated into `pre`) of the plain or the deterministic entry point; a part not in `use` passes null."""
        from csmpn_hip import native
        i = self.inp
        tab = Guarded((i["T"], i["K"]), pre if pre is not None else 0.0)
        gn = ptr(self.g_node) if "node" in use else None
        ge = ptr(self.g_edge) if "edge" in use else None
        head = (i["n"], i["T"], i["K"], self.types.data_ptr(), i["S"], ptr(self.src), ptr(self.dst), i["E"], gn, ge, tab.t.data_ptr())
        if det:
            ws = Guarded((self.bytes // 4,), fill)
            native.check(self.lib.csmpn_type_attr_backward_det(*head, ws.t.data_ptr(), self.bytes, stream()))
            assert ws.ok(written=False), (self.tag, "scratch overrun")
        else:
            native.check(self.lib.csmpn_type_attr_backward(*head, stream()))
        assert tab.ok(), self.tag
        return tab.t.clone()

    def uses(self):
        """Both gradients, the node gradient alone, the edge gradient alone; one run where a case has one kind of row only
        (the missing kind's gradient is a null pointer there)."""
        return [("node", "edge"), ("node",), ("edge",)] if self.inp["S"] and self.inp["E"] else [("node", "edge")]


def attr_compare(name, got, inp, use, base=None):
    t64, t32 = G.attr_backward(inp, torch.float64, use), G.attr_backward(inp, torch.float32, use)
    if base is not None:
        t64, t32 = t64 + base.double(), t32 + base
    err = G.check(name, got.double().cpu().numpy(), t64.numpy(), t32.double().numpy(), 4.0)
    print(f"glue {name} g_table err={err:.2e} yard={G.relmax(t32.double().numpy(), t64.numpy()):.2e}")


def check_attr(m):
    i, tag = m.inp, m.tag
    node, edge = m.forward()
    want_node, want_edge = G.attr_forward(i)
    assert torch.equal(node.cpu(), want_node) and torch.equal(edge.cpu(), want_edge), tag
    assert bool((node[..., 1:] == 0).all()) and bool((edge[..., 1:] == 0).all())
    for use in m.uses():
        name = f"{tag}-{'+'.join(use)}"
        attr_compare(name + "-plain", m.backward(use, det=False), i, use)
        det = m.backward(use, det=True)
        attr_compare(name + "-det", det, i, use)
        assert torch.equal(det, m.backward(use, det=True)), "the deterministic form does not repeat its bits"
        again = m.backward(use, det=True, fill=float("nan"))       # stale scratch never reaches the result
        assert bool(torch.isfinite(again).all()) and torch.equal(det, again)
    use = m.uses()[0]
    for det in (False, True):        # accumulation into a pre-filled g_table
        attr_compare(f"{tag}-prefilled-{'det' if det else 'plain'}", m.backward(use, det=det, pre=m.base), i, use, base=i["base"])


@pytest.mark.parametrize("tag", sorted(G.ATTR_CASES))
def test_type_attr_against_float64(pkg, tag):
    check_attr(Attr(tag))


def test_type_attr_clamped_ids(pkg):
    """A1 with ids of -2 and T + 4 among the types: clamped into [0, T) both ways."""
    m = Attr("A1", bad_ids=True)
    ty = m.inp["types"]
    assert int((ty < 0).sum()) > 0 and int((ty >= m.inp["T"]).sum()) > 0
    check_attr(m)


@pytest.mark.parametrize("tag", [t for t in sorted(G.ATTR_CASES) if G.ATTR_CASES[t]["S"]])
def test_type_attr_through_ops(pkg, tag):
    """ops.type_attr_apply and its autograd backward, plain and under ops.set_deterministic(True)."""
    from csmpn_hip import ops
    m = Attr(tag)
    i = m.inp
    empty = torch.empty(0, dtype=torch.int32, device=dev())
    want_node, want_edge = G.attr_forward(i)
    for det in (False, True):
        ops.set_deterministic(True if det else None)
        try:
            table = m.table.clone().requires_grad_(True)
            node, edge = ops.type_attr_apply(table, m.types, m.src if i["E"] else empty, m.dst if i["E"] else empty, i["n"])
            assert torch.equal(node.cpu(), want_node) and torch.equal(edge.cpu(), want_edge)
            total = (node * m.g_node).sum() + ((edge * m.g_edge).sum() if i["E"] else 0)
            (g,) = torch.autograd.grad(total, table)
            torch.cuda.synchronize()
        finally:
            ops.set_deterministic(None)
        attr_compare(f"{tag}-ops-{'det' if det else 'plain'}", g, i, ("node", "edge"))


def test_type_attr_too_many_bins(pkg):
    """T K = 65 > kTypeBins: CSMPN_ERR_INVALID from all three entry points, the scratch query answers 0, nothing written."""
    from csmpn_hip import native
    m = Attr("A5")
    i, lib = m.inp, m.lib
    out = [Guarded((4096,)) for _ in range(4)]
    o = [g.t.data_ptr() for g in out]
    T, K = 13, 5
    assert lib.csmpn_type_attr_forward(i["n"], m.table.data_ptr(), T, K, m.types.data_ptr(), i["S"], None, None, 0, o[0], o[1], stream()) == native.ERR_INVALID
    assert lib.csmpn_type_attr_backward(i["n"], T, K, m.types.data_ptr(), i["S"], None, None, 0, m.g_node.data_ptr(), None, o[2], stream()) == native.ERR_INVALID
    assert lib.csmpn_type_attr_backward_det(i["n"], T, K, m.types.data_ptr(), i["S"], None, None, 0, m.g_node.data_ptr(), None, o[2], o[3],
                                            4096 * 4, stream()) == native.ERR_INVALID
    assert lib.csmpn_type_attr_backward_det_bytes(T, K, i["S"], 0) == 0
    for g in out:
        assert g.ok(written=False) and bool(torch.isnan(g.t).all())


def test_type_attr_comparison_can_fail(pkg):
    """A3's deterministic table gradient without the float64 sum of one workgroup's chunk (rows 8 .. 15 of 1100)."""
    m = Attr("A3")
    i = m.inp
    chunk = G.attr_det_chunk_rows(i["S"] + i["E"], i["K"])
    assert chunk == 8
    got = m.backward(("node", "edge"), det=True)
    attr_compare("A3", got, i, ("node", "edge"))
    bad = got.double().cpu() - G.attr_backward(i, torch.float64, rows=(chunk, 2 * chunk))
    with pytest.raises(AssertionError):
        attr_compare("A3-mutated", bad, i, ("node", "edge"))


# ====================================================================================================== simplex rows
def rows_cabi(inp, n_rows=None, grades=None, extra_blocks=0):
    from csmpn_hip import native
    feats = [f.to(dev()).contiguous() for f in inp["feats"]]
    feats += [feats[-1]] * extra_blocks
    grades = list(grades or inp["grades"]) + [inp["grades"][-1]] * extra_blocks
    verts = inp["verts"].to(dev())
    arr = (native.VertexBlock * len(feats))()
    for k, (f, g) in enumerate(zip(feats, grades)):
        arr[k].data, arr[k].channels, arr[k].grade = f.data_ptr(), f.shape[1], int(g)
    ctot = sum(verts.shape[1] * f.shape[1] for f in feats)
    out = Guarded((verts.shape[0], ctot, 1 << inp["n"]))
    rc = native.lib().csmpn_simplex_rows(inp["n"], arr, len(feats), verts.data_ptr(), verts.shape[0] if n_rows is None else n_rows,
                                         verts.shape[1], inp["S"], out.t.data_ptr(), stream())
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("tag", sorted(G.ROWS_CASES))
def test_simplex_rows_equal_reference(pkg, tag):
    from csmpn_hip import ops
    inp = G.rows_inputs(tag)
    want = G.rows_reference(inp)
    rc, out = rows_cabi(inp)
    assert rc == 0 and out.ok(), tag
    assert torch.equal(out.t.cpu(), want), tag
    through_ops = ops.simplex_rows(inp["n"], [(f.to(dev()), g) for f, g in zip(inp["feats"], inp["grades"])], inp["verts"].to(dev()))
    assert torch.equal(through_ops.cpu(), want), tag


def test_simplex_rows_invalid_arguments(pkg):
    from csmpn_hip import native
    inp = G.rows_inputs("R1")
    rc, out = rows_cabi(inp, extra_blocks=1)                       # five blocks
    assert rc == native.ERR_INVALID and out.ok(written=False) and bool(torch.isnan(out.t).all())
    rc, out = rows_cabi(inp, grades=[1, 0, 2, 6])                  # a grade above n = 5
    assert rc == native.ERR_INVALID and out.ok(written=False) and bool(torch.isnan(out.t).all())
    rc, out = rows_cabi(inp, n_rows=0)                             # no row: OK, nothing written
    assert rc == 0 and out.ok(written=False) and bool(torch.isnan(out.t).all())


def test_simplex_rows_comparison_can_fail(pkg):
    """One element of R1's grade-2 block moved one blade to the right."""
    inp = G.rows_inputs("R1")
    want = G.rows_reference(inp)
    rc, out = rows_cabi(inp)
    assert rc == 0 and torch.equal(out.t.cpu(), want)
    bad = out.t.cpu().clone()
    ch = 3 * 1 + 3 * 2                                             # first channel of the third block: (1 channel, grade 2)
    blade = int(G.algebra(5).grade_slices[2].start) + 4
    assert float(bad[11, ch + 1, blade]) != 0
    bad[11, ch + 1, blade + 1], bad[11, ch + 1, blade] = bad[11, ch + 1, blade], 0.0
    assert not torch.equal(bad, want)
