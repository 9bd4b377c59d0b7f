"""Shared by tests/test_f64_cpu.py and tests/test_f64_gpu.py (float64 CEMLP / EGCL on the device): the case tables, the
references, the one comparison rule and the child-process scenarios.

Comparison rule (one for every tensor): err(a, truth) = max|a - truth| / max|truth|. The truth is the imported reference's own
float64 run where a fixture holds one (tests/golden/egcl*_*.npz, model_*.npz), else oracle/ref_path.py in float64 on the
host. The yardstick is the same measure between a SECOND, independent float64 implementation and that truth, computed on
the host in the test, never from the code under test: the float64 build of the C++ twin for layers and CEMLPs, the model on
the host through the oracle injection for the task models. bound = max(FLOOR, 4 x yardstick): 4 is the suite's standing
slack (tests/test_hip_parity.py), FLOOR = 1e-5 * 2^-29 the suite's float32 floor scaled by the ratio of the unit round-offs
(a tensor's yardstick can be a few ulp by luck). Cl(4,1) gets no constant of its own: its yardstick carries the conditioning.

Run as a program (`python tests/f64_helpers.py <scenario>`) it is the fresh child process of the GPU tests: it prints one
JSON line on stdout, the library's CSMPN_DEBUG dispatch log goes to stderr.
"""
import functools
import hashlib
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "clifford-group-equivariant-simplicial-message-passing-networks_amd"
GOLD = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOOR = 1e-5 * 2.0 ** -29
SLACK = 4.0

METRICS = {"cl20": (1.0, 1.0), "cl30": (1.0, 1.0, 1.0), "cl40": (1.0,) * 4, "cl31": (1.0, 1.0, 1.0, -1.0), "cl50": (1.0,) * 5,
           "cl41": (1.0, 1.0, 1.0, 1.0, -1.0)}
EGCL_FIXTURES = [("egcl", "cl20"), ("egcl", "cl30"), ("egcl", "cl41"), ("egcl", "cl50"), ("egcl8", "cl30"), ("egcl8", "cl41")]
EGCL_TAGS = ["sum_res1_ag0", "sum_res1_ag1", "sum_res0_ag0", "mean_res1_ag0", "mean_res1_ag1", "mean_res0_ag0", "noattr"]
MODELS = ["hulls", "md17", "motion", "nba"]
KEYS = ["0.weight", "0.bias", "1.a", "1.b", "2.weight", "2.normalization.a", "2.linear_right.weight", "2.linear_left.weight",
        "2.linear_left.bias", "3.a"]


def pkg():
    return importlib.import_module(PKG_NAME)


def err(a, truth):
    a, truth = np.asarray(a, np.float64), np.asarray(truth, np.float64)
    assert a.shape == truth.shape, (a.shape, truth.shape)
    if truth.size == 0:
        return 0.0
    return float(np.abs(a - truth).max() / max(np.abs(truth).max(), 1e-300))


def bound(yard):
    return max(FLOOR, SLACK * yard)


def assert_close(name, got, truth, yard):
    e, b = err(got, truth), bound(yard)
    print(f"[f64] {name}: err {e:.3e} yardstick {yard:.3e} bound {b:.3e}")
    assert np.isfinite(np.asarray(got)).all(), name
    assert e <= b, f"{name}: err {e:.3e} > bound {b:.3e} (yardstick {yard:.3e})"


# ------------------------------------------------------------------------------------------------ tile plan (include/csmpn_hip.h)

def plan(n, widths, rows):
    """(tile rows R, tiles, grid, workspace bytes) of the float64 family as include/csmpn_hip.h documents them;
    widths = [(in, out)] per block."""
    D, G = 1 << n, n + 1
    from oracle.tables import AlgebraTables
    P = AlgebraTables([1.0] * n).P      # the path count depends on n alone
    maxO = max(o for _, o in widths)
    maxW = max(max(i, o) for i, o in widths)
    r = 8 * (7 * maxO * D + 5 * maxO * G + 3 * maxO + 2)
    R = min(32, 65536 // r)
    if R == 0:
        R = 163840 // r
    tiles = -(-rows // R)
    grid = min(tiles, 512 if R * r <= 65536 else 256)
    slices = sum(o * i * G + 3 * o + 3 * o * G + o * P + 2 * o * o * G for i, o in widths)
    return R, tiles, grid, 8 * grid * (slices + R * D * sum(i for i, _ in widths) + 2 * R * D * maxW)


def widths_of(in_f, hid, out_f, nl):
    return [(in_f if k == 0 else hid, hid if k < nl - 1 else out_f) for k in range(nl)]


# ------------------------------------------------------------------------------------------------ EGCL fixtures

@functools.lru_cache(maxsize=None)
def load(kind, name):
    return np.load(os.path.join(GOLD, f"{kind}_{name}.npz"))


def egcl_case(kind, name, variant):
    """Inputs, parameters and the reference's float64 results of one fixture variant."""
    g, f = load(kind, name), f"f64/{variant}"
    noattr = variant == "noattr"
    c = dict(metric=tuple(load("tables", name)["metric"].tolist()), noattr=noattr,
             aggr="mean" if noattr else variant.split("_")[0], residual="res0" not in variant, ag=variant.endswith("ag1"),
             h=g[f"{f}/h"], ei=g[f"{f}/edge_index"], gout=g[f"{f}/gout"],
             ea=None if noattr else g[f"{f}/edge_attr"], na=None if noattr else g[f"{f}/node_attr"],
             params={k[len(f) + 3:]: g[k] for k in g.files if k.startswith(f + "/p/")})
    keys = ["y", "gh"] + (["g_edge_attr", "g_node_attr"] if c["ag"] else [])
    c["truth"] = {k: g[f"{f}/{k}"] for k in keys}
    c["truth"].update({"g/" + k: g[f"{f}/g/{k}"] for k in c["params"]})
    assert c["h"].dtype == np.float64 and c["truth"]["y"].dtype == np.float64
    return c


def twin_egcl(c):
    """The float64 build of the C++ twin on a case: the same keys as c['truth']."""
    from oracle import cpu_twin
    r = cpu_twin.egcl_layer(c["metric"], c["params"], c["h"], c["ei"], c["ea"], c["na"], aggr=c["aggr"], residual=c["residual"],
                            gout=c["gout"], want_attr_grads=c["ag"], real64=True)
    out = {"y": r["out"], "gh": r["gh"]}
    if c["ag"]:
        out["g_edge_attr"], out["g_node_attr"] = r["g_edge_attr"], r["g_node_attr"]
    out.update({"g/" + k: v.reshape(c["params"][k].shape) for k, v in r["grads"].items()})
    return out


@functools.lru_cache(maxsize=None)
def egcl_yardsticks(kind, name, variant):
    c = egcl_case(kind, name, variant)
    tw = twin_egcl(c)
    assert set(tw) == set(c["truth"])
    return {k: err(tw[k], v) for k, v in c["truth"].items()}


def egcl_module(c, dev):
    """EGCL(...).double() on dev with the case's parameters."""
    P = pkg()
    C = c["h"].shape[1]
    layer = P.EGCL(P.CliffordAlgebra(c["metric"]), C, C + 1 if c["noattr"] else C, C, edge_attr_features=0 if c["noattr"] else 6,
                   node_attr_features=0 if c["noattr"] else 3, residual=c["residual"], aggr=c["aggr"]).double()
    sd = layer.state_dict()
    for k, v in c["params"].items():
        assert k in sd and tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v)
    layer.load_state_dict(sd, strict=True)
    return layer.to(dev)


def run_egcl(c, dev):
    layer = egcl_module(c, dev)
    t = lambda a, rg=False: None if a is None else torch.from_numpy(a).to(dev).requires_grad_(rg)
    h, ea, na = t(c["h"], True), t(c["ea"], c["ag"]), t(c["na"], c["ag"])
    y = layer(h, t(c["ei"]), ea, na)
    (y * t(c["gout"])).sum().backward()
    res = {"y": y.detach().cpu().numpy(), "gh": h.grad.cpu().numpy()}
    if c["ag"]:
        res["g_edge_attr"], res["g_node_attr"] = ea.grad.cpu().numpy(), na.grad.cpu().numpy()
    res.update({"g/" + k: p.grad.cpu().numpy() for k, p in layer.named_parameters()})
    return res


# ------------------------------------------------------------------------------------------------ standalone CEMLP

# (algebra, in, hidden, out, blocks, rows); rows: int, or "R-1" / "R" / "R+1" / "2nd" (one more tile than the grid cap holds)
CEMLP_CASES = (
    [(a, 1, 1, 1, 1, 1) for a in METRICS] + [(a, 5, 4, 4, 2, "R+1") for a in METRICS] + [
        ("cl30", 5, 4, 4, 4, "R-1"), ("cl20", 5, 4, 4, 1, "R"), ("cl31", 5, 4, 4, 4, 3),
        ("cl50", 28, 28, 28, 1, 3), ("cl41", 30, 28, 28, 2, 2), ("cl30", 60, 32, 32, 2, "R+1"), ("cl20", 46, 40, 40, 2, 3),
        ("cl30", 7, 64, 64, 1, 2), ("cl41", 3, 64, 64, 1, 2), ("cl20", 5, 4, 4, 2, "2nd")])


def case_rows(alg, in_f, hid, out_f, nl, rows):
    R, _, _, _ = plan(len(METRICS[alg]), widths_of(in_f, hid, out_f, nl), 1)
    return {"R-1": R - 1, "R": R, "R+1": R + 1, "2nd": 512 * R + 1}.get(rows, rows)


@functools.lru_cache(maxsize=None)
def cemlp_reference(alg, in_f, hid, out_f, nl, rows, seed=0):
    """Parameters, input, cotangent; truth = oracle/ref_path.py in float64, yardstick = the float64 twin against it."""
    from oracle import cpu_twin, ref_path as O
    rows = case_rows(alg, in_f, hid, out_f, nl, rows)
    o = O.Algebra(list(METRICS[alg]), torch.float64)
    gen = torch.Generator().manual_seed(seed)
    p = O.init_cemlp_params(o, in_f, hid, out_f, nl, gen=gen, randomize=True, dtype=torch.float64)
    x = torch.randn(rows, in_f, o.D, generator=gen, dtype=torch.float64)
    gy = torch.randn(rows, out_f, o.D, generator=gen, dtype=torch.float64)
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.clone().requires_grad_(True)
    y = O.cemlp(o, xr, q)
    (y * gy).sum().backward()
    truth = {"y": y.detach().numpy(), "gx": xr.grad.numpy()}
    truth.update({"g/" + k: v.grad.numpy() for k, v in q.items()})
    ty, tgx, tg = cpu_twin.cemlp(METRICS[alg], {k: v.numpy() for k, v in p.items()}, x.numpy(), gy.numpy(), real64=True)
    tw = {"y": ty, "gx": tgx, **{"g/" + k: v.reshape(p[k].shape) for k, v in tg.items()}}
    yard = {k: err(tw[k], v) for k, v in truth.items()}
    return dict(params=p, x=x, gy=gy, truth=truth, yard=yard, rows=rows)


def cemlp_module(alg, in_f, hid, out_f, nl, params, dev):
    P = pkg()
    m = P.CEMLP(P.CliffordAlgebra(METRICS[alg]), in_f, hid, out_f, n_layers=nl).double()
    sd = m.state_dict()
    for k, v in params.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        sd[k] = v.clone()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def run_cemlp(alg, in_f, hid, out_f, nl, ref, dev):
    m = cemlp_module(alg, in_f, hid, out_f, nl, ref["params"], dev)
    x = ref["x"].to(dev).requires_grad_(True)
    y = m(x)
    (y * ref["gy"].to(dev)).sum().backward()
    res = {"y": y.detach().cpu().numpy(), "gx": x.grad.cpu().numpy()}
    res.update({"g/" + k: p.grad.cpu().numpy() for k, p in m.named_parameters()})
    return res


# ------------------------------------------------------------------------------------------------ task models

def direction_for(name, shape):
    key = sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)     # as tests/test_model_harness.py records them
    return torch.randn(shape, generator=torch.Generator().manual_seed(key), dtype=torch.float64)


def build_model(kind, g, dtype=torch.float32, device=None):
    from csmpn.models import simplicial_mpnn as M
    model = {"hulls": M.HullsSimplicialMPNN, "md17": M.MD17SimplicialMPNN, "motion": M.MotionSimplicialMPNN,
             "nba": M.NBASimplicialMPNN}[kind]()
    sd = model.state_dict()
    for k in [k[2:] for k in g.files if k.startswith("p/")]:
        sd[k] = torch.from_numpy(g["p/" + k])
    model.load_state_dict(sd, strict=True)
    model = model.to(dtype)
    return model.to(device) if device is not None else model


def load_batch(g, device=None, dtype=None):
    from csmpn.data.complexes import SimplicialBatch
    b = SimplicialBatch(**{k[2:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("b/")})
    device = device if device is not None else "cpu"
    return b.to(device) if dtype is None else b.to(device, dtype=dtype)


def model_step(kind, dtype, device=None):
    """One forward + backward on the fixture batch: (loss, {name: (norm, directional dot)}, {name: gradient})."""
    g = load("model", kind)
    model = build_model(kind, g, dtype, device)
    loss, _parts = model(load_batch(g, device, dtype if dtype != torch.float32 else None))
    loss.backward()
    gn, grads = {}, {}
    for k, p in model.named_parameters():
        gr = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu()
        grads[k] = gr.numpy()
        gr = gr.double()
        gn[k] = np.array([float(gr.norm()), float((gr * direction_for(k, gr.shape)).sum())])
    return loss.detach().cpu().numpy(), gn, grads


def host_oracle_injection(monkeypatch_setattr):
    """CEMLP / EGCL of the models computed by oracle/ref_path.py on host tensors, in the tensors' own dtype."""
    from csmpn_hip import ops
    from oracle import ref_path as O

    class _Csr:
        def __init__(self, ei, n):
            self.edge_index, self.n_nodes = ei, n

    pd = lambda flat, prefix="": {f"{prefix}layers.{k // 10}.{KEYS[k % 10]}": p for k, p in enumerate(flat)}

    def cemlp_apply(x, binding, params):
        return O.cemlp(O.Algebra(list(binding.metric), x.dtype), x, pd(params))

    def egcl_apply(h, edge_attr, node_attr, spec, csr, params):
        ne = spec.edge.nblk * 10
        p = {**pd(params[:ne], "edge_model."), **pd(params[ne:], "node_model.")}
        return O.egcl(O.Algebra(list(spec.edge.metric), h.dtype), h, csr.edge_index, edge_attr, node_attr, p,
                      aggr="mean" if spec.mean else "sum", residual=bool(spec.residual))

    monkeypatch_setattr(ops, "cemlp_apply", cemlp_apply)
    monkeypatch_setattr(ops, "egcl_apply", egcl_apply)
    monkeypatch_setattr(ops, "get_csr", lambda ei, n: _Csr(ei, n))


def model_errors(kind, loss, gn):
    """err of the loss and, per parameter, of (norm, dot) relative to the norm, against the reference's float64 fixture."""
    g = load("model", kind)
    out = {"backprop_loss": err(loss, g["f64/backprop_loss"])}
    for k, v in gn.items():
        truth = g[f"f64/gn/{k}"]
        out["gn/" + k] = float(np.abs(v - truth).max() / max(truth[0], 1e-300))
    return out


F32_RECORDING = os.path.join(GOLD, "f32_steps_parent.npz")


def f32_step_record():
    """The float32 loss and gradients of the four model steps under CSMPN_DETERMINISTIC=1, as raw bytes (tools/record_f32_steps.py
    writes them to F32_RECORDING on the commit in front of the float64 family; the test compares this build bit for bit)."""
    assert os.environ.get("CSMPN_DETERMINISTIC") == "1"
    out = {}
    dev = torch.device("cuda:0")
    for kind in MODELS:
        loss, _gn, grads = model_step(kind, torch.float32, dev)
        out[f"{kind}/loss"] = np.asarray(loss, np.float32)
        h = hashlib.sha256()
        for k in sorted(grads):
            h.update(k.encode()); h.update(np.ascontiguousarray(grads[k]).tobytes())
        out[f"{kind}/grads_sha256"] = np.frombuffer(h.digest(), np.uint8)
        # a few whole tensors too, so that a mismatch can be looked at
        for k in sorted(grads)[:3]:
            out[f"{kind}/g/{k}"] = grads[k]
    return out


# ------------------------------------------------------------------------------------------------ child-process scenarios

def _digest(res):
    h = hashlib.sha256()
    for k in sorted(res):
        h.update(k.encode()); h.update(np.ascontiguousarray(res[k]).tobytes())
    return h.hexdigest()


def scenario_layer():
    """Bits of one fixture layer and of the second-tile CEMLP case (the dispatch log on stderr proves the second tile)."""
    dev = torch.device("cuda:0")
    out = {"egcl": _digest(run_egcl(egcl_case("egcl8", "cl30", "mean_res1_ag1"), dev))}
    case = CEMLP_CASES[-1]
    ref = cemlp_reference(*case)
    sys.stderr.write("[f64-child] second-tile case\n")
    out["cemlp"] = _digest(run_cemlp(*case[:5], ref, dev))
    return out


def scenario_models():
    """One float64 step of every task model; the dispatch log on stderr names every launch."""
    dev = torch.device("cuda:0")
    out = {}
    for kind in MODELS:
        sys.stderr.write(f"[f64-child] model {kind}\n")
        loss, gn, _ = model_step(kind, torch.float64, dev)
        out[kind] = {"loss": float(loss), "gn": {k: v.tolist() for k, v in gn.items()}}
    return out


if __name__ == "__main__":
    pkg()
    print(json.dumps({"layer": scenario_layer, "models": scenario_models}[sys.argv[1]]()))
