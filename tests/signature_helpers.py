"""Shared by tests/test_signature_cpu.py and tests/test_signature_gpu.py (CEMLP / EGCL on every signature Cl(p,q), p + q = 2..5,
through the run-time-signature kernels, csrc/cemlp_sig.hpp): the signatures, the fixtures, the host restatement of the sign
rule and of the float tile plan, the two comparison rules and the child-process scenarios.

Comparison rules, err(a, truth) = max|a - truth| / max|truth| per tensor (tests/f64_helpers.py):
  float64  bound = max(1e-5 * 2^-29, 4 x yardstick) - the rule of tests/f64_helpers.py. Truth: the reference's float64 fixture
           run (tests/golden/egcl_sig_*.npz) where one exists, else oracle/ref_path.py in float64. Yardstick: the float64 build
           of the C++ twin against that truth.
  float32  bound = max(1e-5, 4 x yardstick) - the standing rule of tests/test_hip_parity.py. Yardstick per tensor: the LARGER
           of two float32 implementations against the float64 truth, the reference's own float32 fixture run and the float32
           build of the twin (on indefinite signatures the twin alone exceeds 4 x the reference's float32 error). Neither is
           the code under test. A (signature, variant) whose largest float32 yardstick exceeds 1e-2 is left out of the float32
           leg only (excluded(): cl23 / noattr, the test on the host asserts that it is the only one).

Run as a program (`python tests/signature_helpers.py <scenario>`) it is the fresh child process of the GPU tests: one JSON
line on stdout, the library's CSMPN_DEBUG dispatch log on stderr.
"""
import functools
import itertools
import json
import os
import sys

import numpy as np
import torch

import f64_helpers as F

ROOT, GOLD = F.ROOT, F.GOLD
err, FLOOR64, SLACK = F.err, F.FLOOR, F.SLACK
FLOOR32 = 1e-5
EXCLUDE_ABOVE = 1e-2

SIGNATURES = {"cl13": (1.0, -1.0, -1.0, -1.0), "cl03": (-1.0, -1.0, -1.0), "cl11": (1.0, -1.0), "cl23": (1.0, 1.0, -1.0, -1.0, -1.0),
              "cl31x": (-1.0, 1.0, 1.0, 1.0)}
TAGS = F.EGCL_TAGS
COMPILED = {(2, 0), (3, 0), (4, 0), (4, 0x8), (5, 0), (5, 0x10)}      # (n, mask of the negative generators)


def all_signatures():
    """The 60 metrics of +1 / -1 entries on 2..5 generators, as (n, mask, metric)."""
    return [(n, neg, tuple(-1.0 if neg >> b & 1 else 1.0 for b in range(n))) for n in range(2, 6) for neg in range(1 << n)]


def bound32(yard):
    return max(FLOOR32, SLACK * yard)


def assert_close(name, got, truth, yard, f32=False):
    e, b = err(got, truth), (bound32(yard) if f32 else F.bound(yard))
    print(f"[sig] {name}: err {e:.3e} yardstick {yard:.3e} bound {b:.3e}")
    assert np.isfinite(np.asarray(got)).all(), name
    assert e <= b, f"{name}: err {e:.3e} > bound {b:.3e} (yardstick {yard:.3e})"


# ------------------------------------------------------------------------------------------------ the sign rule, restated

def blade_bitmaps(n):
    """Blade order: by grade, then lexicographic in the generator indices."""
    return [sum(1 << i for i in c) for g in range(n + 1) for c in itertools.combinations(range(n), g)]


def sign_rule(n, neg, flip_one=None):
    """(sign [D, D], out [D, D], qsign [D]) of the signature `neg` from the structural tables of the all-positive signature
    and the rule of csrc/cemlp_sig.hpp: sign(i, k) flips when popcount(bitmap[i] & bitmap[k] & neg) is odd, qsign(d) when
    popcount(bitmap[d] & neg) is odd. flip_one = (i, k): the mutation of the guard test."""
    bm = blade_bitmaps(n)
    D = 1 << n
    index = {b: i for i, b in enumerate(bm)}
    pop = lambda v: bin(v).count("1")
    sign, out, qsign = np.zeros((D, D), np.int64), np.zeros((D, D), np.int64), np.zeros(D, np.int64)
    for i, a in enumerate(bm):
        for k, b in enumerate(bm):
            s = sum(pop((a >> (t + 1)) & b) for t in range(n))            # structural: reordering of the generators
            sign[i, k] = (-1 if s & 1 else 1) * (-1 if pop(a & b & neg) & 1 else 1)
            out[i, k] = index[a ^ b]
    for d, a in enumerate(bm):
        g = pop(a)
        structural = (-1 if (g * (g - 1) // 2) & 1 else 1) * (-1 if sum(pop((a >> (t + 1)) & a) for t in range(n)) & 1 else 1)
        qsign[d] = structural * (-1 if pop(a & neg) & 1 else 1)
    if flip_one is not None:
        sign[flip_one] = -sign[flip_one]
    return sign, out, qsign


def cayley_from_rule(n, neg, flip_one=None):
    sign, out, _ = sign_rule(n, neg, flip_one)
    D = 1 << n
    c = np.zeros((D, D, D))
    for i in range(D):
        for k in range(D):
            c[i, out[i, k], k] = sign[i, k]
    return c


# ------------------------------------------------------------------------------------------------ tile plans (include/csmpn_hip.h)

def paths(n):
    from oracle.tables import AlgebraTables
    return AlgebraTables([1.0] * n).P      # the path count depends on n alone


def plan32(n, widths, rows):
    """(tile rows R, tiles, grid, workspace bytes, LDS bytes) of the float32 sig entry points as include/csmpn_hip.h states them."""
    D, G, P = 1 << n, n + 1, paths(n)
    maxO = max(o for _, o in widths)
    maxW = max(max(i, o) for i, o in widths)
    t = (D * D + D + 15) // 16 * 16
    r = 4 * (7 * maxO * D + 5 * maxO * G + 3 * maxO + 2)
    R = min(32, (65536 - t) // r)
    if R == 0:
        R = (163840 - t) // r
    tiles = -(-rows // R)
    grid = min(tiles, 512 if R * r + t <= 65536 else 256)
    slices = sum(o * i * G + 3 * o + 3 * o * G + o * P + 2 * o * o * G for i, o in widths)
    return R, tiles, grid, 4 * grid * (slices + R * D * sum(i for i, _ in widths) + 2 * R * D * maxW), R * r + t


plan64 = F.plan


# ------------------------------------------------------------------------------------------------ EGCL fixtures

@functools.lru_cache(maxsize=None)
def load(name):
    """One fixture as a dict: tests/golden/egcl_sig_<name>.npz and, where the float32 runs were split off, ..._f32.npz."""
    out = {}
    for f in (f"egcl_sig_{name}.npz", f"egcl_sig_{name}_f32.npz"):
        p = os.path.join(GOLD, f)
        if os.path.exists(p):
            with np.load(p) as g:
                out.update({k: g[k] for k in g.files})
    assert tuple(out["metric"].tolist()) == SIGNATURES[name]
    return out


def compiled_case(kind, name, variant):
    """A fixture of a compiled algebra (tests/golden/egcl*_*.npz) in the form of egcl_case below."""
    g = {k: v for k, v in F.load(kind, name).items()}
    g["metric"] = np.asarray(F.METRICS[name], np.float32)
    return _case(g, variant)


def egcl_case(name, variant):
    return _case(load(name), variant)


def _case(g, variant):
    """Inputs, parameters, the reference's float64 results (truth) and its float32 results (ref32) of one fixture variant."""
    f, f32 = f"f64/{variant}", f"f32/{variant}"
    noattr = variant == "noattr"
    c = dict(metric=tuple(float(m) for m in g["metric"]), noattr=noattr, aggr="mean" if noattr else variant.split("_")[0],
             residual="res0" not in variant, ag=variant.endswith("ag1"), h=g[f"{f}/h"], ei=g[f"{f}/edge_index"], gout=g[f"{f}/gout"],
             ea=None if noattr else g[f"{f}/edge_attr"], na=None if noattr else g[f"{f}/node_attr"],
             params={k[len(f) + 3:]: g[k] for k in g if k.startswith(f + "/p/")})
    keys = ["y", "gh"] + (["g_edge_attr", "g_node_attr"] if c["ag"] else [])
    for tag, pre in (("truth", f), ("ref32", f32)):
        c[tag] = {k: g[f"{pre}/{k}"] for k in keys}
        c[tag].update({"g/" + k: g[f"{pre}/g/{k}"] for k in c["params"]})
    assert c["h"].dtype == np.float64 and c["truth"]["y"].dtype == np.float64 and c["ref32"]["y"].dtype == np.float32
    assert np.array_equal(g[f"{f32}/h"].astype(np.float64), c["h"])       # both runs describe the same function
    return c


def twin_egcl(c, real64):
    from oracle import cpu_twin
    r = cpu_twin.egcl_layer(c["metric"], c["params"], c["h"], c["ei"], c["ea"], c["na"], aggr=c["aggr"], residual=c["residual"],
                            gout=c["gout"], want_attr_grads=c["ag"], real64=real64)
    out = {"y": r["out"], "gh": r["gh"]}
    if c["ag"]:
        out["g_edge_attr"], out["g_node_attr"] = r["g_edge_attr"], r["g_node_attr"]
    out.update({"g/" + k: v.reshape(c["params"][k].shape) for k, v in r["grads"].items()})
    return out


def _yards(c):
    t64, t32 = twin_egcl(c, True), twin_egcl(c, False)
    assert set(t64) == set(c["truth"]) == set(t32)
    y64 = {k: err(t64[k], v) for k, v in c["truth"].items()}
    y32 = {k: max(err(t32[k], v), err(c["ref32"][k], v)) for k, v in c["truth"].items()}
    return y64, y32, {k: (err(c["ref32"][k], v), err(t32[k], v)) for k, v in c["truth"].items()}


@functools.lru_cache(maxsize=None)
def yardsticks(name, variant):
    """(float64 yardsticks, float32 yardsticks, {tensor: (reference f32, twin f32)}) of one fixture variant."""
    return _yards(egcl_case(name, variant))


@functools.lru_cache(maxsize=None)
def compiled_yardsticks(kind, name, variant):
    return _yards(compiled_case(kind, name, variant))


def excluded(name, variant):
    """Left out of the float32 leg: the float32 arithmetic itself is off by more than 1e-2 on this variant."""
    return max(yardsticks(name, variant)[1].values()) > EXCLUDE_ABOVE


def egcl_module(c, dev, dtype):
    P = F.pkg()
    C = c["h"].shape[1]
    layer = P.EGCL(P.CliffordAlgebra(c["metric"]), C, C + 1 if c["noattr"] else C, C, edge_attr_features=0 if c["noattr"] else 6,
                   node_attr_features=0 if c["noattr"] else 3, residual=c["residual"], aggr=c["aggr"])
    sd = layer.state_dict()
    for k, v in c["params"].items():
        assert k in sd and tuple(sd[k].shape) == v.shape, k
        sd[k] = torch.from_numpy(v).float()
    layer.load_state_dict(sd, strict=True)
    if dtype == torch.float64:
        layer = layer.double()
        sd = layer.state_dict()
        for k, v in c["params"].items():
            sd[k] = torch.from_numpy(v)
        layer.load_state_dict(sd, strict=True)
    return layer.to(dev)


def run_egcl(c, dev, dtype):
    layer = egcl_module(c, dev, dtype)
    t = lambda a, rg=False: None if a is None else torch.from_numpy(a).to(dtype).to(dev).requires_grad_(rg)
    h, ea, na = t(c["h"], True), t(c["ea"], c["ag"]), t(c["na"], c["ag"])
    y = layer(h, torch.from_numpy(c["ei"]).to(dev), ea, na)
    (y * t(c["gout"])).sum().backward()
    res = {"y": y.detach().cpu().numpy(), "gh": h.grad.cpu().numpy()}
    if c["ag"]:
        res["g_edge_attr"], res["g_node_attr"] = ea.grad.cpu().numpy(), na.grad.cpu().numpy()
    res.update({"g/" + k: p.grad.cpu().numpy() for k, p in layer.named_parameters()})
    assert all(v.dtype == (np.float64 if dtype == torch.float64 else np.float32) for v in res.values())
    return res


# ------------------------------------------------------------------------------------------------ oracle cases (no fixture)

@functools.lru_cache(maxsize=None)
def cemlp_reference(metric, in_f, hid, out_f, nl, rows, seed=0):
    """Parameters, input, cotangent in float64 and the float64 / float32 twin on them."""
    from oracle import cpu_twin, ref_path as O
    o = O.Algebra(list(metric), torch.float64)
    gen = torch.Generator().manual_seed(seed)
    p = O.init_cemlp_params(o, in_f, hid, out_f, nl, gen=gen, randomize=True, dtype=torch.float64)
    x = torch.randn(rows, in_f, o.D, generator=gen, dtype=torch.float64)
    gy = torch.randn(rows, out_f, o.D, generator=gen, dtype=torch.float64)
    out = dict(params=p, x=x, gy=gy)
    for tag, r64 in (("twin64", True), ("twin32", False)):
        ty, tgx, tg = cpu_twin.cemlp(metric, {k: v.numpy() for k, v in p.items()}, x.numpy(), gy.numpy(), real64=r64)
        out[tag] = {"y": ty, "gx": tgx, **{"g/" + k: v.reshape(p[k].shape) for k, v in tg.items()}}
    return out


def oracle_cemlp(metric, ref):
    """oracle/ref_path.py in float64 on a cemlp_reference case."""
    from oracle import ref_path as O
    o = O.Algebra(list(metric), torch.float64)
    q = {k: v.clone().requires_grad_(True) for k, v in ref["params"].items()}
    xr = ref["x"].clone().requires_grad_(True)
    y = O.cemlp(o, xr, q)
    (y * ref["gy"]).sum().backward()
    truth = {"y": y.detach().numpy(), "gx": xr.grad.numpy()}
    truth.update({"g/" + k: v.grad.numpy() for k, v in q.items()})
    return truth


def run_cemlp(metric, in_f, hid, out_f, nl, ref, dev, dtype):
    P = F.pkg()
    m = P.CEMLP(P.CliffordAlgebra(metric), in_f, hid, out_f, n_layers=nl).to(dtype)
    sd = m.state_dict()
    for k, v in ref["params"].items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        sd[k] = v.clone().to(dtype)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev)
    x = ref["x"].to(dtype).to(dev).requires_grad_(True)
    y = m(x)
    (y * ref["gy"].to(dtype).to(dev)).sum().backward()
    res = {"y": y.detach().cpu().numpy(), "gx": x.grad.cpu().numpy()}
    res.update({"g/" + k: p.grad.cpu().numpy() for k, p in m.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def small_egcl_case(metric, seed=5):
    """A two-block EGCL on N = 5, E = 7, 2 channels, no attributes, float64: the case of the sweep and of gradcheck. truth =
    oracle/ref_path.py in float64, twin64 = the float64 twin."""
    from oracle import ref_path as O
    o = O.Algebra(list(metric), torch.float64)
    gen = torch.Generator().manual_seed(seed)
    p = O.init_egcl_params(o, 2, 2, 2, gen=gen, randomize=True, dtype=torch.float64)
    ei = torch.randint(0, 4, (2, 7), generator=gen)       # node 4 is isolated
    ei[:, 1] = ei[:, 0]                                   # a duplicate edge
    ei[1, 2] = ei[0, 2]                                   # a self loop
    h = torch.randn(5, 2, o.D, generator=gen, dtype=torch.float64)
    gout = torch.randn(5, 2, o.D, generator=gen, dtype=torch.float64)
    c = dict(metric=tuple(metric), noattr=True, aggr="mean", residual=True, ag=False, ea=None, na=None,
             params={k: v.numpy() for k, v in p.items()}, h=h.numpy(), ei=ei.numpy(), gout=gout.numpy())
    q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    hr = h.clone().requires_grad_(True)
    y = O.egcl(o, hr, ei, None, None, q, aggr="mean", residual=True)
    (y * gout).sum().backward()
    c["truth"] = {"y": y.detach().numpy(), "gh": hr.grad.numpy(), **{"g/" + k: v.grad.numpy() for k, v in q.items()}}
    c["twin64"] = twin_egcl(c, True)
    return c


def run_small_egcl(c, dev, dtype=torch.float64):
    P = F.pkg()
    layer = P.EGCL(P.CliffordAlgebra(c["metric"]), 2, 2, 2, aggr="mean").to(dtype)
    sd = layer.state_dict()
    for k, v in c["params"].items():
        sd[k] = torch.from_numpy(v).to(dtype)
    layer.load_state_dict(sd, strict=True)
    layer = layer.to(dev)
    h = torch.from_numpy(c["h"]).to(dtype).to(dev).requires_grad_(True)
    y = layer(h, torch.from_numpy(c["ei"]).to(dev))
    (y * torch.from_numpy(c["gout"]).to(dtype).to(dev)).sum().backward()
    res = {"y": y.detach().cpu().numpy(), "gh": h.grad.cpu().numpy()}
    res.update({"g/" + k: p.grad.cpu().numpy() for k, p in layer.named_parameters()})
    return res


# ------------------------------------------------------------------------------------------------ child-process scenarios

def _hex(res):
    return F._digest(res)


BIT_FIXTURES = [("egcl", "cl30"), ("egcl", "cl41"), ("egcl8", "cl41")]
BIT_VARIANT = "mean_res1_ag1"


def scenario_bits():
    """float64 digests of three compiled fixtures (the parent compares a CSMPN_FORCE_SIG=1 child with a default one), of a
    sig-only float32 and float64 layer, and the last kernel names."""
    from csmpn_hip import native
    dev = torch.device("cuda:0")
    out = {}
    for kind, name in BIT_FIXTURES:
        sys.stderr.write(f"[sig-child] {kind}_{name}\n")
        out[f"{kind}_{name}"] = _hex(run_egcl(compiled_case(kind, name, BIT_VARIANT), dev, torch.float64))
        out[f"{kind}_{name}/kernel"] = native.lib().csmpn_last_kernel().decode()
    sys.stderr.write("[sig-child] cl13\n")
    c = egcl_case("cl13", BIT_VARIANT)
    out["cl13/f32"] = _hex(run_egcl(c, dev, torch.float32))
    out["cl13/f64"] = _hex(run_egcl(c, dev, torch.float64))
    return out


def scenario_sweep():
    """All 60 signatures in float64 on a one-block CEMLP 2 -> 3 channels on 3 rows and a two-block EGCL on N = 5, E = 7: per
    tensor [err of the device, err of the float64 twin] against oracle/ref_path.py in float64; the dispatch log on stderr
    names the kernel of every launch."""
    dev = torch.device("cuda:0")
    out = {}
    for n, neg, metric in all_signatures():
        sys.stderr.write(f"[sig-child] signature n={n} neg={neg}\n")
        ref = cemlp_reference(metric, 2, 3, 3, 1, 3)
        truth = oracle_cemlp(metric, ref)
        got = run_cemlp(metric, 2, 3, 3, 1, ref, dev, torch.float64)
        out[f"{n}/{neg}/cemlp"] = {k: [err(got[k], v), err(ref["twin64"][k], v)] for k, v in truth.items()}
        c = small_egcl_case(metric)
        got = run_small_egcl(c, dev)
        out[f"{n}/{neg}/egcl"] = {k: [err(got[k], v), err(c["twin64"][k], v)] for k, v in c["truth"].items()}
    return out


TILE_METRIC = (1.0, -1.0)


def tile_rows(plan):
    """One row more than the grid cap holds tiles of the 2-channel Cl(1,1) CEMLP: a workgroup takes a second tile."""
    R, _, grid, *_ = plan(2, [(2, 2)], 10 ** 9)
    return grid * R + 1


def scenario_tiles():
    """Cl(1,1), 2 channels, one block, tile_rows() rows, both dtypes: per tensor [err of the device, yardstick] against
    oracle/ref_path.py in float64 (yardstick: the twin of that dtype; in float32 the larger of the twin and the oracle's own
    float32 run); grid and tile count go to the dispatch log."""
    from oracle import ref_path as O
    dev = torch.device("cuda:0")
    out = {}
    for tag, dtype, plan in (("f64", torch.float64, plan64), ("f32", torch.float32, plan32)):
        rows = tile_rows(plan)
        sys.stderr.write(f"[sig-child] tiles {tag} rows={rows}\n")
        ref = cemlp_reference(TILE_METRIC, 2, 2, 2, 1, rows)
        truth = oracle_cemlp(TILE_METRIC, ref)
        got = run_cemlp(TILE_METRIC, 2, 2, 2, 1, ref, dev, dtype)
        if dtype == torch.float64:
            yard = {k: err(ref["twin64"][k], v) for k, v in truth.items()}
        else:
            o = O.Algebra(list(TILE_METRIC), torch.float32)
            q = {k: v.float().requires_grad_(True) for k, v in ref["params"].items()}
            xr = ref["x"].float().requires_grad_(True)
            y = O.cemlp(o, xr, q)
            (y * ref["gy"].float()).sum().backward()
            o32 = {"y": y.detach().numpy(), "gx": xr.grad.numpy(), **{"g/" + k: v.grad.numpy() for k, v in q.items()}}
            yard = {k: max(err(ref["twin32"][k], v), err(o32[k], v)) for k, v in truth.items()}
        out[tag] = {k: [err(got[k], v), yard[k]] for k, v in truth.items()}
        out[tag + "/rows"] = rows
    return out


if __name__ == "__main__":
    F.pkg()
    print(json.dumps({"bits": scenario_bits, "sweep": scenario_sweep, "tiles": scenario_tiles}[sys.argv[1]]()))
