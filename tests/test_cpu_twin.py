"""CPU: the C++ sparse-formulation twin (include/csmpn_cpu.h) against the golden vectors recorded from
the imported reference - the same fixtures that pin the PyTorch oracle. A second, torch-free ground
truth for the kernels and bench.py's strong CPU baseline; never on the product path."""
import os

import numpy as np
import pytest

from oracle import cpu_twin

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALGS = ["cl20", "cl30", "cl50", "cl41"]
EGCL_TAGS = ["sum_res1_ag0", "sum_res1_ag1", "sum_res0_ag0", "mean_res1_ag0", "mean_res1_ag1", "mean_res0_ag0", "noattr"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", ALGS)
@pytest.mark.parametrize("variant", EGCL_TAGS)
def test_twin_egcl_vs_reference_fixture(name, variant):
    g = np.load(os.path.join(GOLD, f"egcl_{name}.npz"))
    metric = np.load(os.path.join(GOLD, f"tables_{name}.npz"))["metric"]
    f32, f64 = f"f32/{variant}", f"f64/{variant}"
    p = {k[len(f32) + 3:]: g[k] for k in g.files if k.startswith(f32 + "/p/")}
    noattr = variant == "noattr"
    ag = variant.endswith("ag1")
    res = cpu_twin.egcl_layer(metric, p, g[f"{f32}/h"], g[f"{f32}/edge_index"],
                              None if noattr else g[f"{f32}/edge_attr"], None if noattr else g[f"{f32}/node_attr"],
                              aggr="mean" if noattr else variant.split("_")[0], residual="res0" not in variant,
                              gout=g[f"{f32}/gout"], want_attr_grads=ag, threads=2)
    # float32 against the float64 reference run; the reference's own float32 run is the yardstick
    slack = 20.0 if (metric < 0).any() else 4.0   # null-cone norms: ill-conditioned in any float32 evaluation
    bound = lambda k: max(1e-5, slack * rel(g[f"{f32}/{k}"], g[f"{f64}/{k}"]))
    assert rel(res["out"], g[f"{f64}/y"]) <= bound("y")
    assert rel(res["gh"], g[f"{f64}/gh"]) <= bound("gh")
    if ag:
        assert rel(res["g_edge_attr"], g[f"{f64}/g_edge_attr"]) <= bound("g_edge_attr")
        assert rel(res["g_node_attr"], g[f"{f64}/g_node_attr"]) <= bound("g_node_attr")
    for k, v in res["grads"].items():
        assert rel(v, g[f"{f64}/g/{k}"]) <= bound(f"g/{k}"), k


@pytest.mark.parametrize("name", ALGS)
@pytest.mark.parametrize("variant", ["sum_res1_ag1", "mean_res0_ag0", "noattr"])
def test_twin_float64_build_vs_reference_float64_fixture(name, variant):
    """The float64 build of the twin (oracle/_build/libcsmpn_cpu64.so: the truth of tests/test_full_size_twin.py) against
    the reference's own float64 run: same parameters and inputs (the float32 ones, widened), agreement to rounding."""
    g = np.load(os.path.join(GOLD, f"egcl_{name}.npz"))
    metric = np.load(os.path.join(GOLD, f"tables_{name}.npz"))["metric"]
    f32, f64 = f"f32/{variant}", f"f64/{variant}"
    p = {k[len(f32) + 3:]: g[k] for k in g.files if k.startswith(f32 + "/p/")}
    noattr = variant == "noattr"
    ag = variant.endswith("ag1")
    for k in ("h", "gout"):
        assert np.array_equal(g[f"{f32}/{k}"].astype(np.float64), g[f"{f64}/{k}"]), k
    res = cpu_twin.egcl_layer(metric, p, g[f"{f32}/h"], g[f"{f32}/edge_index"],
                              None if noattr else g[f"{f32}/edge_attr"], None if noattr else g[f"{f32}/node_attr"],
                              aggr="mean" if noattr else variant.split("_")[0], residual="res0" not in variant,
                              gout=g[f"{f32}/gout"], want_attr_grads=ag, threads=2, real64=True)
    assert res["out"].dtype == np.float64
    tol = 1e-7 if (metric < 0).any() else 1e-10
    assert rel(res["out"], g[f"{f64}/y"]) <= tol
    assert rel(res["gh"], g[f"{f64}/gh"]) <= tol
    if ag:
        assert rel(res["g_edge_attr"], g[f"{f64}/g_edge_attr"]) <= tol
        assert rel(res["g_node_attr"], g[f"{f64}/g_node_attr"]) <= tol
    for k, v in res["grads"].items():
        assert v.dtype == np.float64 and rel(v, g[f"{f64}/g/{k}"]) <= tol, k


@pytest.mark.parametrize("name", ALGS)
@pytest.mark.parametrize("tag", ["cemlp1_C3", "cemlp2_C8"])
def test_twin_cemlp_vs_reference_fixture(name, tag):
    g = np.load(os.path.join(GOLD, f"layers_{name}.npz"))
    metric = np.load(os.path.join(GOLD, f"tables_{name}.npz"))["metric"]
    p = {k[len(tag) + 3:]: g[k] for k in g.files if k.startswith(tag + "/p/")}
    y, gx, grads = cpu_twin.cemlp(metric, p, g[f"{tag}/x"], g[f"{tag}/gout"], threads=1)
    tol = 2e-4 if (metric < 0).any() else 2e-5     # float32 twin against the float32 fixture
    assert rel(y, g[f"{tag}/y"]) <= tol
    assert rel(gx, g[f"{tag}/gx"]) <= 10 * tol
    for k, v in grads.items():
        assert rel(v, g[f"{tag}/g/{k}"]) <= 10 * tol, k


def test_twin_rejects_bad_indices():
    g = np.load(os.path.join(GOLD, "egcl_cl30.npz"))
    f32 = "f32/noattr"
    p = {k[len(f32) + 3:]: g[k] for k in g.files if k.startswith(f32 + "/p/")}
    ei = g[f"{f32}/edge_index"].copy()
    ei[1, 0] = 10_000
    with pytest.raises(RuntimeError, match="outside"):
        cpu_twin.egcl_layer([1.0, 1.0, 1.0], p, g[f"{f32}/h"], ei)


@pytest.mark.parametrize("tag", ["S1", "M32"])
def test_twin_float64_vs_reference_fixture_full_size(tag):
    """The float64 build of the twin - the truth of tests/test_full_size_twin.py, and the only truth of S2 / H28 where the
    reference's dense formulation does not fit in memory - against the imported reference's own float64 run at FULL size
    (100 k edges; tests/golden/make_fullsize_golden.py): y and d/dh on the stored node subsample, every parameter gradient."""
    import importlib
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    T = importlib.import_module("test_full_size_twin")
    g = np.load(os.path.join(GOLD, f"fullsize_{tag}.npz"))
    metric, C, aggr, h, ei, ea, na, p, gout, t64, _t32 = T._case(tag)
    np.testing.assert_allclose(T._input_checksums(h, ei, ea, na, p, gout), g["checksums"], rtol=1e-12, atol=0)
    st = int(g["node_stride"])
    assert rel(t64["out"][::st], g["f64/y"]) < 1e-10 and rel(t64["gh"][::st], g["f64/gh"]) < 1e-10
    for k, v in t64["grads"].items():
        assert rel(v, g[f"f64/g/{k}"]) < 1e-10, k


# one small EGCL per algebra at a width of the wide row-tile kernel (65..256 channels): (metric, N, E, C, hidden, aggr, residual)
WIDE_TWIN_CASES = [
    ((1.0, 1.0), 12, 40, 80, 80, "sum", True),
    ((1.0, 1.0, 1.0), 12, 40, 48, 96, "mean", False),
    ((1.0, 1.0, 1.0, 1.0), 8, 20, 72, 72, "mean", True),
    ((1.0, 1.0, 1.0, -1.0), 8, 20, 72, 72, "sum", False),
    ((1.0,) * 5, 6, 14, 80, 80, "mean", True),
    ((1.0, 1.0, 1.0, 1.0, -1.0), 6, 14, 65, 65, "sum", True),
]


@pytest.mark.parametrize("metric,N,E,C,hidden,aggr,residual", WIDE_TWIN_CASES,
                         ids=[f"n{len(c[0])}{'m' if min(c[0]) < 0 else ''}-{c[3]}-{c[4]}" for c in WIDE_TWIN_CASES])
def test_twin_float64_build_vs_oracle_at_wide_widths(metric, N, E, C, hidden, aggr, residual):
    """The twin's float64 build is the truth of tests/test_wide_multitile_gpu.py (the only reference that reaches those sizes
    at D = 32), and it had never been compared with anything above 32 channels. Here against the float64 torch oracle
    (oracle/ref_path.py) at 65..96 channels, every algebra: y, d/dh, d/d(edge_attr), d/d(node_attr) and every parameter
    gradient at the agreement level of test_twin_float64_build_vs_reference_float64_fixture (1e-10; 1e-7 on the indefinite
    metrics, whose inputs are kept off the null cone as in the GPU tests: neg_scale = 0.02)."""
    import torch
    from oracle import ref_path as O
    oa, o32 = O.Algebra(list(metric), torch.float64), O.Algebra(list(metric), torch.float32)
    h, ei, ea, na = O.synthetic_complex(o32, N, E, C, seed=N + E + C)
    if min(metric) < 0:
        neg_bits = sum(1 << i for i, m in enumerate(metric) if m < 0)
        mask = torch.from_numpy(((np.asarray(o32.t.index_to_bitmap) & neg_bits) != 0).astype(np.float32))
        h = h * (1.0 - mask + 0.02 * mask)
    gen = torch.Generator().manual_seed(N + E + C + 1)
    p = O.init_egcl_params(o32, C, hidden, C, ea.shape[1], na.shape[1], gen=gen, randomize=True)
    gout = torch.randn(N, C, 1 << len(metric), generator=gen)
    q = {k: v.double().requires_grad_(True) for k, v in p.items()}
    h64, ea64, na64 = (t.double().requires_grad_(True) for t in (h, ea, na))
    y64 = O.egcl(oa, h64, ei, ea64, na64, q, aggr=aggr, residual=residual)
    (y64 * gout.double()).sum().backward()
    res = cpu_twin.egcl_layer(np.asarray(metric, np.float32), {k: v.numpy() for k, v in p.items()}, h.numpy(), ei.numpy(),
                              ea.numpy(), na.numpy(), aggr=aggr, residual=residual, gout=gout.numpy(), want_attr_grads=True,
                              threads=2, real64=True)
    tol = 1e-7 if min(metric) < 0 else 1e-10
    assert res["out"].dtype == np.float64
    assert rel(res["out"], y64.detach().numpy()) <= tol
    assert rel(res["gh"], h64.grad.numpy()) <= tol
    assert rel(res["g_edge_attr"], ea64.grad.numpy()) <= tol
    assert rel(res["g_node_attr"], na64.grad.numpy()) <= tol
    assert set(res["grads"]) == set(q)
    for k, v in res["grads"].items():
        assert rel(v, q[k].grad.numpy()) <= tol, k


def test_twin_float64_build_vs_reference_wide_fixture():
    """The twin's float64 build against the reference's own 96-channel EGCL run (tests/golden/egcl_wide_cl30.npz,
    make_wide_golden.py): y, d/dh and every parameter gradient, the weight-matrix gradients on the stored output-channel
    rows. The fixture keeps the reference's float64 values rounded to float32: each element is within 2^-24 (6e-8) of its
    own magnitude, so within 6e-8 of the tensor's maximum; the twin itself agrees with the reference to 1e-10. Bound: 1e-7."""
    from wide_helpers import wide_fixture_param
    g = np.load(os.path.join(GOLD, "egcl_wide_cl30.npz"))
    C = 96
    import importlib
    pkg = importlib.import_module("clifford-group-equivariant-simplicial-message-passing-networks_amd")
    layer = pkg.EGCL(pkg.CliffordAlgebra((1.0, 1.0, 1.0)), C, C, C, edge_attr_features=6, node_attr_features=3, aggr="mean")
    shapes = {k: tuple(v.shape) for k, v in layer.named_parameters()}
    assert {"psum/" + k for k in shapes} == {k for k in g.files if k.startswith("psum/")}
    p = {}
    for k, shp in shapes.items():
        v = wide_fixture_param(k, shp)
        assert float(v.double().sum()) == float(g["psum/" + k]), k    # the parameter rule and the shapes are the fixture's
        p[k] = v.numpy()
    res = cpu_twin.egcl_layer([1.0, 1.0, 1.0], p, g["h"], g["edge_index"], g["edge_attr"], g["node_attr"], aggr="mean",
                              residual=True, gout=g["gout"], threads=2, real64=True)
    rows = g["rows"]
    got = {"y": res["out"], "gh": res["gh"]}
    n_weight_matrices = 0
    for k, a in res["grads"].items():
        full = a.ndim == 3 and a.shape[0] == C
        n_weight_matrices += full
        got["g/" + k] = a[rows] if full else a
    assert n_weight_matrices == 12
    assert set(got) == {k[4:] for k in g.files if k.startswith("f64/")}
    for k, v in got.items():
        assert v.shape == g["f64/" + k].shape, k
        assert rel(v, g["f64/" + k]) <= 1e-7, (k, rel(v, g["f64/" + k]))
