"""Host side of the float64 kernel family (no GPU): the new C-ABI names, the workspace query against its documented formula,
every rejected argument combination (code and message, without a device), the yardstick table of the comparison rule, and
a guard that the comparison can fail. The rule itself: tests/f64_helpers.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import f64_helpers as H

NEW = ["csmpn_cemlp_f64_workspace_bytes", "csmpn_cemlp_forward_f64", "csmpn_cemlp_backward_f64", "csmpn_egcl_edge_forward_f64",
       "csmpn_egcl_edge_backward_f64", "csmpn_egcl_node_forward_f64", "csmpn_egcl_node_backward_f64", "csmpn_segment_reduce_f64"]


def _blocks(native, widths, ptr=8):
    bp = (native.BlockParams * len(widths))()
    for k, (i, o) in enumerate(widths):
        bp[k].in_features, bp[k].out_features, bp[k].lin_subspaces = i, o, 1
        for name in native.PARAM_FIELDS:
            setattr(bp[k], name, ptr)     # never dereferenced: every call below is rejected or launches nothing
    return bp


def test_new_entry_points_are_declared_exported_and_bound(pkg):
    from csmpn_hip import native
    header = open(os.path.join(H.ROOT, "include", "csmpn_hip.h")).read()
    declared = set(re.findall(r"\b(csmpn_[a-z0-9_]+)\s*\(", header))
    lib = native.lib()
    for name in NEW:
        assert name in declared and name in native.EXPORTS and hasattr(lib, name), name
    assert lib.csmpn_abi_version() == 2
    assert "csmpn_block_params_f64" in header and "csmpn_block_grads_f64" in header


@pytest.mark.parametrize("alg,widths", [("cl20", [(5, 4), (4, 4)]), ("cl30", [(14, 8), (8, 8)]), ("cl41", [(3, 64)]),
                                        ("cl50", [(34, 28), (28, 28)]), ("cl31", [(5, 4)] + [(4, 4)] * 3)])
def test_workspace_query_is_the_documented_formula_and_monotone(pkg, alg, widths):
    from csmpn_hip import native
    n = len(H.METRICS[alg])
    bp = _blocks(native, widths)
    R, _, _, _ = H.plan(n, widths, 1)
    cap = 512 if R * 8 * (7 * max(o for _, o in widths) * (1 << n) + 5 * max(o for _, o in widths) * (n + 1)
                          + 3 * max(o for _, o in widths) + 2) <= 65536 else 256
    last = 0
    for rows in sorted({0, 1, R - 1, R, R + 1, 2 * R, cap * R, cap * R + 1, 10 * cap * R}):
        got = int(native.lib().csmpn_cemlp_f64_workspace_bytes(n, bp, len(widths), rows))
        _, tiles, grid, want = H.plan(n, widths, rows)
        assert got == want, (rows, got, want)
        assert grid == min(tiles, cap) and got >= last
        last = got
    assert int(native.lib().csmpn_cemlp_f64_workspace_bytes(n, bp, len(widths), 0)) == 0
    assert H.plan(n, widths, cap * R + 1)[3] == H.plan(n, widths, cap * R)[3]     # above the grid cap: no more slices


def test_rejected_arguments_return_their_code_and_message_without_a_device(pkg):
    from csmpn_hip import native
    L, INV, UNS = native.lib(), native.ERR_INVALID, native.ERR_UNSUPPORTED
    m3, bad = native.metric_array([1, 1, 1]), native.metric_array([1, 1, 0.5])
    ok = _blocks(native, [(5, 4), (4, 4)])
    wide = _blocks(native, [(5, 65)])
    broken = _blocks(native, [(5, 4), (3, 4)])
    nullp = _blocks(native, [(5, 4)], ptr=None)
    gr = (native.BlockGrads * 2)()
    big = 1 << 30
    fwd = lambda metric, n, bp, nb, x, rows, y, ws, wsb: L.csmpn_cemlp_forward_f64(metric, n, bp, nb, x, rows, y, ws, wsb, None)
    cases = [
        ("x null", lambda: fwd(m3, 3, ok, 2, None, 3, 8, 8, big), INV, "null"),
        ("blocks null", lambda: fwd(m3, 3, None, 2, 8, 3, 8, 8, big), INV, "blocks is null"),
        ("metric null", lambda: fwd(None, 3, ok, 2, 8, 3, 8, 8, big), INV, "metric is null"),
        ("parameter null", lambda: fwd(m3, 3, nullp, 1, 8, 3, 8, 8, big), INV, "null parameter"),
        ("n = 6", lambda: fwd(native.metric_array([1] * 6), 6, ok, 2, 8, 3, 8, 8, big), UNS, "not supported"),
        ("metric 0.5", lambda: fwd(bad, 3, ok, 2, 8, 3, 8, 8, big), UNS, "not supported"),
        ("0 blocks", lambda: fwd(m3, 3, ok, 0, 8, 3, 8, 8, big), INV, "blocks not in 1..4"),
        ("5 blocks", lambda: fwd(m3, 3, ok, 5, 8, 3, 8, 8, big), INV, "blocks not in 1..4"),
        ("width 65", lambda: fwd(m3, 3, wide, 1, 8, 3, 8, 8, big), UNS, "above the limit of 64"),
        ("chain", lambda: fwd(m3, 3, broken, 2, 8, 3, 8, 8, big), INV, "in_features 3 of block 1"),
        ("small workspace", lambda: fwd(m3, 3, ok, 2, 8, 3, 8, 8, H.plan(3, [(5, 4), (4, 4)], 3)[3] - 1), INV, "workspace of"),
        ("workspace null", lambda: fwd(m3, 3, ok, 2, 8, 3, 8, None, big), INV, "workspace of"),
        ("rows < 0", lambda: fwd(m3, 3, ok, 2, 8, -1, 8, 8, big), INV, "negative row count"),
        ("backward: grads null", lambda: L.csmpn_cemlp_backward_f64(m3, 3, ok, None, 2, 8, 8, 3, 8, 8, big, None), INV, "grads is null"),
        ("backward: gy null", lambda: L.csmpn_cemlp_backward_f64(m3, 3, ok, gr, 2, 8, None, 3, 8, 8, big, None), INV, "null"),
        ("edge: E < 0", lambda: L.csmpn_egcl_edge_forward_f64(m3, 3, ok, 2, 8, 3, 8, 2, 8, 8, 8, -1, 4, 8, 8, big, None), INV,
         "negative row count"),
        ("edge: N < 0", lambda: L.csmpn_egcl_edge_forward_f64(m3, 3, ok, 2, 8, 3, 8, 2, 8, 8, 8, 2, -4, 8, 8, big, None), INV,
         "negative node count"),
        ("edge: perm null", lambda: L.csmpn_egcl_edge_forward_f64(m3, 3, ok, 2, 8, 3, 8, 2, None, 8, 8, 2, 4, 8, 8, big, None), INV, "null"),
        ("edge: channels", lambda: L.csmpn_egcl_edge_forward_f64(m3, 3, ok, 2, 8, 4, 8, 2, 8, 8, 8, 2, 4, 8, 8, big, None), INV,
         "in_features 5 != 6"),
        ("edge backward: width", lambda: L.csmpn_egcl_edge_backward_f64(m3, 3, wide, gr, 1, 8, 3, 8, 2, 8, 8, 8, 2, 4, 8, 8, None, 8, big,
                                                                          None), UNS, "above the limit of 64"),
        ("node: N < 0", lambda: L.csmpn_egcl_node_forward_f64(m3, 3, ok, 2, 8, 2, 8, 2, 8, 1, 8, 1, 0, -3, 8, 8, big, None), INV,
         "negative row count"),
        ("node: residual width", lambda: L.csmpn_egcl_node_forward_f64(m3, 3, ok, 2, 8, 2, 8, 2, 8, 1, 8, 1, 1, 3, 8, 8, big, None), INV,
         "residual needs"),
        ("node: in_degree null", lambda: L.csmpn_egcl_node_forward_f64(m3, 3, ok, 2, 8, 2, 8, 2, 8, 1, None, 1, 0, 3, 8, 8, big, None), INV,
         "in_degree is null"),
        ("node backward: gh null", lambda: L.csmpn_egcl_node_backward_f64(m3, 3, ok, gr, 2, 8, 2, 8, 2, 8, 1, 8, 1, 0, 3, 8, None, 8, None, 8,
                                                                          big, None), INV, "null"),
        ("segment sum: N < 0", lambda: L.csmpn_segment_reduce_f64(8, 16, -1, 8, None, None, None, 8, 0, None), INV, "segment sum"),
        ("segment sum: out null", lambda: L.csmpn_segment_reduce_f64(8, 16, 3, 8, None, None, None, None, 0, None), INV, "null"),
    ]
    for name, call, code, text in cases:
        rc = call()
        assert rc == code, (name, rc, L.csmpn_last_error())
        assert text in L.csmpn_last_error().decode(), (name, L.csmpn_last_error())
    # the query itself answers 0 for what the entry points reject
    for bp, nb, n, rows in [(wide, 1, 3, 3), (ok, 5, 3, 3), (ok, 2, 6, 3), (ok, 2, 3, -1), (broken, 2, 3, 3), (None, 2, 3, 3)]:
        assert int(L.csmpn_cemlp_f64_workspace_bytes(n, bp, nb, rows)) == 0
    # rows = 0 is no error and launches nothing (null data pointers allowed)
    assert fwd(m3, 3, ok, 2, None, 0, None, None, 0) == 0


def test_module_errors_on_the_host(pkg):
    """A CPU float64 tensor raises the 'no CPU fallback' error first, whatever the parameters' dtype."""
    alg = pkg.CliffordAlgebra((1.0, 1.0, 1.0))
    for m in (pkg.CEMLP(alg, 2, 2, 2), pkg.CEMLP(alg, 2, 2, 2).double()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros(3, 2, 8, dtype=torch.float64))


YARDSTICK_TABLE = {}


@pytest.mark.parametrize("kind,name", H.EGCL_FIXTURES)
def test_yardstick_table(kind, name):
    """Two independent float64 implementations of one function - the float64 C++ twin against the reference's float64
    fixture - agree to the documented level; the figures are what DESIGN.md §4.10 records."""
    worst = {}
    for variant in H.EGCL_TAGS:
        for k, y in H.egcl_yardsticks(kind, name, variant).items():
            cls = "params" if k.startswith("g/") else k
            worst[cls] = max(worst.get(cls, 0.0), y)
    YARDSTICK_TABLE[(kind, name)] = worst
    print(f"[f64] yardstick {kind}_{name}: " + "  ".join(f"{k} {v:.2e}" for k, v in sorted(worst.items())))
    # float64 agreement, nothing coarser (measured: 4.5e-15 .. 3.0e-13 on the 4-channel fixtures of the definite metrics,
    # 2.1e-12 on egcl8_cl30's parameter gradients, up to 5.8e-12 on Cl(4,1))
    assert all(0 < v <= 1e-10 for v in worst.values()), worst
    # ... and the table DESIGN.md §4.10 states is this one: every documented figure within a factor 2 of the recomputed one
    # (the twin's figures move by an ulp or so with the host's libm, not by more)
    rows = [l for l in open(os.path.join(H.ROOT, "DESIGN.md")).read().splitlines() if l.startswith(f"| {kind}_{name} |")]
    assert len(rows) == 1, rows
    documented = dict(zip(["y", "gh", "g_edge_attr", "g_node_attr", "params"], (float(c) for c in rows[0].strip("| ").split("|")[1:])))
    for k, v in worst.items():
        assert 0.5 <= documented[k] / v <= 2.0, (kind, name, k, documented[k], v)


def test_comparison_can_fail():
    """The comparison helper fails on a 1e-10 relative perturbation of one element (and passes on the exact tensor)."""
    c = H.egcl_case("egcl", "cl30", "sum_res1_ag1")
    yard = H.egcl_yardsticks("egcl", "cl30", "sum_res1_ag1")
    for k in ("y", "gh", "g/edge_model.layers.0.0.weight"):
        truth = c["truth"][k]
        H.assert_close(k, truth.copy(), truth, yard[k])
        bad = truth.copy()
        i = np.unravel_index(np.abs(bad).argmax(), bad.shape)
        bad[i] *= 1.0 + 1e-10
        with pytest.raises(AssertionError):
            H.assert_close(k, bad, truth, yard[k])
    with pytest.raises(AssertionError):
        H.assert_close("nan", np.full_like(c["truth"]["y"], np.nan), c["truth"]["y"], 1.0)


def test_batch_to_casts_features_only(pkg):
    g = H.load("model", "motion")
    b32 = H.load_batch(g)
    b64 = H.load_batch(g, dtype=torch.float64)
    for k in b32._names:
        t32, t64 = getattr(b32, k), getattr(b64, k)
        assert t64.dtype == (torch.float64 if t32.is_floating_point() else t32.dtype), k
        assert torch.equal(t64.to(t32.dtype), t32)


@pytest.mark.parametrize("kind", ["motion", "nba", "md17"])
def test_model_glue_runs_in_float64_on_the_host(pkg, monkeypatch, kind):
    """The models' composed glue follows the feature dtype: with the layers computed by the oracle, a .double() model on a
    float64 batch reproduces the reference's float64 loss and gradient figures to float64 accuracy (float32 glue anywhere
    in between would leave errors of 1e-7)."""
    H.host_oracle_injection(monkeypatch.setattr)
    loss, gn, _ = H.model_step(kind, torch.float64)
    errs = H.model_errors(kind, loss, gn)
    print(f"[f64] host model {kind}: worst {max(errs.values()):.3e} loss {errs['backprop_loss']:.3e}")
    assert max(errs.values()) <= 1e-10, sorted(errs.items(), key=lambda kv: -kv[1])[:3]
