"""Host side of the run-time-signature kernel family (no GPU): the two support queries on all 60 signatures, the host
restatement of the sign rule against the library's Cayley tensor, the float workspace query against its documented formula,
every rejected argument combination of the seven *_sig entry points (code and message, without a device), what the *_f64
entry points now accept, the conditioning of the fixtures (which variant the float32 leg leaves out) and a guard that the
sign comparison can fail. The rules: tests/signature_helpers.py."""
import os
import re

import numpy as np
import pytest

import signature_helpers as H

NEW = ["csmpn_signature_supported", "csmpn_cemlp_sig_workspace_bytes", "csmpn_cemlp_forward_sig", "csmpn_cemlp_backward_sig",
       "csmpn_egcl_edge_forward_sig", "csmpn_egcl_edge_backward_sig", "csmpn_egcl_node_forward_sig", "csmpn_egcl_node_backward_sig"]


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


def test_support_queries_truth_table(pkg):
    from csmpn_hip import native
    L, arr = native.lib(), native.metric_array
    sigs = H.all_signatures()
    assert len(sigs) == 60 and len({m for _, _, m in sigs}) == 60
    for n, neg, metric in sigs:
        assert L.csmpn_signature_supported(arr(metric), n) == 1, metric
        assert L.csmpn_metric_supported(arr(metric), n) == (1 if (n, neg) in H.COMPILED else 0), metric
        alg = pkg.CliffordAlgebra(metric)
        assert alg.hip_signature is True and alg.hip_supported is ((n, neg) in H.COMPILED)
    assert sum(L.csmpn_metric_supported(arr(m), n) for n, _, m in sigs) == 6
    assert L.csmpn_metric_supported(arr(H.SIGNATURES["cl13"]), 4) == 0
    for metric in [(1.0,), (-1.0,), (1.0,) * 6, (1.0, -1.0, 1.0, -1.0, 1.0, -1.0), (1.0, 0.0, 1.0), (1.0, 0.5), (1.0, -1.0, 2.0, 1.0),
                   (float("nan"), 1.0)]:
        assert L.csmpn_signature_supported(arr(metric), len(metric)) == 0, metric
        assert L.csmpn_metric_supported(arr(metric), len(metric)) == 0, metric
    assert L.csmpn_signature_supported(None, 3) == 0
    assert pkg.CliffordAlgebra((1.0, 0.5)).hip_signature is False


def _library_tables(pkg, metric):
    from csmpn.algebra.metric import native_tables
    return native_tables(tuple(metric))


def test_sign_rule_restated_on_the_host_is_the_library_cayley_tensor(pkg):
    """sign, output index and qsign of the rule (structural table of the all-positive signature, flipped by the parity of the
    shared negative generators) against csmpn_algebra_tables, which builds the Cayley tensor from the metric itself."""
    for n, neg, metric in H.all_signatures():
        cay = np.asarray(_library_tables(pkg, metric)["cayley"], np.float64)
        sign, out, qsign = H.sign_rule(n, neg)
        D = 1 << n
        assert cay.shape == (D, D, D)
        assert np.array_equal(H.cayley_from_rule(n, neg), cay), metric
        assert np.array_equal(np.abs(cay).sum(axis=1), np.ones((D, D)))          # one output blade per pair
        assert np.array_equal(np.argmax(np.abs(cay), axis=1), out), metric
        grade = np.array([bin(b).count("1") for b in H.blade_bitmaps(n)])
        beta = np.where((grade * (grade - 1) // 2) % 2 == 0, 1, -1)
        assert np.array_equal(qsign, beta * cay[np.arange(D), 0, np.arange(D)]), metric


def test_a_flipped_sign_fails_the_comparison(pkg):
    """Mutation guard: one sign of the host rule flipped and the comparison above does not hold."""
    for n, neg, metric in [(2, 0x2, (1.0, -1.0)), (4, 0xe, H.SIGNATURES["cl13"]), (5, 0x1c, H.SIGNATURES["cl23"])]:
        cay = np.asarray(_library_tables(pkg, metric)["cayley"], np.float64)
        D = 1 << n
        assert np.array_equal(H.cayley_from_rule(n, neg), cay)
        for i, k in [(1, 1), (D - 1, D - 1), (1, D - 1), (D // 2, 2)]:
            assert not np.array_equal(H.cayley_from_rule(n, neg, flip_one=(i, k)), cay), (metric, i, k)
        assert not np.array_equal(H.cayley_from_rule(n, neg ^ 1), cay)             # another signature is another table


@pytest.mark.parametrize("n,widths", [(2, [(5, 4), (4, 4)]), (3, [(14, 8), (8, 8)]), (5, [(3, 64)]), (5, [(34, 28), (28, 28)]),
                                      (4, [(5, 4)] + [(4, 4)] * 3), (2, [(2, 2)]), (5, [(2, 31)]), (5, [(2, 32)])])
def test_float_workspace_query_is_the_documented_formula_and_monotone(pkg, n, widths):
    from csmpn_hip import native
    bp = _blocks(native, widths)
    R, _, _, _, lds = H.plan32(n, widths, 1)
    assert 1 <= R <= 32 and lds <= 163840
    cap = 512 if lds <= 65536 else 256
    last = 0
    for rows in sorted({0, 1, R - 1, R, R + 1, 2 * R, cap * R, cap * R + 1, 10 * cap * R}):
        got = int(native.lib().csmpn_cemlp_sig_workspace_bytes(n, bp, len(widths), rows))
        _, tiles, grid, want, _ = H.plan32(n, widths, rows)
        assert got == want, (rows, got, want)
        assert grid == min(tiles, cap) and got >= last
        last = got
    assert int(native.lib().csmpn_cemlp_sig_workspace_bytes(n, bp, len(widths), 0)) == 0
    # the float64 query does not depend on the metric and is what it was
    assert int(native.lib().csmpn_cemlp_f64_workspace_bytes(n, bp, len(widths), 3)) == H.plan64(n, widths, 3)[3]


def test_rejected_arguments_return_their_code_and_message_without_a_device(pkg):
    from csmpn_hip import native
    L, INV, UNS = native.lib(), native.ERR_INVALID, native.ERR_UNSUPPORTED
    m4, bad = native.metric_array(H.SIGNATURES["cl13"]), native.metric_array([1, -1, 0.5, 1])
    ok = _blocks(native, [(5, 4), (4, 4)])
    wide = _blocks(native, [(5, 65)])
    broken = _blocks(native, [(5, 4), (3, 4)])
    nullp = _blocks(native, [(5, 4)], ptr=None)
    gr = (native.BlockGrads * 2)()
    big = 1 << 30
    need = H.plan32(4, [(5, 4), (4, 4)], 3)[3]
    fwd = lambda metric, n, bp, nb, x, rows, y, ws, wsb: L.csmpn_cemlp_forward_sig(metric, n, bp, nb, x, rows, y, ws, wsb, None)
    bwd = lambda metric, n, bp, g, nb, x, gy, rows, gx, ws, wsb: L.csmpn_cemlp_backward_sig(metric, n, bp, g, nb, x, gy, rows, gx, ws, wsb, None)
    ef = lambda bp, nb, perm, E, N, C=3, wsb=big, metric=m4, n=4: L.csmpn_egcl_edge_forward_sig(metric, n, bp, nb, 8, C, 8, 2, perm, 8, 8, E, N, 8, 8,
                                                                                              wsb, None)
    eb = lambda bp, nb, g_agg, wsb=big, metric=m4, n=4: L.csmpn_egcl_edge_backward_sig(metric, n, bp, gr, nb, 8, 3, 8, 2, 8, 8, 8, 2, 4, g_agg, 8,
                                                                                     None, 8, wsb, None)
    nf = lambda bp, nb, deg, resid, N, wsb=big, metric=m4, n=4: L.csmpn_egcl_node_forward_sig(metric, n, bp, nb, 8, 2, 8, 2, 8, 1, deg, 1, resid, N,
                                                                                            8, 8, wsb, None)
    nb_ = lambda bp, nb, gh, wsb=big, metric=m4, n=4: L.csmpn_egcl_node_backward_sig(metric, n, bp, gr, nb, 8, 2, 8, 2, 8, 1, 8, 1, 0, 3, 8, gh, 8,
                                                                                   None, 8, wsb, None)
    six = native.metric_array([1] * 6)
    cases = [
        ("x null", lambda: fwd(m4, 4, ok, 2, None, 3, 8, 8, big), INV, "null"),
        ("y null", lambda: fwd(m4, 4, ok, 2, 8, 3, None, 8, big), INV, "null"),
        ("blocks null", lambda: fwd(m4, 4, None, 2, 8, 3, 8, 8, big), INV, "blocks is null"),
        ("metric null", lambda: fwd(None, 4, ok, 2, 8, 3, 8, 8, big), INV, "metric is null"),
        ("parameter null", lambda: fwd(m4, 4, nullp, 1, 8, 3, 8, 8, big), INV, "null parameter"),
        ("n = 6", lambda: fwd(six, 6, ok, 2, 8, 3, 8, 8, big), UNS, "metric not supported by the HIP path"),
        ("n = 1", lambda: fwd(m4, 1, ok, 2, 8, 3, 8, 8, big), UNS, "metric not supported by the HIP path"),
        ("metric 0.5", lambda: fwd(bad, 4, ok, 2, 8, 3, 8, 8, big), UNS, "metric not supported by the HIP path"),
        ("0 blocks", lambda: fwd(m4, 4, ok, 0, 8, 3, 8, 8, big), INV, "blocks not in 1..4"),
        ("5 blocks", lambda: fwd(m4, 4, ok, 5, 8, 3, 8, 8, big), INV, "blocks not in 1..4"),
        ("width 65", lambda: fwd(m4, 4, wide, 1, 8, 3, 8, 8, big), UNS, "above the limit of 64"),
        ("chain", lambda: fwd(m4, 4, broken, 2, 8, 3, 8, 8, big), INV, "in_features 3 of block 1"),
        ("small workspace", lambda: fwd(m4, 4, ok, 2, 8, 3, 8, 8, need - 1), INV, "workspace of"),
        ("workspace null", lambda: fwd(m4, 4, ok, 2, 8, 3, 8, None, big), INV, "workspace of"),
        ("rows < 0", lambda: fwd(m4, 4, ok, 2, 8, -1, 8, 8, big), INV, "negative row count"),
        ("backward: grads null", lambda: bwd(m4, 4, ok, None, 2, 8, 8, 3, 8, 8, big), INV, "grads is null"),
        ("backward: gy null", lambda: bwd(m4, 4, ok, gr, 2, 8, None, 3, 8, 8, big), INV, "null"),
        ("backward: 5 blocks", lambda: bwd(m4, 4, ok, gr, 5, 8, 8, 3, 8, 8, big), INV, "blocks not in 1..4"),
        ("backward: width", lambda: bwd(m4, 4, wide, gr, 1, 8, 8, 3, 8, 8, big), UNS, "above the limit of 64"),
        ("backward: small workspace", lambda: bwd(m4, 4, ok, gr, 2, 8, 8, 3, 8, 8, need - 1), INV, "workspace of"),
        ("backward: n = 6", lambda: bwd(six, 6, ok, gr, 2, 8, 8, 3, 8, 8, big), UNS, "not supported"),
        ("edge: E < 0", lambda: ef(ok, 2, 8, -1, 4), INV, "negative row count"),
        ("edge: N < 0", lambda: ef(ok, 2, 8, 2, -4), INV, "negative node count"),
        ("edge: perm null", lambda: ef(ok, 2, None, 2, 4), INV, "null"),
        ("edge: channels", lambda: ef(ok, 2, 8, 2, 4, C=4), INV, "in_features 5 != 6"),
        ("edge: 0 blocks", lambda: ef(ok, 0, 8, 2, 4), INV, "blocks not in 1..4"),
        ("edge: metric 0.5", lambda: ef(ok, 2, 8, 2, 4, metric=bad), UNS, "not supported"),
        ("edge: small workspace", lambda: ef(ok, 2, 8, 2, 4, wsb=H.plan32(4, [(5, 4), (4, 4)], 2)[3] - 1), INV, "workspace of"),
        ("edge backward: width", lambda: eb(wide, 1, 8), UNS, "above the limit of 64"),
        ("edge backward: g_agg null", lambda: eb(ok, 2, None), INV, "null"),
        ("edge backward: chain", lambda: eb(broken, 2, 8), INV, "in_features 3 of block 1"),
        ("edge backward: n = 6", lambda: eb(ok, 2, 8, metric=six, n=6), UNS, "not supported"),
        ("node: N < 0", lambda: nf(ok, 2, 8, 0, -3), INV, "negative row count"),
        ("node: residual width", lambda: nf(ok, 2, 8, 1, 3), INV, "residual needs"),
        ("node: in_degree null", lambda: nf(ok, 2, None, 0, 3), INV, "in_degree is null"),
        ("node: 5 blocks", lambda: nf(ok, 5, 8, 0, 3), INV, "blocks not in 1..4"),
        ("node: small workspace", lambda: nf(ok, 2, 8, 0, 3, wsb=need - 1), INV, "workspace of"),
        ("node backward: gh null", lambda: nb_(ok, 2, None), INV, "null"),
        ("node backward: width", lambda: nb_(wide, 1, 8), UNS, "above the limit of 64"),
        ("node backward: metric 0.5", lambda: nb_(ok, 2, 8, metric=bad), UNS, "not supported"),
        ("node backward: small workspace", lambda: nb_(ok, 2, 8, wsb=need - 1), INV, "workspace of"),
    ]
    for name, call, code, text in cases:
        rc = call()
        assert rc == code, (name, rc, L.csmpn_last_error())
        assert text in L.csmpn_last_error().decode(), (name, L.csmpn_last_error())
    for bp, nb, n, rows in [(wide, 1, 4, 3), (ok, 5, 4, 3), (ok, 2, 6, 3), (ok, 2, 1, 3), (ok, 2, 4, -1), (broken, 2, 4, 3), (None, 2, 4, 3)]:
        assert int(L.csmpn_cemlp_sig_workspace_bytes(n, bp, nb, rows)) == 0
    # rows = 0 is no error and launches nothing (null data pointers allowed), on a compiled algebra too
    assert fwd(m4, 4, ok, 2, None, 0, None, None, 0) == 0
    assert fwd(native.metric_array([1, 1, 1, 1]), 4, ok, 2, None, 0, None, None, 0) == 0


def test_float64_entry_points_take_every_signature(pkg):
    """cl13 passes the metric check of the *_f64 entry points: what follows is INVALID for a null workspace, not UNSUPPORTED;
    the float32 entry points of the general path still reject it."""
    from csmpn_hip import native
    L, INV, UNS = native.lib(), native.ERR_INVALID, native.ERR_UNSUPPORTED
    m4 = native.metric_array(H.SIGNATURES["cl13"])
    ok = _blocks(native, [(5, 4), (4, 4)])
    gr = (native.BlockGrads * 2)()
    big = 1 << 30
    calls = [
        lambda ws, b: L.csmpn_cemlp_forward_f64(m4, 4, ok, 2, 8, 3, 8, ws, b, None),
        lambda ws, b: L.csmpn_cemlp_backward_f64(m4, 4, ok, gr, 2, 8, 8, 3, 8, ws, b, None),
        lambda ws, b: L.csmpn_egcl_edge_forward_f64(m4, 4, ok, 2, 8, 3, 8, 2, 8, 8, 8, 2, 4, 8, ws, b, None),
        lambda ws, b: L.csmpn_egcl_edge_backward_f64(m4, 4, ok, gr, 2, 8, 3, 8, 2, 8, 8, 8, 2, 4, 8, 8, None, ws, b, None),
        lambda ws, b: L.csmpn_egcl_node_forward_f64(m4, 4, ok, 2, 8, 2, 8, 2, 8, 1, 8, 1, 0, 3, 8, ws, b, None),
        lambda ws, b: L.csmpn_egcl_node_backward_f64(m4, 4, ok, gr, 2, 8, 2, 8, 2, 8, 1, 8, 1, 0, 3, 8, 8, 8, None, ws, b, None),
    ]
    for call in calls:
        assert call(None, big) == INV and "workspace of" in L.csmpn_last_error().decode(), L.csmpn_last_error()
        assert call(8, 7) == INV and "workspace of" in L.csmpn_last_error().decode()
    assert L.csmpn_cemlp_forward_f64(m4, 4, ok, 2, None, 0, None, None, 0, None) == 0
    assert int(L.csmpn_cemlp_f64_workspace_bytes(4, ok, 2, 3)) == H.plan64(4, [(5, 4), (4, 4)], 3)[3] > 0
    assert L.csmpn_cemlp_forward_f64(native.metric_array([1, -1, 0.5, 1]), 4, ok, 2, 8, 3, 8, 8, big, None) == UNS
    assert L.csmpn_cemlp_workspace_bytes(4, ok, 2) > 0
    assert L.csmpn_cemlp_forward(m4, 4, ok, 2, 8, 3, 8, None, 8, big, 0, None) == UNS
    assert "metric not supported by the HIP path" in L.csmpn_last_error().decode()


def test_fixture_conditioning_and_the_excluded_variant():
    """The float32 yardsticks recomputed: at most one of the 35 (signature, variant) pairs is left out of the float32 leg
    (cl23 / noattr, where float32 itself is off by tens of percent), and cl03 and cl31x keep every float32 yardstick at or
    below 1e-4, so the float32 leg has force. The float64 yardsticks are float64 agreement everywhere."""
    out, worst64 = [], 0.0
    for name in H.SIGNATURES:
        for variant in H.TAGS:
            y64, y32, pair = H.yardsticks(name, variant)
            k = max(y32, key=y32.get)
            print(f"[sig] yardstick {name}/{variant}: f64 {max(y64.values()):.2e}  f32 {y32[k]:.2e} ({k}: reference {pair[k][0]:.2e}, "
                  f"twin {pair[k][1]:.2e})")
            worst64 = max(worst64, max(y64.values()))
            if H.excluded(name, variant):
                out.append((name, variant))
            if name in ("cl03", "cl31x"):
                # compared at the two significant digits the figures of this rule are stated in: the largest one, the twin's
                # float32 error on cl03 / mean_res*_ag0 / edge_model.layers.0.0.bias, is 1.0039e-4 = "1.0e-4"
                assert float(f"{max(y32.values()):.1e}") <= 1e-4, (name, variant, y32)
    assert len(out) <= 1 and out == [("cl23", "noattr")], out
    assert 0 < worst64 <= 1e-9, worst64
