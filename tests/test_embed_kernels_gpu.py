"""GPU: the fused simplex embedding (csmpn_embed_cemlp_forward / _backward: MODE_PLAIN of csrc/cemlp_plw.hpp with the embed
descriptor) against float64 at its group edges. Cases, inputs, reference and the child-process side: tests/embed_helpers.py;
the reference itself is checked without a GPU by tests/test_embed_reference_cpu.py.

Each group of cases runs in one child process with CSMPN_DEBUG=1 CSMPN_QUIET=1 and the group's switches; the child runs the
HIP side (every comparison case twice: all tensors must be bit-identical, the entry points take no deterministic flag) and
stores the tensors; the references are computed once per shape on the host.

    group      environment          what runs
    default    -                    every case through ops.embed_cemlp_apply; two-block modules with CSMPN_FLAG_SAVE_STATE
    recompute  CSMPN_SAVE_STATE=0   the two-block cases and the triangle walk on the backward without saved state
    abi        -                    the C-ABI called directly (sentinels, clamp, refusals, predicate sweep) and the models

Cases (each on Cl(5,0) and Cl(4,1) unless noted; rows = simplices x orders):
    edges program 2 -> 28, one block, 2 orders, 1 / 2 / 3 / 5 / 23 simplices: partial tiles, fewer rows than a tile
    triangles program 3 -> 28 -> 28, 6 orders, 1 / 2 / 3 / 5 / 23 simplices: 2 fill one 12-row group, the others end in a group
        of one simplex and a half tile
    what the C-ABI admits and the model never makes: 1 order with 1 vertex x 2 channels; 2 orders on the two-block program
        with 1 vertex x 3 channels; 6 orders on the one-block program; 1 order with 3 vertices - 7 simplices each
    walks, Cl(5,0): 1031 edges = 2062 rows = 516 tiles (4 workgroups of the 512 take a second tile; the backward's 256 stride),
        1031 triangles = 6186 rows = 1547 tiles = 516 groups (the last one: two tiles, one of 2 rows, a single simplex)
Each walk proves from its own `[csmpn] plw mode=0 ..` lines that rows > grid x 4 x GT in the forward (GT = 3 for 6 orders, else
1) and rows > grid x 4 in the backward with the grid at its cap; every other case proves <=.

Inputs: 97 feature rows of which the last 8 are never referenced and hold 3e4 (a stray read lands far outside the bound);
every table holds id 0, id 88, and where it is large enough a simplex of one repeated id and two identical simplices.

Bound: general_helpers.check unchanged - per tensor max(1e-5, 4 x float32 yardstick), 10 x that per element - under the
condition, asserted on the references, that every yardstick of every case is at most 1e-5 (seed offsets:
embed_helpers.RESEED).
"""
import math

import numpy as np
import pytest
import torch

import embed_helpers as E
from embed_helpers import CASES, CL50

pytestmark = pytest.mark.gpu


def _ok(tag):
    r = E.result(tag)
    print(tag, r["message"], *r["log"], sep="\n")
    assert r["ok"], r["message"]
    return r


def _tags(kind, group=None):
    return [t for t, c in CASES.items() if c["kind"] == kind and group in (None, c["group"])]


# ------------------------------------------------------------------------------------------------------- comparisons
@pytest.mark.parametrize("group", ["default", "recompute"])
def test_embed_against_float64(group):
    """Every case of the group: out and every parameter gradient within the bound of the float64 reference; two runs,
    bit-identical (asserted in the child); each launch on plw with the case's rows; walks exactly where the table says.
    Measured on one MI355X: HIP error 4.8e-7 .. 5.2e-6 (0.05 .. 0.26 of the bound), the walks 9.6e-7 and 1.7e-6; nearest its
    bound in both groups: g.layers.1.2.linear_right.weight of abi-cl41-o2-v1k3, 1.25e-5 with a float32 yardstick of 4.6e-6 on
    that host (0.67 of the bound)."""
    failures, nearest = [], (0.0, "")
    for tag in _tags("embed", group):
        c = CASES[tag]
        try:
            t64, t32 = E.reference(c["seed_tag"])
            r = _ok(tag)
            msg, ratio = E.compare(tag, r["got"], t64, t32)
            print(f"{tag}: {msg} ({ratio:.2f} of its bound)")
            nearest = max(nearest, (ratio, f"{tag}: {msg}"))
            runs = E.launches(r)
            assert [n for n, _ in runs] == ["", "run 2"], r["log"]
            for _, ls in runs:
                E.check_launches(c, ls, tag)
        except AssertionError as e:
            failures.append(f"{tag}: {str(e)[-1500:]}")
    print(f"group {group}: nearest its bound: {nearest[1]} ({nearest[0]:.2f} of the bound)")
    assert not failures, "\n".join(failures)


# --------------------------------------------------------------------------------------------------------- sentinels
@pytest.mark.parametrize("tag", _tags("guard"))
def test_sentinels(tag):
    """The C-ABI on out of exactly nsimp x 28 x 32 floats (NaN before the call: it needs no zeroing), a saved buffer of exactly
    csmpn_cemlp_saved_floats floats and a workspace of exactly csmpn_cemlp_workspace_bytes bytes, each between sentinels with a
    NaN interior; with CSMPN_FLAG_SAVE_STATE and with flags 0: sentinels intact, results finite and within the bound."""
    c = CASES[tag]
    t64, t32 = E.reference(c["seed_tag"])
    r = _ok(tag)
    got = r["got"]
    runs = E.launches(r)
    assert [n for n, _ in runs] == list(E.GUARD_VARIANTS), r["log"]
    floats = {}
    for v, ls in runs:
        E.check_launches(c, ls, f"{tag} {v}")
        assert int(got[f"{v}.floats.out"]) == c["nsimp"] * 28 * 32
        for k in ("out", "saved", "ws"):
            assert bool(got[f"{v}.intact.{k}"]), f"{tag} {v}: a sentinel around {k} is gone"
        mine = {k[len(v) + 1:]: a for k, a in got.items() if k.startswith(v + ".y") or k.startswith(v + ".g.")}
        assert all(np.isfinite(a).all() for a in mine.values()), [k for k, a in mine.items() if not np.isfinite(a).all()]
        print(v, E.compare(f"{tag} {v}", mine, t64, t32)[0])
        floats[v] = int(got[f"{v}.floats.saved"])
    rows = c["nsimp"] * c["n_orders"]
    if c["nl"] == 2:    # the block-1 inputs; the flag adds the state regions
        assert floats["noflag"] >= rows * 28 * 32 and floats["state"] > floats["noflag"], floats
    else:
        assert floats == {"state": 0, "noflag": 0}, floats


# ------------------------------------------------------------------------------------------------- clamp and validation
@pytest.mark.parametrize("tag", _tags("clamp"))
def test_clamp_and_validation(tag):
    """A table that holds -1, S and S + 1000. Validated (no flag): CSMPN_ERR_INVALID, "outside" in the message, out and the
    gradients untouched (asserted in the child), nothing launched. With CSMPN_FLAG_NO_VALIDATE: the result of the table clamped
    into [0, S - 1], as include/csmpn_hip.h documents."""
    c = CASES[tag]
    t64, t32 = E.reference(c["seed_tag"], c, E.clamped)
    r = _ok(tag)
    runs = dict(E.launches(r))
    assert sorted(runs) == ["clamped", "validated"] and not runs["validated"], r["log"]    # the refused calls launched nothing
    E.check_launches(c, runs["clamped"], tag)
    print(E.compare(tag, r["got"], t64, t32)[0])
    # the comparison tells the clamp from any other reading of the bad ids: against the reference of ids wrapped modulo S it fails
    feat, verts, p, gout = E.case_inputs(c, E.SUITE.seed_of(c["seed_tag"]))
    wrapped = E.reference_run(c["metric"], feat, verts % E.S_ROWS, c["n_orders"], p, gout, torch.float64)
    yard = {k: t32[k].astype(np.float64) + (wrapped[k] - t64[k]) for k in t64}    # the same yardsticks around the other truth
    with pytest.raises(AssertionError):
        E.compare(tag, r["got"], wrapped, yard)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """n_rows % n_orders != 0 and n_vertex_rows = 0: CSMPN_ERR_INVALID; 3 orders, nv x kpv != in_features, nv x kpv > 8,
    Cl(3,0), a two-block backward without saved inputs: CSMPN_ERR_UNSUPPORTED. Codes and untouched outputs are asserted in the
    child; here: nothing was launched by a refused call."""
    E.G._pkg()
    from csmpn_hip import native
    r = _ok("refusals@abi")
    got = r["got"]
    want = dict.fromkeys(E.REFUSALS, native.ERR_UNSUPPORTED)
    want.update({"rows-not-multiple": native.ERR_INVALID, "no-vertex-rows": native.ERR_INVALID})
    assert {k: int(v) for k, v in got.items()} == want
    runs = E.launches(r)
    assert [n.split(":")[0] for n, _ in runs] == [f"refused {k}" for k in E.REFUSALS if k != "no-saved-inputs"] + [
        "forward for the backward refusal", "backward refusal", "refused no-saved-inputs"], r["log"]
    for note, ls in runs:    # the one launch: the forward in front of the refused backward
        assert [(l["family"], l["bwd"]) for l in ls] == ([("plw", 0)] if note.startswith("forward for") else []), (note, ls)


# --------------------------------------------------------------------------------------------- predicate against library
def test_predicate_matches_library():
    """Both algebras x out 8 / 16 / 24 / 28 / 32 / 40 x (in_features, blocks) (2, 1), (3, 2), (2, 2), (3, 1), (4, 1), (6, 2) at 6
    rows: ops.embed_cemlp_supported is True exactly where csmpn_embed_cemlp_forward returns CSMPN_OK (every other cell:
    CSMPN_ERR_UNSUPPORTED, out untouched, nothing launched); every served cell is held to the reference."""
    r = _ok("sweep@abi")
    got = r["got"]
    runs = dict(E.launches(r))
    served, wrong = [], []
    for cell in E.sweep_cells():
        c = E.sweep_case(*cell)
        name = c["seed_tag"]
        rc, sup = int(got[f"{name}.rc"]), bool(got[f"{name}.supported"])
        if sup != (rc == 0):
            wrong.append(f"{name}: predicate {sup}, library returned {rc}")
        if rc == 0:
            served.append(cell)
            E.check_launches(c, runs[name], name)
            t64, t32 = E.reference(name, c)
            mine = {k[len(name) + 1:]: a for k, a in got.items() if k.startswith(name + ".y") or k.startswith(name + ".g.")}
            print(name, E.compare(name, mine, t64, t32)[0])
        else:
            assert not runs.get(name), (name, runs[name])
    assert not wrong, "\n".join(wrong)
    # the two programs csrc/plw_inst.inc instantiates for MODE_PLAIN are served on both algebras
    assert {(an, 28, in_f, nl) for an in E.ALGS for in_f, nl in ((2, 1), (3, 2))} <= set(served), served


# ------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("hidden,kpv", E.MODEL_SHAPES)
def test_model_embedding(hidden, kpv):
    """SimplexEmbedding of HullsSimplicialMPNN(num_layers=1) at 16 / 24 / 28 / 32 channels, and at 28 with a 2-channel vertex
    block, on a hull batch of 3 graphs: forward + backward run on the device at every width - fused where the predicate holds
    (embed_launches() advances by 2: edges and triangles), composed from simplex_rows + CEMLP + sum elsewhere (by 0) -, and the
    rows of dimension >= 1 and the gradients of cl_feature_embedding[1:] meet the reference, with the module's own parameters.
    The hulls model then trains one step (Adam) on the device: finite loss, every parameter moved."""
    tag = f"model-{hidden}-k{kpv}@abi"
    r = _ok(tag)
    got = r["got"]
    pred = bool(got["predicate"])
    assert pred == ((hidden, kpv) == (28, 1)), "the predicate is the two instantiated programs: out 28, one channel per vertex"
    assert int(got["launches"]) == (2 if pred else 0)
    feat = torch.from_numpy(got["feat"])
    for k in (1, 2):
        prefix = f"p{k}."
        p = {n[len(prefix):]: torch.from_numpy(a) for n, a in got.items() if n.startswith(prefix)}
        assert len(p) == 10 * k
        verts, w = torch.from_numpy(got[f"verts{k}"]), torch.from_numpy(got[f"w{k}"])
        t64, t32 = (E.reference_run(CL50, feat, verts, math.factorial(k + 1), p, w, dt) for dt in (torch.float64, torch.float32))
        mine = {"y": got[f"x{k}"], **{"g." + n: got[f"g{k}.{n}"] for n in p}}
        print(k, verts.shape, E.compare(f"{tag} d={k}", mine, t64, t32)[0])
    if kpv == 1:
        assert np.isfinite(got["loss"]) and int(got["moved"]) >= 40, (got["loss"], got["moved"])


# --------------------------------------------------------------------------------------------------------- mutations
@pytest.mark.parametrize("tag", ["tris-cl50-23@default", "walk-tris-cl50-1031@default"], ids=["oracle", "walk"])
def test_comparison_can_fail(tag):
    """Results the way a bug of this code path would leave them must be rejected: one simplex built from 5 of its 6 orders,
    the last group's single simplex zeroed, the simplices of the second sweep copied from the first sweep's; and the stored
    result must be rejected by a reference whose parameter gradients leave out the rows of one tile, and by one whose backward
    reads g_out shifted by one simplex (the float32 yardstick run shifted alike, so that the bound stays what it is)."""
    c = CASES[tag]
    no, ns = c["n_orders"], c["nsimp"]
    t64, t32 = E.reference(c["seed_tag"])
    got = _ok(tag)["got"]
    E.compare(tag, got, t64, t32)
    feat, verts, p, gout = E.case_inputs(c, E.SUITE.seed_of(c["seed_tag"]))
    fwd = next(l for l in E.launches(E.result(tag))[0][1] if not l["bwd"])

    def rejected(name, mine, truth, yard):
        with pytest.raises(AssertionError):
            E.compare(f"{tag} {name}", mine, truth, yard)

    def with_y(fn):
        bad = dict(got)
        bad["y"] = got["y"].copy()
        fn(bad["y"])
        assert not np.array_equal(bad["y"], got["y"])
        return bad

    s = ns // 2
    one_order = E.reference_run(c["metric"], feat, verts[s * no + no - 1:s * no + no], 1, p, None, torch.float64)["y"][0]

    def five_orders(y):
        y[s] -= one_order.astype(np.float32)
    rejected("five of six orders", with_y(five_orders), t64, t32)

    def last_zeroed(y):
        y[-1] = 0.0
    rejected("last simplex zeroed", with_y(last_zeroed), t64, t32)
    sweep = min(fwd["grid"] * E.TILE * E.group_tiles(no) // no, ns // 2)    # simplices of one sweep of the forward grid

    def second_from_first(y):
        y[sweep:] = y[:ns - sweep].copy()
    rejected("second sweep from the first", with_y(second_from_first), t64, t32)

    def shifted(delta):    # both runs moved by the same float64 difference: every yardstick stays what it is
        return ({k: a + delta.get(k, 0.0) for k, a in t64.items()}, {k: a.astype(np.float64) + delta.get(k, 0.0) for k, a in t32.items()})
    tile = E.geometry(c)["tiles"] // 2
    part = E.row_gradients(c["metric"], feat, verts, no, p, gout, torch.arange(4 * tile, 4 * tile + 4))
    for k in sorted(part):    # each parameter gradient alone
        bad64, bad32 = shifted({k: -part[k]})
        rejected(f"{k} without tile {tile}", got, bad64, bad32)
    rolled = torch.roll(gout, 1, dims=0)
    delta = E.reference_run(c["metric"], feat, verts, no, p, rolled - gout, torch.float64)
    delta.pop("y")
    rejected("g_out shifted by one simplex", got, *shifted(delta))
