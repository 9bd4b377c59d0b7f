"""Cases, groups, expected dispatch and tile geometry of tests/test_lane_n3_gpu.py and tests/test_lane_n3_cpu.py: every
Cl(3,0) lane kernel at 16 and 32 channels - the channel-MFMA forward (cemlp_cm.hpp), its 16-channel backward with dynamic
tile claims (cemlp_cmb.hpp), the 32-channel wave-pair backward with and without saved state (cemlp_cmp.hpp), the 16-row-tile
EGCL and MODE_PLAIN programs (cemlp_pq.hpp, k_pq_n3.hip) - under every switch that routes a launch to another of them, and
each where a workgroup takes a second row tile.

Built on tests/general_helpers.py (Suite) with the division of work of tests/lane_d32_helpers.py: the child of a group runs the
HIP side of its cases only and stores every tensor (one .npz per case); the references are computed on the host ONCE per seed
tag - the same inputs run in up to seven groups - and the comparison happens there. A case of group `det` runs twice in its
child, which compares the two runs bit for bit itself. Behind the autograd run every EGCL case runs its four stages once more
on the child's main thread (csmpn_last_kernel is kept per thread, autograd's backward has its own) and notes the label of each.

Tags: `<seed tag>@<group>`; the seed follows from the seed tag.
"""
import atexit
import os
import re
import shutil
import tempfile

import numpy as np
import torch

import general_helpers as G
from general_helpers import CL30, Suite, relmax, say

D = 8
EA, NA = 6, 3    # attribute channels of the EGCL stages the units instantiate

# ------------------------------------------------------------------------------------------------------- tile geometry
# Rows of one workgroup iteration and workgroups of a launch at its cap (cm_grid, pq_grid of csrc/dispatch.hip; kCm*,
# kPqGridCap of csrc/launch.hpp; the tile loops of the kernels). A tile is 16 rows everywhere.
#   cm forward   tile t belongs to wave t % (4 gridDim) (kCmWaves = 4): 64 rows per iteration; cap kCmMaxFwdGroups = 768 at 16
#                channels, 256 at 32
#   cmb          16-channel backward: 8 waves (kCbWaves), claim n is tile (n >> 3) * 8 gridDim + 8 blockIdx + (n & 7): 128 rows
#                per iteration; cap kCmMaxBwdGroups = 256 (cm_grid asks for a workgroup per 4 tiles, so the grid is at its
#                cap from 16 321 rows on and walks past 32 768)
#   cmp          32-channel backward: a wave PAIR per tile, two pairs (kCpWaves / 2): 32 rows per iteration; cap 256
#   pq           one tile per workgroup iteration: 16 rows; cap kPqGridCap = 768
TILE = 16


def kernel_of(family, channels, bwd):
    if family == "pq":
        return "pq"
    assert family == "cm", family
    return "cm_fwd" if not bwd else ("cmb" if channels == 16 else "cmp")


def rows_per_iteration(family, channels, bwd):
    return {"pq": 16, "cm_fwd": 4 * 16, "cmb": 8 * 16, "cmp": 2 * 16}[kernel_of(family, channels, bwd)]


def grid_cap(family, channels, bwd):
    k = kernel_of(family, channels, bwd)
    if k == "pq":
        return 768
    if k == "cm_fwd":
        return 768 if channels == 16 else 256
    return 256


def sweep_rows(family, channels, bwd):
    """Rows one sweep of the grid holds: past it a wave (pq: a workgroup, cmp: a wave pair) takes a second row tile."""
    return grid_cap(family, channels, bwd) * rows_per_iteration(family, channels, bwd)


# --------------------------------------------------------------------------------------------------- expected dispatch
# (mode, bwd) of the launches: MODE_PLAIN 0, MODE_EDGE 1, MODE_NODE 2 (cemlp_device.hpp)
EDGE_F, NODE_F, NODE_B, EDGE_B = (1, 0), (2, 0), (2, 1), (1, 1)
EGCL_STAGES = (EDGE_F, NODE_F, NODE_B, EDGE_B)
PLAIN_F, PLAIN_B = (0, 0), (0, 1)
GENERAL = "general"    # the general row-tile kernels at the bottom of run_rows


def _fb(fwd, bwd, stages=EGCL_STAGES):
    return {s: (bwd if s[1] else fwd) for s in stages}


# The family of every launch by group and channels, derived from csrc/dispatch.hip and csmpn_hip/ops.py, not read off a run.
# kFamilies is walked in the order pq, pg, plw, pl, cl, cm and the first eligible family takes the launch; pg / plw / pl are
# D = 32 only, cl serves 8 channels only (serves(cemlp_cl_n3(), shape)).
#   pq_eligible  Cl(3,0), 32 channels, two uniform blocks (MODE_PLAIN: one or two), a shape of k_pq_n3.hip, not CSMPN_NO_PQ /
#                CSMPN_NO_CM; its BACKWARD only with a saved buffer and io.save_state.
#   cm_eligible  Cl(3,0), two uniform blocks, an EGCL stage, a shape of cm_inst.inc (16 / 32 channels), not CSMPN_NO_CM; its
#                BACKWARD only with a saved buffer and where cm_saved claims the shape (not under CSMPN_NO_CM_BWD).
#   io.save_state  the caller's CSMPN_FLAG_SAVE_STATE (ops.py: _SAVE_STATE = CSMPN_SAVE_STATE != 0, for a saved buffer of its
#                own), cleared by run_rows where saved_layout has no state regions: family_saved is pq_saved for the
#                MODE_PLAIN shapes and cm_saved for the EGCL shapes (3 x 2 x 32 channels at 32 channels, NONE at 16), both
#                empty under CSMPN_NO_CM_BWD. The standalone entry points honour the flag where pq_plain_shape holds.
#   the instantiation  cm_launch: 16 channels cemlp_cmb_kernel; 32 channels cemlp_cmp_kernel<.., true> with io.save_state and
#                two blocks, else <.., false>. cemlp_cm_fwd_kernel<32> writes state with io.save_state, else none.
# CSMPN_FLAG_DETERMINISTIC enters none of the eligibility functions: group `det` dispatches as `default` does (the flag selects
# the row-store form inside cemlp_cm.hpp / cemlp_cmb.hpp / cemlp_cmp.hpp / cemlp_pq.hpp - the fixed tile assignment in cmb -
# and the separate node / edge backward entry points in ops.py).
_PLAIN = (PLAIN_F, PLAIN_B)
EXPECTED = {
    "default": {16: _fb("cm", "cm"), 32: {**_fb("pq", "pq"), **_fb("pq", "pq", _PLAIN)}},
    # CSMPN_SAVE_STATE=0: 16 channels have no state regions anyway; at 32 pq's backward is not eligible and cm, last in the
    # table, recomputes (cmp <.., false>); a standalone CEMLP is no shape of cm's: the general kernels
    "recompute": {16: _fb("cm", "cm"), 32: {**_fb("pq", "cm"), **_fb("pq", GENERAL, _PLAIN)}},
    "nopq": {32: _fb("cm", "cm")},
    "nopq-recompute": {32: _fb("cm", "cm")},
    # CSMPN_NO_CM_BWD=1: no lane backward, no state regions; the forwards stay
    "nocmbwd": {16: _fb("cm", GENERAL), 32: {**_fb("pq", GENERAL), **_fb("pq", GENERAL, _PLAIN)}},
    "nopq-nocmbwd": {32: _fb("cm", GENERAL)},
}
EXPECTED.update({"det": EXPECTED["default"], "plain": EXPECTED["default"], "plain-recompute": EXPECTED["recompute"]})

GROUP_ENV = {"default": {}, "recompute": {"CSMPN_SAVE_STATE": "0"}, "nopq": {"CSMPN_NO_PQ": "1"},
             "nopq-recompute": {"CSMPN_NO_PQ": "1", "CSMPN_SAVE_STATE": "0"}, "nocmbwd": {"CSMPN_NO_CM_BWD": "1"},
             "nopq-nocmbwd": {"CSMPN_NO_PQ": "1", "CSMPN_NO_CM_BWD": "1"}, "det": {"CSMPN_DETERMINISTIC": "1"}, "plain": {},
             "plain-recompute": {"CSMPN_SAVE_STATE": "0"}}
GROUPS = {g: (env, (lambda g: lambda t: t.endswith("@" + g))(g)) for g, env in GROUP_ENV.items()}


def saves_state(group, channels):
    """The forward of the group writes the state regions and the backward reads them."""
    env = GROUP_ENV[group]
    return channels == 32 and "CSMPN_SAVE_STATE" not in env and "CSMPN_NO_CM_BWD" not in env


def expected_label(group, channels, stage, state=None):
    """What csmpn_last_kernel names behind the stage (cm_label, pq_label and the bottom of run_rows in csrc/dispatch.hip)."""
    family = EXPECTED[group][channels][stage]
    state = saves_state(group, channels) if state is None else state
    if family == GENERAL:
        return ("csmpn::cemlp_kernel<",)
    if family == "pq":
        return ("csmpn::cemlp_pq_%s_kernel<" % ("bwd" if stage[1] else "fwd"), f"(mode {stage[0]}, 32 channels")
    k = kernel_of(family, channels, stage[1])
    name = "csmpn::cemlp_%s_kernel<" % k
    return (name, ", true>" if state else ", false>") if k == "cmp" else (name,)


# --------------------------------------------------------------------------------------------------------- the cases
def _egcl(C, N, E, aggr, residual, rewire=False, ref="oracle", walks=()):
    return dict(kind="egcl", metric=CL30, C=C, hidden=C, N=N, E=E, aggr=aggr, residual=residual, attrs=True, rewire=rewire, ref=ref,
                walks=tuple(walks))


def _plain(nl, in_f, rows):
    return dict(kind="cemlp", metric=CL30, nl=nl, widths=(in_f, 32, 32), rows=rows, ref="twin" if rows > 1000 else "oracle",
                walks=(PLAIN_F, PLAIN_B) if rows > 12288 else ())


def _guard(kind, **k):
    return dict(kind=kind, metric=CL30, ref=None, walks=(), **k)


WIDTHS = (16, 32)
# (N, E, rewire: duplicates, a self loop, two isolated nodes): below one tile, one tile + one row, ragged tiles
SMALL_SHAPES = ((2, 1, False), (5, 3, False), (37, 101, True), (64, 258, False))
PLAIN_PROGRAMS = ((1, 60), (2, 90), (1, 32))    # (blocks, input channels) of k_pq_n3.hip's MODE_PLAIN entries
BASES = {}    # seed tag -> case
for _ci, _C in enumerate(WIDTHS):
    for _s, (_N, _E, _rw) in enumerate(SMALL_SHAPES):
        BASES[f"n3-{_C}-{_E}"] = _egcl(_C, _N, _E, "mean" if (_ci + _s) % 2 == 0 else "sum", (_ci + _s // 2) % 2 == 0, rewire=_rw)
# walks against the twin: one sweep of the stage's grid + a few whole tiles + a partial tile (sweeps: see sweep_rows)
BASES.update({
    # cm forward 49 152, cmb 32 768: all four stages walk
    "walk-cm-16": _egcl(16, 49173, 49205, "sum", True, ref="twin", walks=EGCL_STAGES),
    # only the backward walks; the forward stays in one sweep
    "walk-cmb-16": _egcl(16, 32789, 32821, "mean", False, ref="twin", walks=(NODE_B, EDGE_B)),
    # pq 12 288 both ways: all four stages, the node stage among them
    "walk-pq-32": _egcl(32, 12309, 12341, "mean", True, ref="twin", walks=EGCL_STAGES),
    # cmp 8 192 behind the pq forward (12 288: one sweep)
    "walk-cmp-32": _egcl(32, 8213, 8245, "sum", False, ref="twin", walks=(NODE_B, EDGE_B)),
    # cm forward at 32 channels 16 384; cmp walks further
    "walk-cm-32": _egcl(32, 16405, 16437, "sum", True, ref="twin", walks=EGCL_STAGES),
})
for _nl, _in in PLAIN_PROGRAMS:
    for _rows in (1, 23, 12341):
        BASES[f"plain-{_in}to32x{_nl}-{_rows}"] = _plain(_nl, _in, _rows)
# sentinels around the saved buffer and the workspace (hip_guard): rows that are no multiple of 16, and one walk size
_LAYER = dict(C=32, hidden=32, aggr="mean", residual=True, attrs=True, rewire=False)
BASES.update({
    "guard-egcl-39": _guard("guard_egcl", N=23, E=39, **_LAYER),
    "guard-egcl-pq-walk": _guard("guard_egcl", N=12309, E=12341, **_LAYER),
    "guard-egcl-cm-walk": _guard("guard_egcl", N=16405, E=16437, **_LAYER),
    "guard-plain-23": _guard("guard_cemlp", nl=2, widths=(90, 32, 32), rows=23),
    "guard-plain-walk": _guard("guard_cemlp", nl=2, widths=(90, 32, 32), rows=12341),
})


def _small(channels, edges=(1, 3, 101, 258)):
    return [f"n3-{C}-{E}" for C in channels for E in edges]


def _plains(rows):
    return [f"plain-{i}to32x{nl}-{r}" for nl, i in PLAIN_PROGRAMS for r in rows]


# which seed tags run in which group: the small matrix in every group that changes a launch of the width (`default`: one shape
# per width - test_lane_kernel_shapes runs these shapes there; `recompute` changes nothing at 16 channels: one shape shows it)
MEMBERS = {
    "default": ["n3-16-101", "n3-32-258", "walk-cm-16", "walk-cmb-16", "walk-pq-32", "guard-egcl-39", "guard-egcl-pq-walk"],
    "recompute": _small((16,), (258,)) + _small((32,)) + ["walk-cmp-32"],
    "nopq": _small((32,)) + ["walk-cm-32", "guard-egcl-39", "guard-egcl-cm-walk"],
    "nopq-recompute": _small((32,)) + ["walk-cm-32"],
    "nocmbwd": _small((16, 32)) + ["guard-egcl-39", "guard-egcl-pq-walk", "guard-plain-23"],
    "nopq-nocmbwd": _small((32,), (101,)) + ["guard-egcl-39", "guard-egcl-cm-walk"],
    "det": _small((16, 32)) + ["walk-cm-16", "walk-pq-32"],
    "plain": _plains((1, 23, 12341)) + ["guard-plain-23", "guard-plain-walk"],
    "plain-recompute": _plains((1, 23)),
}
CASES = {f"{base}@{group}": dict(BASES[base], seed_tag=base, group=group) for group, bases in MEMBERS.items() for base in bases}

# A case may enter only if every yardstick of its seed tag - float32 oracle against float64 oracle, float32 twin against
# float64 twin on the walks - is at most YARD: under that cap the bound of every tensor is the floor 1e-5. A condition on the
# inputs (host runs, no kernel involved: tests/test_lane_n3_cpu.py); a seed tag that misses it takes the first seed offset
# 1, 2, .. that meets it. Every seed tag meets it at offset 0, the aggr = sum walks at tens of thousands of edges included:
# worst yardsticks small 8.4e-7 .. 3.6e-6, walks 2.0e-6 (walk-cmp-32) .. 5.1e-6 (walk-cm-16, g.node_model.layers.1.0.weight),
# CEMLPs 7.5e-7 .. 4.3e-6. So the table is empty.
RESEED = {}
YARD = 1e-5


def channels_of(c):
    return c["widths"][2] if "widths" in c else c["C"]


def stages_of(c):
    return (PLAIN_F, PLAIN_B) if "widths" in c else EGCL_STAGES


class Guarded:
    """`n` elements between two runs of sentinels, the interior NaN (float32) or 0xFF bytes (uint8: NaN as floats)."""
    GUARD = 4096    # elements: a multiple of every alignment the workspace tail asks for

    def __init__(self, n, dev, dtype=torch.float32):
        self.n, self.sentinel = n, (-12345.0 if dtype == torch.float32 else 0xA5)
        self.full = torch.full((n + 2 * self.GUARD,), self.sentinel, dtype=dtype, device=dev)
        self.body = self.full[self.GUARD:self.GUARD + n]
        self.body.fill_(float("nan") if dtype == torch.float32 else 0xFF)

    def intact(self):
        return bool((torch.cat([self.full[:self.GUARD], self.full[self.GUARD + self.n:]]) == self.sentinel).all())


class N3Suite(Suite):
    """The child runs the HIP side of a case and stores its tensors; the references are the host's business."""

    out_dir = None

    def child_env(self, group):
        if N3Suite.out_dir is None:
            N3Suite.out_dir = tempfile.mkdtemp(prefix="lane_n3_")
            atexit.register(shutil.rmtree, N3Suite.out_dir, ignore_errors=True)
        env = {k: v for k, v in super().child_env(group).items() if k not in SWITCHES or k in self.groups[group][0]}
        return dict(env, LANE_N3_OUT=N3Suite.out_dir)

    def twin_cemlp(self, tag, inputs, real64):
        from test_full_size_twin import _twin
        c = self.cases[tag]
        x, p, gout = inputs
        y, gx, grads = _twin().cemlp(np.asarray(c["metric"], np.float32), {k: v.numpy() for k, v in p.items()}, x.numpy(),
                                     gy=gout.numpy(), real64=real64)
        return {"y": y, "gx": gx, **{"g." + k: v for k, v in grads.items()}}

    def references(self, tag, inputs):
        c = self.cases[tag]
        if c["kind"] == "cemlp" and c["ref"] == "twin":
            return self.twin_cemlp(tag, inputs, True), self.twin_cemlp(tag, inputs, False)
        return super().references(tag, inputs)

    # ---------------------------------------------------------------------------------------------------- the child
    def stage_labels(self, tag, inputs):
        """The four stages through ops.HipBackend on this thread; a note with csmpn_last_kernel behind each."""
        from csmpn_hip import native, ops
        c = self.cases[tag]
        h, ei, ea, na, p, gout = inputs
        layer = self.egcl_layer(tag, p)
        be, spec, d = ops.HipBackend, layer.spec(), G.dev()
        note = lambda stage: say(G._NOTE + "label %d %d %s" % (stage + (native.lib().csmpn_last_kernel().decode(),)))
        csr = ops.get_csr(ei.to(d), c["N"])
        pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
        hd, ead, nad, gd = h.to(d), ea.to(d), na.to(d), gout.to(d)
        agg, st_e = be.edge_forward(spec, csr, hd, ead, pe)
        note(EDGE_F)
        _out, st_n = be.node_forward(spec, csr.deg, hd, agg, nad, pn)
        note(NODE_F)
        gh, g_agg, _g_na, _ = be.node_backward(spec, csr.deg, hd, agg, nad, pn, gd, True, st_n)
        note(NODE_B)
        be.edge_backward(spec, csr, hd, ead, pe, g_agg, gh, True, st_e)
        note(EDGE_B)
        torch.cuda.synchronize()

    def child_case(self, tag):
        c = self.cases[tag]
        if c["kind"].startswith("guard_"):
            got = hip_guard(tag)
        else:
            inputs = self.cemlp_inputs(tag) if c["kind"] == "cemlp" else self.egcl_inputs(tag)
            run = self.hip_cemlp if c["kind"] == "cemlp" else self.hip_egcl
            got = run(tag, inputs)
            if c["group"] == "det":
                say(G._NOTE + "run 2")
                again = run(tag, inputs)
                differ = [k for k in sorted(got) if not np.array_equal(got[k], again[k])]
                assert not differ, f"not bit-identical between two runs in deterministic mode: {differ}"
            if c["kind"] == "egcl":
                say(G._NOTE + "labels")
                self.stage_labels(tag, inputs)
        np.savez(os.path.join(os.environ["LANE_N3_OUT"], tag + ".npz"), **got)
        return "stored"


# every switch a group sets: a child inherits none of them from the environment of the test process
SWITCHES = sorted({k for env in GROUP_ENV.values() for k in env} | {"CSMPN_NO_CM", "CSMPN_NO_CL", "CSMPN_NO_SLICED_GRADS",
                                                                    "CSMPN_PHASED_MIN_ROWS", "CSMPN_NO_PHASED", "CSMPN_FORCE_H"})
SUITE = N3Suite("lane_n3_helpers", CASES, GROUPS, RESEED)
group_of, group_tags = SUITE.group_of, SUITE.group_tags

GUARD_VARIANTS = ("state", "noflag")    # the entry points called with CSMPN_FLAG_SAVE_STATE, and with flags 0


def guard_group(group, variant):
    """The group whose row of EXPECTED a guard case's variant dispatches by: flags 0 is what CSMPN_SAVE_STATE=0 makes ops.py pass."""
    if variant == "state" or "nocmbwd" in group:
        return group
    return {"default": "recompute", "nopq": "nopq-recompute", "plain": "plain-recompute"}[group]


def hip_guard(tag):
    """Runs in the child. The stage entry points through the C-ABI, forward and backward, on a saved buffer of exactly
    csmpn_cemlp_saved_floats(rows, flags) floats and a workspace of exactly csmpn_cemlp_workspace_bytes bytes, each inside a
    larger tensor: sentinels in front and behind, NaN inside. Once with CSMPN_FLAG_SAVE_STATE and once with flags 0. Stored per
    variant: `<v>.intact.<buffer>`, `<v>.floats.<buffer>`, `<v>.finite.<tensor>`; a label note behind every stage."""
    from csmpn_hip import native, ops
    c = CASES[tag]
    lib, d = native.lib(), G.dev()
    st = ops._stream(d)
    got = {}
    note = lambda stage: say(G._NOTE + "label %d %d %s" % (stage + (lib.csmpn_last_kernel().decode(),)))

    def buffers(v, name, binding, rows, flags):
        n = int(lib.csmpn_cemlp_saved_floats(binding.n, binding.params, binding.nblk, rows, flags))
        saved = Guarded(n, d)
        ws = Guarded(int(lib.csmpn_cemlp_workspace_bytes(binding.n, binding.params, binding.nblk)), d, torch.uint8)
        got[f"{v}.floats.saved_{name}"] = np.asarray(n)
        return saved, ws

    def verdict(v, guards, tensors):
        torch.cuda.synchronize()
        for k, g in guards.items():
            got[f"{v}.intact.{k}"] = np.asarray(g.intact())
        for k, t in tensors.items():
            got[f"{v}.finite.{k}"] = np.asarray(bool(torch.isfinite(t).all()))

    for v in GUARD_VARIANTS:
        say(G._NOTE + v)
        fl = native.FLAG_SAVE_STATE if v == "state" else 0
        if c["kind"] == "guard_cemlp":
            x, p, gout = SUITE.cemlp_inputs(tag)
            m = SUITE.cemlp_module(tag, p)
            b, params = m.binding(), m.flat_params()
            b.bind(params)
            rows = c["rows"]
            saved, ws = buffers(v, "x", b, rows, fl)
            xd, gd = x.to(d), gout.to(d)
            y = torch.full((rows, 32, D), float("nan"), device=d)
            native.check(lib.csmpn_cemlp_forward(b.metric_arr, b.n, b.params, b.nblk, xd.data_ptr(), rows, y.data_ptr(),
                                                 saved.body.data_ptr(), ws.body.data_ptr(), ws.n, fl, st))
            note(PLAIN_F)
            _, views = b.new_grads(params, d)
            gx = torch.full_like(xd, float("nan"))
            native.check(lib.csmpn_cemlp_backward(b.metric_arr, b.n, b.params, b.grads, b.nblk, xd.data_ptr(), gd.data_ptr(), rows,
                                                  gx.data_ptr(), saved.body.data_ptr(), ws.body.data_ptr(), ws.n,
                                                  native.FLAG_WEIGHTS_PACKED | fl, st))
            note(PLAIN_B)
            verdict(v, {"saved_x": saved, "ws_x": ws}, {"y": y, "gx": gx, **{f"g{i}": t for i, t in enumerate(views) if t is not None}})
            continue
        h, ei, ea, na, p, gout = SUITE.egcl_inputs(tag)
        N, E = c["N"], c["E"]
        layer = SUITE.egcl_layer(tag, p)
        spec, csr = layer.spec(), ops.get_csr(ei.to(d), N)
        e, nd = spec.edge, spec.node
        pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
        e.bind(pe)
        nd.bind(pn)
        hh, ead, nad, gd = h.to(d), ea.to(d), na.to(d), gout.to(d)
        saved_e, ws_e = buffers(v, "e", e, E, fl)
        saved_n, ws_n = buffers(v, "n", nd, N, fl)
        agg = torch.zeros(N, 32, D, device=d)
        native.check(lib.csmpn_egcl_edge_forward(
            e.metric_arr, e.n, e.params, e.nblk, hh.data_ptr(), spec.C, ead.data_ptr(), spec.A, csr.perm.data_ptr(), csr.src.data_ptr(),
            csr.dst.data_ptr(), E, N, agg.data_ptr(), saved_e.body.data_ptr(), ws_e.body.data_ptr(), ws_e.n, fl, st))
        note(EDGE_F)
        out = torch.full((N, 32, D), float("nan"), device=d)
        native.check(lib.csmpn_egcl_node_forward(
            nd.metric_arr, nd.n, nd.params, nd.nblk, hh.data_ptr(), spec.C, agg.data_ptr(), spec.O, nad.data_ptr(), spec.T,
            csr.deg.data_ptr(), spec.mean, spec.residual, N, out.data_ptr(), saved_n.body.data_ptr(), ws_n.body.data_ptr(), ws_n.n, fl, st))
        note(NODE_F)
        _, views_n = nd.new_grads(pn, d)
        gh, g_agg, g_na = (torch.full((N, ch, D), float("nan"), device=d) for ch in (32, 32, NA))
        native.check(lib.csmpn_egcl_node_backward(
            nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, hh.data_ptr(), spec.C, agg.data_ptr(), spec.O, nad.data_ptr(), spec.T,
            csr.deg.data_ptr(), spec.mean, spec.residual, N, gd.data_ptr(), gh.data_ptr(), g_agg.data_ptr(), g_na.data_ptr(),
            saved_n.body.data_ptr(), ws_n.body.data_ptr(), ws_n.n, native.FLAG_WEIGHTS_PACKED | fl, st))
        note(NODE_B)
        _, views_e = e.new_grads(pe, d)
        g_ea = torch.full((E, EA, D), float("nan"), device=d)
        native.check(lib.csmpn_egcl_edge_backward(
            e.metric_arr, e.n, e.params, e.grads, e.nblk, hh.data_ptr(), spec.C, ead.data_ptr(), spec.A, csr.perm.data_ptr(),
            csr.src.data_ptr(), csr.dst.data_ptr(), E, N, g_agg.data_ptr(), gh.data_ptr(), g_ea.data_ptr(), saved_e.body.data_ptr(),
            ws_e.body.data_ptr(), ws_e.n, native.FLAG_WEIGHTS_PACKED | fl, st))
        note(EDGE_B)
        tensors = {"agg": agg, "y": out, "gh": gh, "g_agg": g_agg, "g_na": g_na, "g_ea": g_ea}
        tensors.update({f"ge{i}": t for i, t in enumerate(views_e) if t is not None})
        tensors.update({f"gn{i}": t for i, t in enumerate(views_n) if t is not None})
        verdict(v, {"saved_e": saved_e, "ws_e": ws_e, "saved_n": saved_n, "ws_n": ws_n}, tensors)
    return got


# ------------------------------------------------------------------------------------------------------------ the host
_refs = {}


def yardsticks(tag):
    """{tensor: error of the float32 reference run against the float64 one} of the case's seed tag, and both runs; computed
    once per seed tag."""
    c = CASES[tag]
    base = c["seed_tag"]
    if base not in _refs:
        inputs = SUITE.cemlp_inputs(tag) if c["kind"] == "cemlp" else SUITE.egcl_inputs(tag)
        t64, t32 = SUITE.references(tag, inputs)
        _refs[base] = (t64, t32, {k: relmax(t32[k], t64[k]) for k in t64})
    return _refs[base]


def reference(tag):
    """(float64 truth, float32 yardstick run) of the case's seed tag; asserts the cap on the yardsticks - a property of the
    references alone - before anything looks at a HIP result."""
    t64, t32, yard = yardsticks(tag)
    worst = max(yard, key=yard.get)
    assert yard[worst] <= YARD, f"{CASES[tag]['seed_tag']}: yardstick of {worst} is {yard[worst]:.3e} > {YARD:.0e}"
    return t64, t32


def result(tag):
    """The case's entry of its group's child (general_helpers.Suite.run_group) with `got`: the tensors the child stored."""
    r = SUITE.run_group(group_of(tag))[tag]
    if "got" not in r and r["ok"]:
        with np.load(os.path.join(N3Suite.out_dir, tag + ".npz")) as z:
            r["got"] = {k: z[k] for k in z.files}
    return r


FAMILY = re.compile(r"\[csmpn\] (?P<family>pq|pg|plw|pl|cl|cm|wide) mode=(?P<mode>\d) bwd=(?P<bwd>\d) "
                    r"channels=(?P<channels>\d+) (?:attr=(?P<attr>\d+)|i0=(?P<i0>\d+)) grid=(?P<grid>\d+) rows=(?P<rows>\d+)$")
_LABEL = "label "


def launches(r):
    """[(note, [launch], {stage: label})]: the launch lines of a case's log split at the child's notes ('' in front of the
    first); a general-kernel line is a launch of family `general`. Any other `[csmpn]` line fails."""
    out = [("", [], {})]
    for line in r["log"]:
        if line.startswith(G._NOTE):
            text = line[len(G._NOTE):].strip()
            if text.startswith(_LABEL):
                mode, bwd, label = text[len(_LABEL):].split(" ", 2)
                out[-1][2][(int(mode), int(bwd))] = label
            else:
                out.append((text, [], {}))
            continue
        m = FAMILY.match(line)
        if m:
            out[-1][1].append({k: (v if k == "family" else int(v)) for k, v in m.groupdict().items() if v is not None})
            continue
        m = G.GENERAL.search(line)
        assert m, f"neither a lane-family nor a general-kernel line: {line}"
        out[-1][1].append(dict({k: int(v) for k, v in m.groupdict().items()}, family=GENERAL))
    return [x for x in out if x[0] or x[1]]


def expected(tag, group=None):
    """{stage: family} of the case's own stages under its group (or `group`)."""
    c = CASES[tag]
    row = EXPECTED[group or c["group"]][channels_of(c)]
    return {s: row[s] for s in stages_of(c)}


def stage_rows(tag):
    c = CASES[tag]
    return lambda stage: c["rows"] if "widths" in c else (c["E"] if stage[0] == 1 else c["N"])


def check_dispatch(tag, ls, group=None):
    """One run's launches against EXPECTED: exactly the stages of the case, each once, on the expected family, with the case's
    channels, block-0 input or attribute channels, and rows."""
    c = CASES[tag]
    channels, rows_of = channels_of(c), stage_rows(tag)
    want = expected(tag, group)
    assert sorted((l["mode"], l["bwd"]) for l in ls) == sorted(want), (tag, ls)
    for l in ls:
        stage = (l["mode"], l["bwd"])
        assert l["family"] == want[stage], f"{tag}: stage {stage} ran on {l['family']}, expected {want[stage]}: {l}"
        assert l["rows"] == rows_of(stage), (tag, l)
        if l["family"] == "pq":     # channels, attribute channels (MODE_PLAIN: input channels)
            assert (l["channels"], l["attr"]) == (32, {0: c["widths"][0] if "widths" in c else None, 1: EA, 2: NA}[l["mode"]]), (tag, l)
        elif l["family"] == "cm":   # channels, block 0's input channels
            assert (l["channels"], l["i0"]) == (channels, channels + EA if l["mode"] == 1 else 2 * channels + NA), (tag, l)


def check_labels(tag, labels, group=None, state=None):
    c = CASES[tag]
    assert sorted(labels) == sorted(stages_of(c)), (tag, labels)
    for stage, label in labels.items():
        for part in expected_label(group or c["group"], channels_of(c), stage, state):
            assert part in label, f"{tag}: stage {stage} names {label!r}, expected {part!r} in it"


def check_walks(tag, ls, walks):
    """From the log: a launch in `walks` has more rows than its grid holds in one iteration of its workgroups (some take a
    second tile; the last tile is partial), every other lane launch has not - so a changed cap fails here instead of quietly
    making a one-sweep case."""
    channels = channels_of(CASES[tag])
    for l in ls:
        stage = (l["mode"], l["bwd"])
        if l["family"] == GENERAL:
            assert stage not in walks, (tag, l)
            continue
        held = l["grid"] * rows_per_iteration(l["family"], channels, l["bwd"])
        if stage in walks:
            assert l["grid"] == grid_cap(l["family"], channels, l["bwd"]) and l["rows"] > held and l["rows"] % TILE != 0, \
                f"{tag}: does not walk: {l}"
        else:
            assert l["rows"] <= held, f"{tag}: walks unexpectedly: {l}"
