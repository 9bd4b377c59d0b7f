"""Suite: inputs, references, comparison, child-process driver and dispatch-log reader over one table of cases and one of
groups (tests/lane_d32_helpers.py passes its own), and the cases of tests/test_general_kernels_gpu.py: the general row-tile
kernels (cemlp_kernel.hpp, cemlp_ps.hpp; planned by make_plan in csrc/plan.hip, launched at the bottom of run_rows in
csrc/dispatch.hip) against the float64 oracle (oracle/ref_path.py) and, where a workgroup walks many row tiles, against the
float64 C++ twin (oracle/cpu_twin).

The environment switches of the library are read once per process and autograd's backward runs on another thread, so a
case that has to prove which configuration it ran is run in a CHILD process with CSMPN_DEBUG=1: `run_group` starts one
child per group (one environment, several cases), the child compares every case itself (`run_case`) and writes a marker
line to stderr in front of and behind each case; the library's own `[csmpn] ...` lines in between are that case's launches.
"""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import torch

from oracle import ref_path as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "clifford-group-equivariant-simplicial-message-passing-networks_amd"
TOL = 1e-5

CL20, CL30, CL40, CL31 = (1.0, 1.0), (1.0, 1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (1.0, 1.0, 1.0, -1.0)
CL50, CL41 = (1.0,) * 5, (1.0, 1.0, 1.0, 1.0, -1.0)
ALG_NAMES = {CL20: "cl20", CL30: "cl30", CL40: "cl40", CL31: "cl31", CL50: "cl50", CL41: "cl41"}
NEG_SCALE = 0.02    # blades that hold a negative generator, on the indefinite metrics (as test_egcl_cl41_well_conditioned)


def relmax(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def check(name, hip, truth, ref32, slack):
    """`check` of tests/test_hip_parity.py (restated): per tensor max(1e-5, slack x the float32 reference's own error against
    float64), and every element within 10 x that bound of |truth| + 0.1 max|truth|."""
    err = relmax(hip, truth)
    bound = max(TOL, slack * relmax(ref32, truth))
    assert err <= bound, f"{name}: rel err {err:.3e} > {bound:.3e}"
    a, b = np.asarray(hip, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    worst = float((np.abs(a - b) / (np.abs(b) + 0.1 * scale)).max())
    assert worst <= 10 * bound, f"{name}: element-wise rel err {worst:.3e} > {10 * bound:.3e}"
    return err


def slack_of(metric):
    return 4.0 if min(metric) > 0 else 10.0


# ------------------------------------------------------------------------------------------------------------ the cases
def _egcl(metric, C, N, E, aggr="mean", residual=True, attrs=True, hidden=None, rewire=False, ref="oracle"):
    return dict(kind="egcl", metric=metric, C=C, hidden=hidden or C, N=N, E=E, aggr=aggr, residual=residual, attrs=attrs,
                rewire=rewire, ref=ref)


def _cemlp(metric, nl, widths, rows):
    return dict(kind="cemlp", metric=metric, nl=nl, widths=widths, rows=rows)


NARROW, MID = (20, 12, 12), (70, 48, 48)   # (in, hidden, out) of the standalone CEMLPs
CASES = {
    # ---- Cl(4,0) / Cl(3,1): 5, 8, 12, 20, 33, 48, 64 channels; mean / sum, residual on / off, with / without attributes,
    # ragged edge counts, isolated nodes + duplicate edges (rewire), hidden != out
    "egcl-cl40-5": _egcl(CL40, 5, 10, 24),
    "egcl-cl40-8": _egcl(CL40, 8, 23, 37, aggr="sum", residual=False),
    "egcl-cl40-12": _egcl(CL40, 12, 40, 101, attrs=False, rewire=True),
    "egcl-cl40-20": _egcl(CL40, 20, 17, 150, aggr="sum", hidden=12),
    "egcl-cl40-33": _egcl(CL40, 33, 30, 101, residual=False, rewire=True),
    "egcl-cl40-48": _egcl(CL40, 48, 24, 80, aggr="sum"),
    "egcl-cl40-64": _egcl(CL40, 64, 16, 37, attrs=False),
    "egcl-cl31-5": _egcl(CL31, 5, 23, 37, aggr="sum", rewire=True),
    "egcl-cl31-8": _egcl(CL31, 8, 10, 24, attrs=False),
    "egcl-cl31-12": _egcl(CL31, 12, 17, 101, aggr="sum", residual=False, hidden=20),
    "egcl-cl31-20": _egcl(CL31, 20, 40, 150, rewire=True),
    "egcl-cl31-33": _egcl(CL31, 33, 24, 80, aggr="sum", attrs=False),
    "egcl-cl31-48": _egcl(CL31, 48, 16, 37, residual=False),
    "egcl-cl31-64": _egcl(CL31, 64, 30, 101, aggr="sum"),
    # ---- Cl(5,0) / Cl(4,1) outside the lane widths: 12, 20, 40, 48, 64 channels (and 5: the parity-split kernels); the dense
    # oracle costs rows x channels x 32^3 per product, so from 40 channels on: 10 nodes (less than a tile), 24 edges (16 + 8)
    "egcl-cl50-5": _egcl(CL50, 5, 10, 24, aggr="sum"),
    "egcl-cl50-12": _egcl(CL50, 12, 12, 37, rewire=True),
    "egcl-cl50-20": _egcl(CL50, 20, 10, 24, aggr="sum", residual=False, hidden=12),
    "egcl-cl50-40": _egcl(CL50, 40, 10, 24, attrs=False),
    "egcl-cl50-48": _egcl(CL50, 48, 10, 24, aggr="sum"),
    "egcl-cl50-64": _egcl(CL50, 64, 10, 24, residual=False),
    "egcl-cl41-12": _egcl(CL41, 12, 10, 24, aggr="sum", attrs=False),
    "egcl-cl41-20": _egcl(CL41, 20, 17, 37, residual=False, rewire=True),
    "egcl-cl41-40": _egcl(CL41, 40, 10, 24, aggr="sum", hidden=24),
    "egcl-cl41-48": _egcl(CL41, 48, 10, 24),
    "egcl-cl41-64": _egcl(CL41, 64, 10, 24, aggr="sum"),
    # ---- lane widths with their families switched off
    "nolane-cl50-28": _egcl(CL50, 28, 12, 37),
    "nolane-cl41-16": _egcl(CL41, 16, 17, 37, aggr="sum", rewire=True),
    "nolane-cl30-8": _egcl(CL30, 8, 37, 101, residual=False),
    # ---- standalone CEMLPs of 1..4 blocks: 20 -> 12 -> 12 and 70 -> 48 -> 48; 1, 17, 100 rows
    "cemlp-cl30-1": _cemlp(CL30, 1, NARROW, 1),
    "cemlp-cl30-2": _cemlp(CL30, 2, MID, 17),
    "cemlp-cl30-3": _cemlp(CL30, 3, NARROW, 100),
    "cemlp-cl30-4": _cemlp(CL30, 4, MID, 100),
    "cemlp-cl40-1": _cemlp(CL40, 1, MID, 17),
    "cemlp-cl40-2": _cemlp(CL40, 2, NARROW, 100),
    "cemlp-cl40-3": _cemlp(CL40, 3, MID, 1),
    "cemlp-cl40-4": _cemlp(CL40, 4, NARROW, 17),
    "cemlp-cl41-1": _cemlp(CL41, 1, NARROW, 17),
    "cemlp-cl41-2": _cemlp(CL41, 2, MID, 1),
    "cemlp-cl41-3": _cemlp(CL41, 3, NARROW, 100),
    "cemlp-cl41-4": _cemlp(CL41, 4, MID, 17),
    # z aliasing the input tile (the widths of test_cemlp_shared_input_buffer, fewer rows)
    "cemlp-cl30-share": _cemlp(CL30, 2, (40, 16, 16), 100),
    # ---- 32-row tiles (CSMPN_FORCE_H=2): 37 nodes = 2 tiles, 101 edges = 4 tiles, both ragged
    "h2-cl30-5": _egcl(CL30, 5, 37, 101),
    "h2-cl20-7": _egcl(CL20, 7, 37, 101, aggr="sum", attrs=False, rewire=True),
    # ---- the block-by-block backward (CSMPN_PHASED_MIN_ROWS lowered to 64 rows)
    "phased-cemlp-cl30-3": _cemlp(CL30, 3, (10, 32, 32), 300),
    "phased-cemlp-cl30-4": _cemlp(CL30, 4, MID, 300),
    "phased-egcl-cl20-40": _egcl(CL20, 40, 130, 333, aggr="sum"),
    # ---- a workgroup walks several row tiles; float64 twin. Cl(2,0), 40 channels: at most 2 workgroups x 256 per CU class
    # and 2 tiles per workgroup = 16 384 rows per sweep; global scratch: 256 workgroups x 1 tile = 4 096 rows per sweep
    "walk-cl20-40": _egcl(CL20, 40, 16391, 16397, ref="twin"),
    "walk-cl50-40": _egcl(CL50, 40, 4100, 4110, aggr="sum", ref="twin"),
}

_NOLANES = {"CSMPN_NO_PG": "1", "CSMPN_NO_PLW": "1", "CSMPN_NO_PL": "1", "CSMPN_NO_CL": "1"}
#  group: (environment beside CSMPN_DEBUG=1, predicate on the tag)
GROUPS = {
    "n4": ({}, lambda t: t.startswith(("egcl-cl40", "egcl-cl31"))),
    "n5": ({}, lambda t: t.startswith(("egcl-cl50", "egcl-cl41"))),
    "cemlp": ({}, lambda t: t.startswith("cemlp-")),
    "nolanes": (_NOLANES, lambda t: t.startswith("nolane-")),
    "h2": ({"CSMPN_FORCE_H": "2"}, lambda t: t.startswith("h2-")),
    "phased": ({"CSMPN_PHASED_MIN_ROWS": "64"}, lambda t: t.startswith("phased-")),
    "walk": ({}, lambda t: t.startswith("walk-")),
}


# ------------------------------------------------------------------------------------------------- inputs and references
# An indefinite metric makes the layer itself ill-conditioned where a quadratic form comes close to zero (d/dq of
# (q^2 + 1e-16)^(1/4) blows up), also on the tamed inputs: then ANY float32 evaluation is far from float64, the error of one
# such evaluation (the yardstick) says little about the next, and the bound would measure the luck of a rounding, not a kernel.
# So the inputs of an indefinite EGCL case must pass `well_conditioned` - a criterion of the references alone: the float32
# C++ twin, which sums in another order than the float32 oracle, is itself within the bound the kernels are held to. The
# seed of the tag is used where it passes; where it does not, the first seed offset 1, 2, .. that passes stands here with
# the figures of the seed that did not (host run, no kernel involved):
#   egcl-cl31-48, offset 0: the float32 oracle is up to 9.8e-5 off float64 (the other cases: ~2e-6), the float32 twin misses
#   the bound on 19 of 44 tensors, worst g.edge_model.layers.0.2.linear_left.bias: twin 2.3e-5, oracle 1.2e-6, bound 1.2e-5
#   (the general HIP kernels gave 1.6e-5 on that tensor there).
RESEED = {"egcl-cl31-48": 1}


def _tame(o32, metric, t):
    """Keep an indefinite metric off its null cone: scale the blades that hold a negative generator."""
    if min(metric) > 0:
        return t
    neg_bits = sum(1 << i for i, m in enumerate(metric) if m < 0)
    mask = torch.from_numpy(((np.asarray(o32.t.index_to_bitmap) & neg_bits) != 0).astype(np.float32))
    return t * (1.0 - mask + NEG_SCALE * mask)


def _rewire(ei, N):
    """Exact duplicates, a self loop and two nodes (the last two) without any edge."""
    ei = ei.clone()
    ei[:, -5:] = ei[:, :5]
    ei[0, 7] = ei[1, 7]
    ei[ei >= N - 2] = 1
    return ei


def _pkg():
    return importlib.import_module(PKG)


def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


def _load(module, p):
    sd = module.state_dict()
    sd.update(p)
    module.load_state_dict(sd, strict=True)
    return module.to(dev())


_BEGIN, _OK, _FAIL, _NOTE = "[case] begin ", "[case] ok ", "[case] FAIL ", "[case] note "
_CHILD = r"""
import importlib, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
importlib.import_module(sys.argv[3]).SUITE.child_main(sys.argv[2])
"""
GENERAL = re.compile(r"\[csmpn\] mode=(?P<mode>\d) bwd=(?P<bwd>\d) var=(?P<var>\d) ps=(?P<ps>\d) share=(?P<share>\d) "
                     r"phased=(?P<phased>\d) H=(?P<H>\d) MT=(?P<MT>\d) RT=(?P<RT>\d) threads=(?P<threads>\d+) lds=(?P<lds>\d+) "
                     r"grid=(?P<grid>\d+) tile_floats=(?P<tile_floats>\d+) mirror=(?P<mirror>\d+) rows=(?P<rows>\d+)")
OTHER = re.compile(r"\[csmpn\] (pq|pg|plw|pl|cl|cm|wide) mode=")
_ended_badly = []    # groups whose child did not end cleanly: nothing more is started on the GPU after that (any suite)


def say(s):
    """A line on the (unbuffered) stderr the library logs to."""
    os.write(2, (s + "\n").encode())


class Suite:
    """One table of cases and one table of groups - group: (environment beside CSMPN_DEBUG=1, predicate on the tag) - with
    the inputs, the references, the comparison and the child-process driver that read them. `module` is the name of the
    module that holds the instance as SUITE: the child imports it. `reseed`: seed offsets per seed tag (see RESEED); a case
    may name the tag its seed follows (`seed_tag`: the same inputs under several tags), else its own tag is that."""

    def __init__(self, module, cases, groups, reseed):
        self.module, self.cases, self.groups, self.reseed = module, cases, groups, reseed
        self._results = {}

    def group_of(self, tag):
        found = [g for g, (_, pred) in self.groups.items() if pred(tag)]
        assert len(found) == 1, (tag, found)
        return found[0]

    def group_tags(self, group):
        return [t for t in self.cases if self.groups[group][1](t)]

    def seed(self, tag):
        st = self.cases[tag].get("seed_tag", tag)
        return 2000 + sum((i + 1) * ord(c) for i, c in enumerate(st)) + self.reseed.get(st, 0)

    def egcl_inputs(self, tag):
        c = self.cases[tag]
        metric, N, E, C = c["metric"], c["N"], c["E"], c["C"]
        o32 = O.Algebra(list(metric), torch.float32)
        h, ei, ea, na = O.synthetic_complex(o32, N, E, C, seed=self.seed(tag))
        if c["rewire"]:
            ei = _rewire(ei, N)
            ea = torch.cat([na[ei[0]], na[ei[1]]], dim=1)    # the edge attributes follow the rewired ends
        h = _tame(o32, metric, h)
        if not c["attrs"]:
            ea = na = None
        gen = torch.Generator().manual_seed(self.seed(tag) + 1)
        p = O.init_egcl_params(o32, C, c["hidden"], C, 6 if c["attrs"] else 0, 3 if c["attrs"] else 0, gen=gen, randomize=True)
        gout = torch.randn(N, C, 1 << len(metric), generator=gen)
        return h, ei, ea, na, p, gout

    def cemlp_inputs(self, tag):
        c = self.cases[tag]
        metric, (in_f, hid, out_f) = c["metric"], c["widths"]
        o32 = O.Algebra(list(metric), torch.float32)
        gen = torch.Generator().manual_seed(self.seed(tag))
        p = O.init_cemlp_params(o32, in_f, hid, out_f, n_layers=c["nl"], gen=gen, randomize=True)
        x = _tame(o32, metric, torch.randn(c["rows"], in_f, o32.D, generator=gen))
        gout = torch.randn(c["rows"], out_f, o32.D, generator=gen)
        return x, p, gout

    def egcl_layer(self, tag, p):
        """The case's layer on the device, with the parameters p."""
        c = self.cases[tag]
        pkg = _pkg()
        return _load(pkg.EGCL(pkg.CliffordAlgebra(tuple(c["metric"])), c["C"], c["hidden"], c["C"],
                              edge_attr_features=6 if c["attrs"] else 0, node_attr_features=3 if c["attrs"] else 0,
                              residual=c["residual"], aggr=c["aggr"]), p)

    def hip_egcl(self, tag, inputs):
        """The layer through autograd: y, gh, g_edge_attr / g_node_attr (with attributes) and g.<parameter>."""
        c = self.cases[tag]
        h, ei, ea, na, p, gout = inputs
        layer = self.egcl_layer(tag, p)
        hd = h.to(dev()).requires_grad_(True)
        args = (ea.to(dev()).requires_grad_(True), na.to(dev()).requires_grad_(True)) if c["attrs"] else ()
        y = layer(hd, ei.to(dev()), *args)
        (y * gout.to(dev())).sum().backward()
        torch.cuda.synchronize()
        got = {"y": y.detach().cpu().numpy(), "gh": hd.grad.cpu().numpy()}
        if c["attrs"]:
            got["g_edge_attr"], got["g_node_attr"] = args[0].grad.cpu().numpy(), args[1].grad.cpu().numpy()
        got.update({"g." + k: v.grad.cpu().numpy() for k, v in layer.named_parameters()})
        return got

    def oracle_egcl(self, tag, inputs, dtype):
        c = self.cases[tag]
        h, ei, ea, na, p, gout = inputs
        leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)    # never the caller's tensor
        q = {k: leaf(v) for k, v in p.items()}
        hh = leaf(h)
        ee, nn = (leaf(ea), leaf(na)) if c["attrs"] else (None, None)
        y = O.egcl(O.Algebra(list(c["metric"]), dtype), hh, ei, ee, nn, q, aggr=c["aggr"], residual=c["residual"])
        (y * gout.to(dtype)).sum().backward()
        out = {"y": y.detach().numpy(), "gh": hh.grad.numpy()}
        if c["attrs"]:
            out["g_edge_attr"], out["g_node_attr"] = ee.grad.numpy(), nn.grad.numpy()
        out.update({"g." + k: v.grad.numpy() for k, v in q.items()})
        return out

    def twin_egcl(self, tag, inputs, real64):
        from test_full_size_twin import _twin
        c = self.cases[tag]
        h, ei, ea, na, p, gout = inputs
        npy = lambda t: None if t is None else t.numpy()
        r = _twin().egcl_layer(np.asarray(c["metric"], np.float32), {k: v.numpy() for k, v in p.items()}, h.numpy(), ei.numpy(),
                               npy(ea), npy(na), aggr=c["aggr"], residual=c["residual"], gout=gout.numpy(),
                               want_attr_grads=c["attrs"], real64=real64)
        out = {"y": r["out"], "gh": r["gh"]}
        if c["attrs"]:
            out["g_edge_attr"], out["g_node_attr"] = r["g_edge_attr"], r["g_node_attr"]
        out.update({"g." + k: v for k, v in r["grads"].items()})
        return out

    def cemlp_module(self, tag, p):
        c = self.cases[tag]
        pkg = _pkg()
        in_f, hid, out_f = c["widths"]
        return _load(pkg.CEMLP(pkg.CliffordAlgebra(tuple(c["metric"])), in_f, hid, out_f, n_layers=c["nl"]), p)

    def hip_cemlp(self, tag, inputs):
        x, p, gout = inputs
        m = self.cemlp_module(tag, p)
        xd = x.to(dev()).requires_grad_(True)
        y = m(xd)
        (y * gout.to(dev())).sum().backward()
        torch.cuda.synchronize()
        got = {"y": y.detach().cpu().numpy(), "gx": xd.grad.cpu().numpy()}
        got.update({"g." + k: v.grad.cpu().numpy() for k, v in m.named_parameters()})
        return got

    def oracle_cemlp(self, tag, inputs, dtype):
        c = self.cases[tag]
        x, p, gout = inputs
        q = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in p.items()}
        xx = x.detach().to(dtype).clone().requires_grad_(True)
        y = O.cemlp(O.Algebra(list(c["metric"]), dtype), xx, q)
        (y * gout.to(dtype)).sum().backward()
        out = {"y": y.detach().numpy(), "gx": xx.grad.numpy()}
        out.update({"g." + k: v.grad.numpy() for k, v in q.items()})
        return out

    def well_conditioned(self, tag, inputs, t64, t32):
        """The float32 twin of an indefinite EGCL case is within the bound of every tensor (see RESEED)."""
        slack = slack_of(self.cases[tag]["metric"])
        w32 = self.twin_egcl(tag, inputs, False)
        for k in sorted(t64):
            err, bound = relmax(w32[k].reshape(t64[k].shape), t64[k]), max(TOL, slack * relmax(t32[k], t64[k]))
            assert err <= bound, f"{tag}: inputs not well conditioned: {k}: float32 twin {err:.3e} > {bound:.3e}"

    def references(self, tag, inputs):
        """(float64 truth, float32 yardstick run) of one case, host only; an indefinite EGCL case held to the oracle must be
        well conditioned."""
        c = self.cases[tag]
        if c["kind"] == "cemlp":
            return self.oracle_cemlp(tag, inputs, torch.float64), self.oracle_cemlp(tag, inputs, torch.float32)
        if c["ref"] == "twin":
            return self.twin_egcl(tag, inputs, True), self.twin_egcl(tag, inputs, False)
        t64, t32 = self.oracle_egcl(tag, inputs, torch.float64), self.oracle_egcl(tag, inputs, torch.float32)
        if min(c["metric"]) < 0:
            self.well_conditioned(tag, inputs, t64, t32)
        return t64, t32

    def compute(self, tag):
        """(HIP result, float64 truth, float32 yardstick run) of one case; dicts with the same keys."""
        c = self.cases[tag]
        inputs = self.cemlp_inputs(tag) if c["kind"] == "cemlp" else self.egcl_inputs(tag)
        got = self.hip_cemlp(tag, inputs) if c["kind"] == "cemlp" else self.hip_egcl(tag, inputs)
        return (got,) + self.references(tag, inputs)

    def compare(self, tag, got, t64, t32):
        """Every tensor of the case - output, d/d input, d/d attributes, every parameter gradient - against the truth."""
        c = self.cases[tag]
        slack = slack_of(c["metric"])
        assert set(got) == set(t64) == set(t32), (sorted(got), sorted(t64))
        assert len([k for k in got if k.startswith("g.")]) == 10 * (c["nl"] if c["kind"] == "cemlp" else 4)
        errs = {}
        for k in sorted(got):
            errs[k] = (check(f"{tag} {k}", got[k].reshape(t64[k].shape), t64[k], t32[k], slack), relmax(t32[k], t64[k]))
        worst = max(errs, key=lambda k: errs[k][0] / max(TOL, slack * errs[k][1]))
        return f"worst tensor {worst}: HIP err {errs[worst][0]:.2e}, float32 yardstick {errs[worst][1]:.2e}"

    def run_case(self, tag):
        return self.compare(tag, *self.compute(tag))

    # -------------------------------------------------------------------------------------------------------- the child
    def child_case(self, tag):
        """What the child does with one case; returns the text behind its ok marker. An AssertionError marks it failed."""
        return self.run_case(tag)

    def child_main(self, group):
        """Runs in the child: every case of the group; markers on the stderr the library logs to. A failed comparison is
        recorded and the next case runs; any other error (a HIP error among them) ends the child."""
        for tag in self.group_tags(group):
            say(_BEGIN + tag)
            try:
                say(_OK + tag + " " + self.child_case(tag))
            except AssertionError as e:
                say(_FAIL + tag + " " + str(e).replace("\n", " ")[:400])

    def child_env(self, group):
        return dict(os.environ, CSMPN_DEBUG="1", CSMPN_QUIET="1", **self.groups[group][0])

    def run_group(self, group):
        """{tag: dict(ok, message, launches = [dict of ints per general-kernel line], other = [family / wide lines], log)} of
        one group, from one child process (started once per session). log: the case's `[csmpn]` lines and the `[case] note`
        lines the child put between them, in order."""
        if group in self._results:
            return self._results[group]
        assert not _ended_badly, f"not started: the child of group {_ended_badly[0]} did not end cleanly"
        r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, group, self.module], env=self.child_env(group), capture_output=True,
                           text=True, timeout=900, cwd=ROOT)
        if r.returncode != 0:
            _ended_badly.append(group)
        assert r.returncode == 0, f"child of group {group} ended with {r.returncode}:\n{r.stderr[-4000:]}"
        out, cur = {}, None
        for line in r.stderr.splitlines():
            if line.startswith(_BEGIN):
                cur = line[len(_BEGIN):].strip()
                out[cur] = dict(ok=None, message="", launches=[], other=[], log=[])
            elif line.startswith((_OK, _FAIL)):
                ok = line.startswith(_OK)
                tag, _, msg = line[len(_OK if ok else _FAIL):].partition(" ")
                assert tag == cur, (tag, cur)
                out[tag]["ok"], out[tag]["message"] = ok, msg
                cur = None
            elif cur is not None and line.startswith(_NOTE):
                out[cur]["log"].append(line)
            elif cur is not None and line.startswith("[csmpn]"):
                out[cur]["log"].append(line)
                m = GENERAL.search(line)
                if m:
                    out[cur]["launches"].append({k: int(v) for k, v in m.groupdict().items()})
                elif OTHER.search(line):
                    out[cur]["other"].append(line)
        assert list(out) == self.group_tags(group) and all(v["ok"] is not None for v in out.values()), r.stderr[-4000:]
        self._results[group] = out
        return out


# the general-kernel cases: what tests/test_general_kernels_gpu.py imports
SUITE = Suite("general_helpers", CASES, GROUPS, RESEED)
group_of, group_tags, run_group = SUITE.group_of, SUITE.group_tags, SUITE.run_group
compute, compare, run_case = SUITE.compute, SUITE.compare, SUITE.run_case
