"""Cases, inputs, float64 reference and child-process side of tests/test_embed_kernels_gpu.py and
tests/test_embed_reference_cpu.py: the fused simplex embedding (csmpn_embed_cemlp_forward / _backward; MODE_PLAIN of
csrc/cemlp_plw.hpp with io.emb_nperm > 0 - its own gather, its group-strided forward schedule, its register sum over the
vertex orders, its one-row-per-simplex store, and a backward that reads d/d(out) at row / emb_nperm).

Built on tests/general_helpers.py (Suite: the seed formula, `_tame`, `check` / `relmax`, the child process with its `[case]`
markers and the reader of the `[csmpn]` lines). As in tests/lane_d32_helpers.py the child of a group runs the HIP side of
its cases only and stores every tensor (one .npz per case); the references are computed on the host by the test process,
once per seed tag, and the comparison happens there.

Reference of one case (`reference_run`): x = feat[verts].reshape(rows, nv * kpv, D); y = O.cemlp(alg, x, params);
out = y.reshape(nsimp, n_orders, O, D).sum(1); loss = (out * gout).sum(); gradients of every parameter (the features are
data). Evaluated in chunks of whole simplices of about 1000 rows - the oracle's dense [rows, C, D, D] intermediates would
take gigabytes at the walk sizes -, the parameter gradients add up across the chunks.

Tags: `<seed tag>@<group>`; the seed follows from the seed tag, so one shape has the same inputs and reference in every group.
"""
import atexit
import os
import shutil
import tempfile

import numpy as np
import torch

import general_helpers as G
from general_helpers import CL30, CL41, CL50, Suite, relmax, say
from lane_d32_helpers import launches    # the reader of the `[csmpn] <family> ..` lines

O = G.O
S_ROWS, POISON_ROWS, POISON = 97, 8, 3.0e4    # feature rows; the last 8 are never referenced and hold a large finite value
OUT, D = 28, 32
TILE = 4                                      # rows of one plw tile (kPlRows)
FWD_CAP, BWD_CAP = 512, 256                   # plw_grid at 28 channels (csrc/dispatch.hip): 2 x kPlwMaxGroups / kPlwMaxGroups
YARD, SLACK = 1e-5, 4.0                       # cap on every float32 yardstick; bound max(1e-5, 4 x yardstick)
SAME_ID = 41                                  # the id of the simplex whose vertices are all the same
ALGS = {"cl50": CL50, "cl41": CL41}


def group_tiles(n_orders):
    """GT of cemlp_plw.hpp: tiles of one forward group (GT x 4 rows = lcm(4, n_orders))."""
    return 3 if n_orders == 6 else 1


def geometry(c):
    """rows, tiles and forward groups of a case."""
    rows = c["nsimp"] * c["n_orders"]
    tiles = (rows + TILE - 1) // TILE
    gt = group_tiles(c["n_orders"])
    return dict(rows=rows, tiles=tiles, groups=(tiles + gt - 1) // gt)


# --------------------------------------------------------------------------------------------------------- the cases
def _case(metric, nl, nv, kpv, n_orders, nsimp, kind="embed", walk=False, out=OUT, poison=True, **more):
    return dict(kind=kind, metric=metric, nl=nl, in_f=nv * kpv, nv=nv, kpv=kpv, n_orders=n_orders, nsimp=nsimp, walk=walk,
                out=out, poison=poison, **more)


SMALL = (1, 2, 3, 5, 23)
BASES = {}    # seed tag -> case
for _an, _m in ALGS.items():
    for _ns in SMALL:
        BASES[f"edges-{_an}-{_ns}"] = _case(_m, 1, 2, 1, 2, _ns)    # 2 -> 28, one block
        BASES[f"tris-{_an}-{_ns}"] = _case(_m, 2, 3, 1, 6, _ns)     # 3 -> 28 -> 28
    # what the C-ABI admits and the model never makes
    BASES[f"abi-{_an}-o1-v1k2"] = _case(_m, 1, 1, 2, 1, 7)
    BASES[f"abi-{_an}-o2-v1k3"] = _case(_m, 2, 1, 3, 2, 7)
    BASES[f"abi-{_an}-o6-v2k1"] = _case(_m, 1, 2, 1, 6, 7)
    BASES[f"abi-{_an}-o1-v3k1"] = _case(_m, 2, 3, 1, 1, 7)
BASES["walk-edges-cl50-1031"] = _case(CL50, 1, 2, 1, 2, 1031, walk=True)
BASES["walk-tris-cl50-1031"] = _case(CL50, 2, 3, 1, 6, 1031, walk=True)

GUARD_BASES = ("edges-cl50-23", "tris-cl50-23", "walk-tris-cl50-1031")
GUARD_VARIANTS = ("state", "noflag")    # the entry points called with CSMPN_FLAG_SAVE_STATE, and with flags 0
# clamp and validation: a table that holds -1 and S (no poisoned rows: the clamp lands on row S - 1)
CLAMP_BASES = {"clamp-edges-cl50-23": _case(CL50, 1, 2, 1, 2, 23, kind="clamp", poison=False),
               "clamp-tris-cl41-23": _case(CL41, 2, 3, 1, 6, 23, kind="clamp", poison=False)}
REFUSALS = ("rows-not-multiple", "three-orders", "width-mismatch", "no-vertex-rows", "nine-inputs", "cl30", "no-saved-inputs")
# predicate against library: (in_features, blocks) -> (nv, kpv, n_orders) at 6 rows
SWEEP_OUT = (8, 16, 24, 28, 32, 40)
SWEEP_IN = {(2, 1): (2, 1, 2), (3, 2): (3, 1, 6), (2, 2): (2, 1, 2), (3, 1): (3, 1, 6), (4, 1): (2, 2, 2), (6, 2): (3, 2, 6)}
SWEEP_ROWS = 6
# model level: (hidden_features, channels per vertex)
MODEL_SHAPES = ((16, 1), (24, 1), (28, 1), (32, 1), (28, 2))


def sweep_cells():
    return [(an, out, in_f, nl) for an in ALGS for out in SWEEP_OUT for (in_f, nl) in SWEEP_IN]


def sweep_case(an, out, in_f, nl):
    nv, kpv, n_orders = SWEEP_IN[(in_f, nl)]
    return _case(ALGS[an], nl, nv, kpv, n_orders, SWEEP_ROWS // n_orders, kind="cell", out=out, seed_tag=f"cell-{an}-{out}-{in_f}x{nl}")


def _two_block(base):
    return BASES[base]["nl"] == 2


MEMBERS = {
    "default": list(BASES),
    # CSMPN_SAVE_STATE=0: the backward instantiation without saved state
    "recompute": [b for b in BASES if _two_block(b) and not BASES[b]["walk"]] + ["walk-tris-cl50-1031"],
}
CASES = {f"{b}@{g}": dict(BASES[b], seed_tag=b, group=g) for g, bases in MEMBERS.items() for b in bases}
CASES.update({f"guard:{b}@abi": dict(BASES[b], kind="guard", seed_tag=b, group="abi") for b in GUARD_BASES})
CASES.update({f"{b}@abi": dict(c, seed_tag=b, group="abi") for b, c in CLAMP_BASES.items()})
CASES["refusals@abi"] = dict(_case(CL50, 2, 3, 1, 6, 5, kind="refusals"), seed_tag="tris-cl50-5", group="abi")
CASES["sweep@abi"] = dict(kind="sweep", seed_tag="sweep", group="abi")
CASES.update({f"model-{h}-k{k}@abi": dict(kind="model", hidden=h, kpv=k, seed_tag=f"model-{h}-k{k}", group="abi")
              for h, k in MODEL_SHAPES})
GROUP_ENV = {"default": {}, "recompute": {"CSMPN_SAVE_STATE": "0"}, "abi": {}}
GROUPS = {g: (env, (lambda g: lambda t: t.endswith("@" + g))(g)) for g, env in GROUP_ENV.items()}

# Seed offsets of the seed tags whose first seed puts a float32 yardstick above YARD (general_helpers.RESEED; host runs, no
# kernel involved); the first offset 0, 1, .. under the cap stands here with the figures of the seeds that were not:
#   tris-cl50-1, offset 0: 1.08e-5 on g.layers.0.1.a (a sum over six rows); offset 1: worst yardstick 2.9e-6.
#   tris-cl41-23, offset 0: 1.01e-5 on g.layers.0.1.a; offset 1: 1.1e-6.
#   clamp-tris-cl41-23, offset 0: 4.5e-4 on g.layers.1.2.linear_right.weight (Cl(4,1): a row near the null cone); offset 1: 8.4e-7.
# Every other case is under the cap at offset 0. Worst yardstick per case (nearly always g.layers.0.1.a): Cl(5,0) small and
# C-ABI-only cases 6.7e-7 .. 5.3e-6, the two walks 1.2e-6 and 1.7e-6, Cl(4,1) 6.7e-7 .. 6.1e-6, the clamp cases 8.4e-7 and
# 1.2e-6, the four servable cells of the predicate sweep 1.2e-6 .. 3.3e-6; y: 6e-8 .. 5e-7.
RESEED = {"tris-cl50-1": 1, "tris-cl41-23": 1, "clamp-tris-cl41-23": 1}


# ------------------------------------------------------------------------------------------------- inputs and reference
def make_table(gen, rows, nv, n_orders):
    """verts [rows, nv] int32, random in [0, S - 8), holding - where the table is large enough - id 0 (first entry), id S - 9
    (last entry), one simplex whose vertices are all SAME_ID (simplex 1, from 3 simplices on) and two simplices with
    identical rows (simplex nsimp - 2 repeats simplex 2, from 5 simplices on)."""
    nsimp = rows // n_orders
    verts = torch.randint(0, S_ROWS - POISON_ROWS, (rows, nv), generator=gen).to(torch.int32)
    if nsimp >= 3:
        verts[n_orders:2 * n_orders] = SAME_ID
    if nsimp >= 5:
        verts[(nsimp - 2) * n_orders:(nsimp - 1) * n_orders] = verts[2 * n_orders:3 * n_orders]
    verts[0, 0] = 0
    verts[-1, -1] = S_ROWS - POISON_ROWS - 1
    return verts


def case_inputs(c, seed):
    """(feat [S, kpv, D], verts [rows, nv] int32, params, gout [nsimp, out, D]) of a case, float32, on the host."""
    metric = c["metric"]
    o32 = O.Algebra(list(metric), torch.float32)
    gen = torch.Generator().manual_seed(seed)
    p = O.init_cemlp_params(o32, c["in_f"], c["out"], c["out"], n_layers=c["nl"], gen=gen, randomize=True)
    feat = G._tame(o32, metric, torch.randn(S_ROWS, c["kpv"], o32.D, generator=gen))
    if c["poison"]:
        feat[S_ROWS - POISON_ROWS:] = POISON
    rows = c["nsimp"] * c["n_orders"]
    verts = make_table(gen, rows, c["nv"], c["n_orders"])
    if c["kind"] == "clamp":    # three ids outside [0, S): the kernels clamp them to 0 and S - 1
        verts[1, 0], verts[rows // 2, c["nv"] - 1], verts[rows - 2, 0] = -1, S_ROWS, S_ROWS + 1000
    gout = torch.randn(c["nsimp"], c["out"], o32.D, generator=gen)
    return feat, verts, p, gout


_algs = {}


def _alg(metric, dtype):
    key = (tuple(metric), dtype)
    if key not in _algs:
        _algs[key] = O.Algebra(list(metric), dtype)
    return _algs[key]


def row_loss(alg, f, verts, q, gout_rows):
    """sum over the given rows of <CEMLP(x_row), gout_rows>: a row's own share of the loss (gout_rows [rows, O, D])."""
    v = verts.long()
    x = f[v].reshape(v.shape[0], v.shape[1] * f.shape[1], alg.D)
    y = O.cemlp(alg, x, q)
    return y, (y * gout_rows).sum()


def reference_run(metric, feat, verts, n_orders, params, gout, dtype, chunk_rows=1000):
    """{'y': out [nsimp, O, D], 'g.<parameter>': d loss / d parameter} in `dtype`; gout None: forward only."""
    alg = _alg(metric, dtype)
    q = {k: v.detach().to(dtype).clone().requires_grad_(gout is not None) for k, v in params.items()}
    f = feat.detach().to(dtype)
    nsimp = verts.shape[0] // n_orders
    assert nsimp * n_orders == verts.shape[0]
    per = max(1, chunk_rows // n_orders)
    outs = []
    for s0 in range(0, nsimp, per):
        s1 = min(s0 + per, nsimp)
        rows = torch.arange(s0 * n_orders, s1 * n_orders)
        with torch.set_grad_enabled(gout is not None):
            if gout is None:
                y, _ = row_loss(alg, f, verts[rows], q, 0.0)
            else:
                y, loss = row_loss(alg, f, verts[rows], q, gout.to(dtype)[rows // n_orders])
                loss.backward()
        outs.append(y.detach().reshape(s1 - s0, n_orders, y.shape[1], alg.D).sum(1))
    res = {"y": torch.cat(outs).numpy()}
    if gout is not None:
        res.update({"g." + k: v.grad.numpy() for k, v in q.items()})
    return res


def row_gradients(metric, feat, verts, n_orders, params, gout, rows):
    """{'g.<parameter>'}: the share of the given rows (a 1-D index tensor) in the parameter gradients, float64."""
    alg = _alg(metric, torch.float64)
    q = {k: v.detach().double().clone().requires_grad_(True) for k, v in params.items()}
    _, loss = row_loss(alg, feat.double(), verts[rows], q, gout.double()[rows // n_orders])
    loss.backward()
    return {"g." + k: v.grad.numpy() for k, v in q.items()}


def clamped(verts):
    return verts.clamp(0, S_ROWS - 1)


def compare(name, got, t64, t32):
    """Every tensor within max(1e-5, 4 x float32 yardstick) of the float64 truth, plus the element-wise bound of `check`.
    Returns (message, worst ratio err / bound)."""
    assert set(got) == set(t64) == set(t32), (sorted(got), sorted(t64))
    errs = {}
    for k in sorted(got):
        errs[k] = (G.check(f"{name} {k}", got[k].reshape(t64[k].shape), t64[k], t32[k], SLACK), relmax(t32[k], t64[k]))
    ratio = lambda k: errs[k][0] / max(G.TOL, SLACK * errs[k][1])
    worst = max(errs, key=ratio)
    return f"worst tensor {worst}: HIP err {errs[worst][0]:.2e}, float32 yardstick {errs[worst][1]:.2e}", ratio(worst)


def assert_yardsticks(name, t64, t32):
    yard = {k: relmax(t32[k], t64[k]) for k in t64}
    worst = max(yard, key=yard.get)
    assert yard[worst] <= YARD, f"{name}: yardstick of {worst} is {yard[worst]:.3e} > {YARD:.0e}"
    return yard


# ---------------------------------------------------------------------------------------------------------- the child
def _module(c, p, metric=None):
    pkg = G._pkg()
    m = pkg.CEMLP(pkg.CliffordAlgebra(tuple(metric or c["metric"])), c["in_f"], c["out"], c["out"], n_layers=c["nl"])
    return G._load(m, p) if p is not None else m.to(G.dev())


def _grads(m):
    return {"g." + k: v.grad.detach().cpu().numpy() for k, v in m.named_parameters()}


class Guarded:
    """`n` elements between two runs of sentinels, the interior NaN (float32) or 0xFF bytes (uint8: NaN as floats)."""
    GUARD = 4096

    def __init__(self, n, dev, dtype=torch.float32):
        self.n, self.sentinel = n, (-12345.0 if dtype == torch.float32 else 0xA5)
        self.full = torch.full((n + 2 * self.GUARD,), self.sentinel, dtype=dtype, device=dev)
        self.body = self.full[self.GUARD:self.GUARD + n]
        self.body.fill_(float("nan") if dtype == torch.float32 else 0xFF)

    def ptr(self):
        return self.body.data_ptr() if self.n else None

    def intact(self):
        return bool((torch.cat([self.full[:self.GUARD], self.full[self.GUARD + self.n:]]) == self.sentinel).all())

    def untouched(self):
        same = torch.isnan(self.body) if self.body.dtype == torch.float32 else self.body == 0xFF
        return self.intact() and bool(same.all())


class Abi:
    """The two entry points through ctypes on buffers of exactly the documented sizes, each between sentinels."""

    def __init__(self, c, feat, verts, p, metric=None, module=None):
        from csmpn_hip import native, ops
        self.native, self.lib, self.d = native, native.lib(), G.dev()
        self.c = c
        self.m = module if module is not None else _module(c, p, metric)
        self.b, self.params = self.m.binding(), self.m.flat_params()
        self.b.bind(self.params)
        self.feat, self.verts = feat.to(self.d).contiguous(), verts.to(self.d).contiguous()
        self.st = ops._stream(self.d)
        self.rows = int(verts.shape[0])
        self.out = Guarded((self.rows // c["n_orders"]) * c["out"] * self.b.D, self.d)
        self.ws = Guarded(int(self.lib.csmpn_cemlp_workspace_bytes(self.b.n, self.b.params, self.b.nblk)), self.d, torch.uint8)
        self.saved = None

    def new_saved(self, flags):
        n = int(self.lib.csmpn_cemlp_saved_floats(self.b.n, self.b.params, self.b.nblk, self.rows,
                                                  flags & self.native.FLAG_SAVE_STATE))
        self.saved = Guarded(n, self.d)
        return n

    def forward(self, flags, **over):
        c, b = self.c, self.b
        a = dict(n_vertex_rows=int(self.feat.shape[0]), kpv=c["kpv"], nv=c["nv"], n_orders=c["n_orders"], rows=self.rows)
        a.update(over)
        return self.lib.csmpn_embed_cemlp_forward(
            b.metric_arr, b.n, b.params, b.nblk, self.feat.data_ptr(), a["n_vertex_rows"], a["kpv"], self.verts.data_ptr(), a["nv"],
            a["n_orders"], a["rows"], self.out.body.data_ptr(), self.saved.ptr() if self.saved else None, self.ws.body.data_ptr(),
            self.ws.n, flags, self.st)

    def backward(self, gout, flags, flat=None, saved=True):
        c, b = self.c, self.b
        self.gout = gout.to(self.d).contiguous()
        self.flat, self.views = b.new_grads(self.params, self.d, flat=flat)
        return self.lib.csmpn_embed_cemlp_backward(
            b.metric_arr, b.n, b.params, b.grads, b.nblk, self.feat.data_ptr(), int(self.feat.shape[0]), c["kpv"],
            self.verts.data_ptr(), c["nv"], c["n_orders"], self.rows, self.gout.data_ptr(),
            self.saved.ptr() if (saved and self.saved) else None, self.ws.body.data_ptr(), self.ws.n, flags, self.st)

    def tensors(self):
        """y and g.<parameter> of the last forward / backward."""
        torch.cuda.synchronize()
        c = self.c
        got = {"y": self.out.body.reshape(-1, c["out"], self.b.D).cpu().numpy()}
        names = [k for k, _ in self.m.named_parameters()]
        by_ptr = {p.data_ptr(): k for k, p in self.m.named_parameters()}
        assert len(by_ptr) == len(names)
        for p, v in zip(self.params, self.views):
            if p is not None:
                got["g." + by_ptr[p.data_ptr()]] = v.cpu().numpy()
        return got

    def error(self):
        return self.lib.csmpn_last_error().decode()


def _expect(rc, want, what, abi=None):
    assert rc == want, f"{what}: returned {rc}, expected {want}" + (f" ({abi.error()})" if abi is not None and rc else "")


class EmbedSuite(Suite):
    out_dir = None

    def child_env(self, group):
        if EmbedSuite.out_dir is None:
            EmbedSuite.out_dir = tempfile.mkdtemp(prefix="embed_")
            atexit.register(shutil.rmtree, EmbedSuite.out_dir, ignore_errors=True)
        env = {k: v for k, v in super().child_env(group).items() if k not in ("CSMPN_SAVE_STATE", "CSMPN_NO_FUSED_EMBED", "CSMPN_NO_PLW")
               or k in self.groups[group][0]}
        return dict(env, EMBED_OUT=EmbedSuite.out_dir)

    def inputs(self, tag):
        return case_inputs(self.cases[tag], self.seed(tag))

    def child_main(self, group):
        G._pkg()    # the package puts csmpn / csmpn_hip on the path
        super().child_main(group)

    # ------------------------------------------------------------------------------------------------ kinds of cases
    def hip_embed(self, tag):
        """The case through ops.embed_cemlp_apply and autograd: out and every parameter gradient; embed_launches() must
        advance by one per forward."""
        from csmpn_hip import ops
        c = self.cases[tag]
        feat, verts, p, gout = self.inputs(tag)
        m = _module(c, p)
        assert ops.embed_cemlp_supported(m.binding(), c["nv"], c["kpv"]), "the predicate rejects a shape of the case table"
        n0 = ops.embed_launches()
        y = ops.embed_cemlp_apply(feat.to(G.dev()), verts.to(G.dev()), c["n_orders"], m.binding(), m.flat_params())
        assert ops.embed_launches() == n0 + 1, "embed_launches() did not advance by one"
        (y * gout.to(G.dev())).sum().backward()
        torch.cuda.synchronize()
        assert ops.embed_launches() == n0 + 1
        return {"y": y.detach().cpu().numpy(), **_grads(m)}

    def hip_guard(self, tag):
        c = self.cases[tag]
        feat, verts, p, gout = self.inputs(tag)
        got = {}
        for v in GUARD_VARIANTS:
            say(G._NOTE + v)
            abi = Abi(c, feat, verts, p)
            fl = abi.native.FLAG_SAVE_STATE if v == "state" else 0
            got[f"{v}.floats.saved"] = np.asarray(abi.new_saved(fl))
            got[f"{v}.floats.out"] = np.asarray(abi.out.n)
            got[f"{v}.bytes.ws"] = np.asarray(abi.ws.n)
            _expect(abi.forward(fl), 0, "forward", abi)
            _expect(abi.backward(gout, fl | abi.native.FLAG_NO_VALIDATE), 0, "backward", abi)
            for k, t in abi.tensors().items():
                got[f"{v}.{k}"] = t
            for k, g in (("out", abi.out), ("saved", abi.saved), ("ws", abi.ws)):
                got[f"{v}.intact.{k}"] = np.asarray(g.intact())
        return got

    def hip_clamp(self, tag):
        c = self.cases[tag]
        feat, verts, p, gout = self.inputs(tag)
        abi = Abi(c, feat, verts, p)
        nat = abi.native
        fl = nat.FLAG_SAVE_STATE if c["nl"] == 2 else 0
        abi.new_saved(fl)
        say(G._NOTE + "validated")
        _expect(abi.forward(fl), nat.ERR_INVALID, "forward on a table that holds -1 and S", abi)
        assert "outside" in abi.error(), abi.error()
        torch.cuda.synchronize()
        assert abi.out.untouched(), "the refused forward wrote to out"
        nan_flat = torch.full((abi.b.grad_floats(abi.params),), float("nan"), device=abi.d)
        _expect(abi.backward(gout, fl, flat=nan_flat), nat.ERR_INVALID, "backward on a table that holds -1 and S", abi)
        torch.cuda.synchronize()
        assert bool(torch.isnan(nan_flat).all()), "the refused backward wrote to the gradients"
        say(G._NOTE + "clamped")
        _expect(abi.forward(fl | nat.FLAG_NO_VALIDATE), 0, "forward with CSMPN_FLAG_NO_VALIDATE", abi)
        _expect(abi.backward(gout, fl | nat.FLAG_NO_VALIDATE), 0, "backward with CSMPN_FLAG_NO_VALIDATE", abi)
        got = abi.tensors()
        assert abi.out.intact() and abi.saved.intact() and abi.ws.intact(), "a sentinel is gone"
        return got

    def hip_refusals(self, tag):
        """Every refusal: the documented code, nothing launched (no `[csmpn]` line between the notes: the host checks), out
        (the parameter gradients of the backward) untouched."""
        c = self.cases[tag]
        feat, verts, p, gout = self.inputs(tag)
        got = {}

        def refused(name, want, rc, abi, buf=None):
            torch.cuda.synchronize()
            _expect(rc, want, name, None)
            assert (abi.out.untouched() if buf is None else bool(torch.isnan(buf).all())), f"{name}: the refused call wrote its output"
            assert abi.ws.untouched(), f"{name}: the refused call wrote to the workspace"
            got[name] = np.asarray(rc)
            say(G._NOTE + f"refused {name}: {abi.error()}")

        def fresh(case=c, f=feat, v=verts, params=p, metric=None):
            a = Abi(case, f, v, params, metric)
            a.new_saved(a.native.FLAG_SAVE_STATE)
            return a

        from csmpn_hip import native as nat
        fl = nat.FLAG_SAVE_STATE
        a = fresh()
        refused("rows-not-multiple", nat.ERR_INVALID, a.forward(fl, rows=a.rows - 1), a)
        refused("three-orders", nat.ERR_UNSUPPORTED, a.forward(fl, n_orders=3), a)
        refused("width-mismatch", nat.ERR_UNSUPPORTED, a.forward(fl, nv=2), a)        # 2 x 1 != 3 input channels
        refused("no-vertex-rows", nat.ERR_INVALID, a.forward(fl, n_vertex_rows=0), a)
        # 9 input channels = 3 vertices x 3 channels, in_features 9: more than the one 8-channel input chunk
        c9 = dict(c, in_f=9, kpv=3)
        f9 = torch.randn(S_ROWS, 3, D, generator=torch.Generator().manual_seed(1))
        a9 = fresh(c9, f9, verts, None)
        refused("nine-inputs", nat.ERR_UNSUPPORTED, a9.forward(fl), a9)
        f3 = torch.randn(S_ROWS, 1, 8, generator=torch.Generator().manual_seed(2))
        a3 = fresh(c, f3, verts, None, CL30)
        refused("cl30", nat.ERR_UNSUPPORTED, a3.forward(fl), a3)
        # a two-block backward without the saved block inputs (behind a forward that wrote them: only the pointer is missing)
        say(G._NOTE + "forward for the backward refusal")
        b = fresh()
        _expect(b.forward(fl), 0, "forward", b)
        say(G._NOTE + "backward refusal")
        nan_flat = torch.full((b.b.grad_floats(b.params),), float("nan"), device=b.d)
        refused_ws = b.ws
        rc = b.backward(gout, fl | nat.FLAG_NO_VALIDATE, flat=nan_flat, saved=False)
        torch.cuda.synchronize()
        _expect(rc, nat.ERR_UNSUPPORTED, "no-saved-inputs", None)
        assert bool(torch.isnan(nan_flat).all()), "no-saved-inputs: the refused backward wrote to the gradients"
        assert refused_ws.intact() and b.saved.intact() and b.out.intact()
        got["no-saved-inputs"] = np.asarray(rc)
        say(G._NOTE + f"refused no-saved-inputs: {b.error()}")
        assert sorted(got) == sorted(REFUSALS)
        return got

    def hip_sweep(self, tag):
        """Every cell: the predicate and the forward's return code; a served cell also runs its backward and is stored."""
        from csmpn_hip import native as nat, ops
        got = {}
        for cell in sweep_cells():
            c = sweep_case(*cell)
            name = c["seed_tag"]
            say(G._NOTE + name)
            feat, verts, p, gout = case_inputs(c, self.seed_of(name))
            abi = Abi(c, feat, verts, p)
            fl = nat.FLAG_SAVE_STATE if c["nl"] == 2 else 0
            abi.new_saved(fl)
            rc = abi.forward(fl)
            got[f"{name}.rc"] = np.asarray(rc)
            got[f"{name}.supported"] = np.asarray(bool(ops.embed_cemlp_supported(abi.b, c["nv"], c["kpv"])))
            if rc == 0:
                _expect(abi.backward(gout, fl | nat.FLAG_NO_VALIDATE), 0, f"backward of {name}", abi)
                for k, t in abi.tensors().items():
                    got[f"{name}.{k}"] = t
                assert abi.out.intact() and abi.saved.intact() and abi.ws.intact(), f"{name}: a sentinel is gone"
            else:
                torch.cuda.synchronize()
                assert rc == nat.ERR_UNSUPPORTED, f"{name}: returned {rc} ({abi.error()})"
                assert abi.out.untouched(), f"{name}: the refused forward wrote to out"
        return got

    def seed_of(self, seed_tag):
        return 2000 + sum((i + 1) * ord(ch) for i, ch in enumerate(seed_tag)) + self.reseed.get(seed_tag, 0)

    def hip_model(self, tag):
        """SimplexEmbedding as HullsSimplicialMPNN holds it (one vertex channel) or on its own (two): forward + backward of
        the embedding on the device, the launches counted; then, for the hulls model, one training step. Stored: what the host
        needs for the reference of the rows of dimension >= 1 (embedded features, index tables, the module's parameters)."""
        from csmpn.models import simplicial_mpnn as M
        from csmpn_hip import ops
        from test_model_harness import _hull_batch
        c = self.cases[tag]
        d = G.dev()
        torch.manual_seed(self.seed(tag))
        batch = _hull_batch(None, seed=5, n_graphs=3, device=d)
        if c["kpv"] == 1:
            model = M.HullsSimplicialMPNN(hidden_features=c["hidden"], num_layers=1).to(d)
            emb, algebra = model._embed, model.algebra
            block = batch.input.unsqueeze(1)
        else:
            algebra = G._pkg().CliffordAlgebra(CL50)
            model = None
            emb = M.SimplexEmbedding(algebra, c["kpv"], c["hidden"], 2).to(d)
            algebra = emb.algebra
            block = torch.randn(batch.input.shape[0], c["kpv"], 5, generator=torch.Generator().manual_seed(7)).to(d)
        with torch.no_grad():    # every parameter away from its initial 0 / 1
            for k, prm in emb.named_parameters():
                if k.endswith(("bias", ".a", ".b")):
                    prm.add_(0.3 * torch.randn(prm.shape, generator=torch.Generator().manual_seed(len(k))).to(d))
        plan = batch.plan(2)
        pred = all(ops.embed_cemlp_supported(emb.cl_feature_embedding[k].binding(), k + 1, c["kpv"]) for k in (1, 2))
        n0 = ops.embed_launches()
        x = emb(batch, [(block, 1)])
        w = torch.randn(x.shape, generator=torch.Generator().manual_seed(3)).to(d)
        (x * w).sum().backward()
        torch.cuda.synchronize()
        got = {"launches": np.asarray(ops.embed_launches() - n0), "predicate": np.asarray(pred),
               "feat": algebra.embed_grade(block, 1).detach().cpu().numpy()}
        for k in (1, 2):
            rows = plan["rows"][k]
            got[f"verts{k}"] = plan["verts"][k].to(torch.int32).cpu().numpy()
            got[f"x{k}"] = x.detach()[rows].cpu().numpy()
            got[f"w{k}"] = w[rows].cpu().numpy()
            for name, prm in emb.cl_feature_embedding[k].named_parameters():
                got[f"p{k}.{name}"] = prm.detach().cpu().numpy()
                got[f"g{k}.{name}"] = prm.grad.detach().cpu().numpy()
        if model is not None:
            say(G._NOTE + "training step")
            opt = torch.optim.Adam(model.parameters(), lr=1e-3)
            before = [prm.detach().clone() for prm in model.parameters()]
            opt.zero_grad(set_to_none=True)
            loss, _ = model(batch, 0, "train")
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
            assert bool(torch.isfinite(loss)), "the training step's loss is not finite"
            assert all(bool(torch.isfinite(prm).all()) for prm in model.parameters()), "a parameter is not finite after the step"
            moved = sum(int(not torch.equal(a, prm.detach())) for a, prm in zip(before, model.parameters()))
            got["moved"], got["loss"] = np.asarray(moved), np.asarray(float(loss))
        return got

    def child_case(self, tag):
        c = self.cases[tag]
        if c["kind"] == "embed":
            got = self.hip_embed(tag)
            say(G._NOTE + "run 2")
            again = self.hip_embed(tag)
            differ = [k for k in sorted(got) if not np.array_equal(got[k], again[k], equal_nan=True)]
            assert not differ, f"not bit-identical between two runs: {differ}"
        else:
            got = getattr(self, "hip_" + c["kind"])(tag)
        np.savez(os.path.join(os.environ["EMBED_OUT"], tag.replace(":", "_") + ".npz"), **got)
        return "stored"


SUITE = EmbedSuite("embed_helpers", CASES, GROUPS, RESEED)
group_of, group_tags = SUITE.group_of, SUITE.group_tags


# ------------------------------------------------------------------------------------------------------------ the host
_refs = {}


def reference(seed_tag, c=None, table=None):
    """(float64 truth, float32 yardstick run) of a seed tag, computed once; asserts the condition of the bound - every
    float32 yardstick at most 1e-5 - before anything looks at a HIP result. table: the index table to use instead of the
    case's own (the clamped one)."""
    if seed_tag not in _refs:
        c = c or BASES.get(seed_tag) or CLAMP_BASES[seed_tag]
        feat, verts, p, gout = case_inputs(c, SUITE.seed_of(seed_tag))
        verts = table(verts) if table else verts
        t64, t32 = (reference_run(c["metric"], feat, verts, c["n_orders"], p, gout, dt) for dt in (torch.float64, torch.float32))
        assert_yardsticks(seed_tag, t64, t32)
        _refs[seed_tag] = (t64, t32)
    return _refs[seed_tag]


def result(tag):
    """The case's entry of its group's child (general_helpers.Suite.run_group) with `got`: the tensors the child stored."""
    r = SUITE.run_group(group_of(tag))[tag]
    if "got" not in r and r["ok"]:
        with np.load(os.path.join(EmbedSuite.out_dir, tag.replace(":", "_") + ".npz")) as z:
            r["got"] = {k: z[k] for k in z.files}
    return r


def check_launches(c, ls, name=""):
    """One forward / backward pair's lines: MODE_PLAIN on plw, the case's channels, input channels and rows; a walk case has
    rows > grid x 4 x GT in the forward and rows > grid x 4 in the backward with the grid at its cap, every other case <=."""
    geo = geometry(c)
    assert [(l["family"], l["mode"], l["bwd"]) for l in ls] == [("plw", 0, 0), ("plw", 0, 1)], (name, ls)
    for l in ls:
        assert (l["channels"], l["attr"], l["rows"]) == (c["out"], c["in_f"], geo["rows"]), (name, l)
        held = l["grid"] * TILE * (1 if l["bwd"] else group_tiles(c["n_orders"]))
        if c["walk"]:
            assert l["grid"] == (BWD_CAP if l["bwd"] else FWD_CAP) and l["rows"] > held, f"{name}: does not walk: {l}"
        else:
            assert l["rows"] <= held, f"{name}: walks unexpectedly: {l}"
