"""The deterministic forms of the four standalone small layers (csmpn_mvsilu_backward_det,
csmpn_mvnorm_backward_det, csmpn_mvlayernorm_forward_det / _backward_det, csmpn_wgp_backward_det: contributions parked in LDS
and added in a fixed order, one partial row per workgroup in scratch, a second launch that adds the rows - no float
atomics): the nn.Modules under a deterministic request against their own host formulation in float64, bit-identical
repeated runs in this process and in a fresh one, agreement with the default forms, the C-ABI contracts, and a block
composed from the modules under nothing but torch.use_deterministic_algorithms(True)."""
import copy
import functools
import os
import subprocess
import sys
import warnings

import pytest
import torch

from small_layers_det_helpers import CHILD_CASES, DET_CALLS, LAYERS, METRICS, digest, make_case, run_module

pytestmark = pytest.mark.gpu

MAX_PARTS, TILE = 512, 256     # include/csmpn_hip.h: at most 512 partial rows; a tile = 256 lanes


def rows_past_the_cap(C):
    """The smallest row count at which every one of the four layers has more tiles than partial rows, so that a workgroup
    walks several tiles: rows * C > 512 * 256 elements (MVSiLU, NormalizationLayer, the product) and rows > 512 *
    floor(256 / C) rows (MVLayerNorm)."""
    return max(MAX_PARTS * TILE // C + 1, MAX_PARTS * (TILE // C) + 1)


CAPPED = rows_past_the_cap(33)
assert CAPPED == 3972 and -(-CAPPED * 33 // TILE) == MAX_PARTS + 1 and -(-CAPPED // (TILE // 33)) > MAX_PARTS

SHAPES = [("cl30", 1, 1),
          ("cl20", 3, 5),          # one ragged workgroup
          ("cl30", 33, 257),       # C does not divide 256, many workgroups, ragged tail
          ("cl40", 129, 37),       # one MVLayerNorm row per workgroup with idle lanes
          ("cl50", 256, 21),       # channel limit, heaviest LDS of the product
          ("cl41", 8, 1031),
          ("cl31", 20, 257),
          ("cl30", 33, CAPPED),    # 513 tiles of 256 lanes: two per workgroup, 257 partial rows
          ("cl30", 33, 4100)]      # 529 tiles: two per workgroup, 265 partial rows, the last workgroup takes one


def dev():
    return torch.device("cuda:0")


class Case:
    """Seeded module and inputs of one (layer, shape), the module's host formulation in float64 (the truth) and in float32
    (the yardstick) on the CPU. Computed once, shared by the tests below, never written."""

    def __init__(self, pkg, layer, name, C, rows):
        self.layer = layer
        self.mod, self.x, self.gout = make_case(pkg, layer, name, C, rows)
        self.truth = run_module(copy.deepcopy(self.mod).double(), self.x.double(), self.gout.double())
        self.host32 = run_module(copy.deepcopy(self.mod), self.x, self.gout)
        self.names = ["y", "gx"] + [k for k, _ in self.mod.named_parameters()]
        self._dev = None

    def device(self):
        if self._dev is None:
            self._dev = (copy.deepcopy(self.mod).to(dev()), self.x.to(dev()), self.gout.to(dev()))
        return self._dev

    def bound(self, i):
        """(scale, relative bound) of result i: 5e-5 of the tensor's scale, or 4x the float32 host formulation's own
        error where the layer is ill-conditioned (the bound of test_small_layers_hip_vs_host_fp64)."""
        b = self.truth[i].float()
        scale = float(b.abs().max().clamp(min=1e-30))
        yard = float((self.host32[i] - b).abs().max()) / scale
        return scale, max(5e-5, 4 * yard), yard


@functools.lru_cache(maxsize=None)
def _case(pkg, layer, name, C, rows):
    return Case(pkg, layer, name, C, rows)


def run_on_device(case, request):
    """One forward + backward of the case's module on the device under ops.set_deterministic(request)."""
    from csmpn_hip import ops
    mod, x, gout = case.device()
    ops.set_deterministic(request)
    try:
        out = run_module(mod, x, gout)
        torch.cuda.synchronize()
        return [t.clone() for t in out]
    finally:
        ops.set_deterministic(None)


@pytest.mark.parametrize("name,C,rows", SHAPES)
@pytest.mark.parametrize("layer", LAYERS)
def test_module_under_a_request_against_fp64_and_bit_repeatable(pkg, layer, name, C, rows):
    from csmpn_hip import ops
    case = _case(pkg, layer, name, C, rows)
    before, small_before = ops.det_launches(), ops.small_layer_launches()
    runs = [run_on_device(case, True) for _ in range(3)]
    assert ops.det_launches() - before == 3 * DET_CALLS[layer], "the _det entry points did not run as expected"
    assert ops.small_layer_launches() > small_before
    for i, what in enumerate(case.names):
        scale, bound, yard = case.bound(i)
        err = float((runs[0][i].cpu() - case.truth[i].float()).abs().max()) / scale
        print(f"{layer} {name} C={C} rows={rows} {what}: rel err {err:.2e}, float32 host formulation {yard:.2e}, bound {bound:.2e}")
        assert err < bound, f"{what}: rel err {err:.2e} (float32 host formulation: {yard:.2e})"
        for r in runs[1:]:
            assert torch.equal(runs[0][i], r[i]), f"{what} differs between two runs"


@pytest.mark.parametrize("name,C,rows", SHAPES)
@pytest.mark.parametrize("layer", LAYERS)
def test_det_agrees_with_the_default_form(pkg, layer, name, C, rows):
    """Same inputs through the default (float atomics) and the _det forms: only the summation order differs."""
    from csmpn_hip import ops
    case = _case(pkg, layer, name, C, rows)
    before = ops.det_launches()
    plain = run_on_device(case, False)
    assert ops.det_launches() == before, "no request, yet a _det entry point ran"
    det = run_on_device(case, True)
    for i, what in enumerate(case.names):
        scale, bound, yard = case.bound(i)
        err = float((det[i] - plain[i]).abs().max()) / scale
        print(f"{layer} {name} C={C} rows={rows} {what}: det vs default {err:.2e}, bound {bound:.2e}")
        assert err < bound, f"{what}: det vs default {err:.2e}"


# ------------------------------------------------------------------------------------------------- straight through the C-ABI
OPS = ["mvsilu", "mvnorm", "mvlayernorm", "wgp"]


class Direct:
    """Device buffers of one op on [rows, C, D] and its backward entry points called straight through the C-ABI."""

    def __init__(self, pkg, op, name="cl30", C=33, rows=257, alloc_rows=None):
        from csmpn_hip import native
        self.native, self.lib, self.op = native, native.lib(), op
        self.metric, self.n = METRICS[name], len(METRICS[name])
        self.C, self.rows = C, rows
        D, G = 1 << self.n, self.n + 1
        P = int(pkg.CliffordAlgebra(self.metric).geometric_product_paths.sum())
        gen = torch.Generator().manual_seed(4242 + OPS.index(op))
        r = max(rows if alloc_rows is None else alloc_rows, 1)
        rnd = lambda *s: torch.randn(*s, generator=gen).to(dev())
        self.x, self.r, self.gy = rnd(r, C, D), rnd(r, C, D), rnd(r, C, D)
        shapes = {"mvsilu": [(C, G), (C, G)], "mvnorm": [(C, G)], "mvlayernorm": [(C,)], "wgp": [(C, P)]}[op]
        self.params = [rnd(*s) for s in shapes]
        self.n_out = 2 if op == "wgp" else 1            # gz and gr
        self.op_id = {"mvsilu": native.LAYER_MVSILU, "mvnorm": native.LAYER_MVNORM, "mvlayernorm": native.LAYER_MVLAYERNORM,
                      "wgp": native.LAYER_WGP}[op]
        self.bytes = int(self.lib.csmpn_small_layer_det_bytes(self.op_id, self.n, rows, C))

    def backward(self, det, outs, grads, ws_ptr=None, ws_bytes=0):
        """Return code of csmpn_<op>_backward[_det]; outs / grads are written / accumulated in place."""
        m, st = self.native.metric_array(self.metric), torch.cuda.current_stream().cuda_stream
        ins = [self.x.data_ptr()] + ([self.r.data_ptr()] if self.op == "wgp" else []) + [p.data_ptr() for p in self.params]
        args = [m, self.n, *ins, self.gy.data_ptr(), self.rows, self.C, *[t.data_ptr() for t in outs], *[t.data_ptr() for t in grads]]
        fn = getattr(self.lib, f"csmpn_{self.op}_backward" + ("_det" if det else ""))
        rc = fn(*args, ws_ptr, ws_bytes, st) if det else fn(*args, st)
        torch.cuda.synchronize()
        return rc

    def fresh(self, out_fill=float("nan"), grad_fill=0.0):
        return ([torch.full_like(self.x, out_fill) for _ in range(self.n_out)],
                [torch.full_like(p, grad_fill) for p in self.params])

    def det(self, grad_fill=0.0, ws_fill=0.0):
        outs, grads = self.fresh(grad_fill=grad_fill)
        ws = torch.full((self.bytes // 4,), ws_fill, dtype=torch.float32, device=dev())
        assert self.backward(True, outs, grads, ws.data_ptr(), self.bytes) == 0, self.lib.csmpn_last_error()
        return outs + grads


# 257 rows: one tile per workgroup; past the cap: two tiles per workgroup, the partial row is read back and added to
@pytest.mark.parametrize("rows", [257, CAPPED])
@pytest.mark.parametrize("op", OPS)
def test_cabi_accumulates_and_reads_no_unwritten_scratch(pkg, op, rows):
    d = Direct(pkg, op, rows=rows)
    assert d.bytes > 0 and d.bytes % 4 == 0
    zero = d.det()
    assert all(bool(torch.isfinite(t).all()) for t in zero)
    # += : targets pre-filled with a constant hold the constant plus the gradient (one rounding, the kernel's own add)
    filled = d.det(grad_fill=0.75)
    for z, f in zip(zero[:d.n_out], filled[:d.n_out]):
        assert torch.equal(z, f)
    for z, f in zip(zero[d.n_out:], filled[d.n_out:]):
        assert float(z.abs().max()) > 0 and torch.equal(f, 0.75 + z)
    # scratch full of NaN before the call: the same bits, so no word is read that the call did not write
    for a, b in zip(zero, d.det(ws_fill=float("nan"))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("op", OPS)
def test_cabi_rejects_a_missing_or_small_workspace(pkg, op):
    d = Direct(pkg, op)
    ws = torch.zeros(d.bytes // 4, dtype=torch.float32, device=dev())
    for ptr, nbytes in ((None, d.bytes), (None, 0), (ws.data_ptr(), d.bytes - 1), (ws.data_ptr(), 0)):
        outs, grads = d.fresh(out_fill=7.0, grad_fill=3.0)
        assert d.backward(True, outs, grads, ptr, nbytes) == d.native.ERR_INVALID, (ptr, nbytes)
        assert "csmpn_small_layer_det_bytes" in d.lib.csmpn_last_error().decode()
        assert all(bool((t == 7.0).all()) for t in outs) and all(bool((t == 3.0).all()) for t in grads)


@pytest.mark.parametrize("op", OPS)
def test_cabi_empty_input_and_channel_limit(pkg, op):
    # rows == 0: CSMPN_OK, nothing touched, no workspace needed
    d = Direct(pkg, op, rows=0)
    assert d.bytes == 0
    outs, grads = d.fresh(out_fill=7.0, grad_fill=3.0)
    assert d.backward(True, outs, grads, None, 0) == 0
    assert all(bool((t == 7.0).all()) for t in outs) and all(bool((t == 3.0).all()) for t in grads)
    # 257 channels: CSMPN_ERR_INVALID as the default forms, nothing launched
    d = Direct(pkg, op, C=257, rows=5)
    assert d.bytes == 0
    ws = torch.zeros(1 << 20, dtype=torch.float32, device=dev())
    outs, grads = d.fresh(out_fill=7.0, grad_fill=3.0)
    assert d.backward(True, outs, grads, ws.data_ptr(), ws.numel() * 4) == d.native.ERR_INVALID
    assert "1..256" in d.lib.csmpn_last_error().decode()
    assert all(bool((t == 7.0).all()) for t in outs) and all(bool((t == 3.0).all()) for t in grads)


def test_cabi_mvlayernorm_forward_det(pkg):
    """The one forward with a _det form: same numbers as the default forward up to the order of the row sum, the same bits
    twice, empty input and the channel limit."""
    d = Direct(pkg, "mvlayernorm")
    m, st = d.native.metric_array(d.metric), torch.cuda.current_stream().cuda_stream

    def fwd(name, x, a, rows, C, y):
        rc = getattr(d.lib, name)(m, d.n, x.data_ptr(), a.data_ptr(), rows, C, y.data_ptr(), st)
        torch.cuda.synchronize()
        return rc

    y0, y1, y2 = (torch.full_like(d.x, float("nan")) for _ in range(3))
    assert fwd("csmpn_mvlayernorm_forward", d.x, d.params[0], d.rows, d.C, y0) == 0
    assert fwd("csmpn_mvlayernorm_forward_det", d.x, d.params[0], d.rows, d.C, y1) == 0
    assert fwd("csmpn_mvlayernorm_forward_det", d.x, d.params[0], d.rows, d.C, y2) == 0
    assert torch.equal(y1, y2)
    # two float32 sums of the row's C positive norms differ by at most 2 (C - 1) 2^-24 relative, whatever their order; the
    # division, the product with a_c x and the 1e-6 floor add a few roundings of 2^-24 each
    assert torch.allclose(y1, y0, rtol=(2 * (d.C - 1) + 8) * 2.0 ** -24, atol=0.0)
    y = torch.full_like(d.x, 7.0)
    assert fwd("csmpn_mvlayernorm_forward_det", d.x, d.params[0], 0, d.C, y) == 0 and bool((y == 7.0).all())
    wide = Direct(pkg, "mvlayernorm", C=257, rows=5)
    y = torch.full_like(wide.x, 7.0)
    assert fwd("csmpn_mvlayernorm_forward_det", wide.x, wide.params[0], 5, 257, y) == d.native.ERR_INVALID
    assert bool((y == 7.0).all())


# ------------------------------------------------------------------------------------------------- another process
@functools.lru_cache(maxsize=None)
def child_digests():
    """The digests tests/small_layers_det_helpers.py prints in ONE fresh process (all of CHILD_CASES)."""
    here = os.path.dirname(os.path.abspath(__file__))
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable, *flags, os.path.join(here, "small_layers_det_helpers.py")], capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return {l.split()[1]: l.split()[2] for l in out.stdout.splitlines() if l.startswith("digest ")}


@pytest.mark.parametrize("layer,name,C,rows", CHILD_CASES)
def test_same_bits_in_a_fresh_process(pkg, layer, name, C, rows):
    case = _case(pkg, layer, name, C, rows)
    assert digest(run_on_device(case, True)) == child_digests()[layer]


# ------------------------------------------------------------------------------------------------- the flag users set
def test_block_of_standalone_modules_under_the_torch_flag_alone(pkg):
    """MVLinear -> MVSiLU -> SteerableGeometricProductLayer -> MVLayerNorm built from the layer classes, with nothing set
    but torch.use_deterministic_algorithms(True) (what the reference's seeding does): forward + backward twice, the same
    bits, no warning, and the _det entry points ran."""
    from csmpn.models import cegnn_utils as cu
    from csmpn_hip import ops
    assert ops._DETERMINISTIC is None and not os.environ.get("CSMPN_DETERMINISTIC")
    torch.manual_seed(99)
    alg = pkg.CliffordAlgebra(METRICS["cl30"])
    block = torch.nn.Sequential(cu.MVLinear(alg, 12, 16), cu.MVSiLU(alg, 16), cu.SteerableGeometricProductLayer(alg, 16),
                                cu.MVLayerNorm(alg, 16)).to(dev())
    x, gout = torch.randn(300, 12, 8, device=dev()), torch.randn(300, 16, 8, device=dev())
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    before = ops.det_launches()
    try:
        torch.use_deterministic_algorithms(True)
        assert ops.deterministic_request() == "soft"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            a = run_module(block, x, gout)
            b = run_module(block, x, gout)
            torch.cuda.synchronize()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
        ops.set_deterministic(None)
    assert not caught, [str(w.message) for w in caught]
    # per pass: three MVLinear backwards, MVSiLU, the normalisation, the weighted product, MVLayerNorm forward + backward
    assert ops.det_launches() - before == 2 * 8
    assert len(a) == len(b) == 2 + len(list(block.parameters()))
    for u, v in zip(a, b):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
