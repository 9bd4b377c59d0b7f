"""torch.autograd Functions over the C-ABI (include/csmpn_hip.h).

PyTorch is plumbing here: it owns device memory and streams and records the
autograd graph; every forward and backward of the path runs in the HIP library.
There is no eager fallback: CPU tensors or a missing library raise.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from typing import List, Optional, Sequence

import torch

from . import native
from .native import BlockGrads, BlockParams, PARAM_FIELDS, check

NP = len(PARAM_FIELDS)  # parameter slots per CEMLP block


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _on_device_of(arg_index):
    """Decorator: run the function with the device of its `arg_index`-th argument current (kernel
    attributes, launches and the stream belong to that device; the caller's current device may be
    another one)."""
    import functools

    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*args, **kwargs):
            t = args[arg_index]
            if isinstance(t, torch.Tensor) and t.is_cuda:
                with torch.cuda.device(t.device):
                    return fn(*args, **kwargs)
            return fn(*args, **kwargs)
        return wrapped
    return deco


def _require_device(t: torch.Tensor, what: str, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(
            f"{what} is on {t.device}: the csmpn HIP path runs on MI355X only and has no CPU fallback "
            f"(the CPU restatement lives in oracle/ and is test infrastructure)."
        )
    if t.dtype != dtype:
        raise RuntimeError(f"{what} must be {str(dtype).replace('torch.', '')}, got {t.dtype}")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


_FUSED_GRAD_ACCUM = False


def set_fused_grad_accumulation(flag: bool):
    """Opt-in: parameter gradients are added by the kernels straight into the existing `p.grad` tensors (the kernels
    accumulate anyway) and the autograd functions return None for the parameters, instead of handing views of a flat
    buffer to autograd's AccumulateGrad - one elementwise kernel per parameter tensor less (the convex-hulls model has
    ~150 of them per step). Needs `optimizer.zero_grad(set_to_none=False)`; falls back to the flat buffer whenever a
    parameter has no (contiguous float32, same-device) .grad yet. Parameter hooks (e.g. DistributedDataParallel's) do
    not see gradients delivered this way: leave it off under DDP."""
    global _FUSED_GRAD_ACCUM
    _FUSED_GRAD_ACCUM = bool(flag)


def _fusable(params, device) -> bool:
    if not _FUSED_GRAD_ACCUM:
        return False
    for p in params:
        if p is None:
            continue
        g = p.grad
        if g is None or not p.requires_grad or g.dtype != torch.float32 or g.device != device or not g.is_contiguous() \
                or g.shape != p.shape:
            return False
    return True


class CemlpBinding:
    """ctypes view of one CEMLP's parameters, cached across calls.

    `specs` is a list (one per block) of dicts with in_features, out_features,
    lin_subspaces. Parameters arrive per call as a flat list of NP tensors per
    block in PARAM_FIELDS order (None for an absent MVLinear bias).
    """

    def __init__(self, metric: Sequence[float], specs: List[dict]):
        self.metric = tuple(float(m) for m in metric)
        self.n = len(self.metric)
        self.D = 1 << self.n
        self.metric_arr = native.metric_array(self.metric)
        self.nblk = len(specs)
        if not 1 <= self.nblk <= native.MAX_BLOCKS:
            raise native.CsmpnError(f"CEMLP with {self.nblk} blocks not supported (1..{native.MAX_BLOCKS})")
        self.params = (BlockParams * self.nblk)()
        self.grads = (BlockGrads * self.nblk)()
        for k, s in enumerate(specs):
            self.params[k].in_features = int(s["in_features"])
            self.params[k].out_features = int(s["out_features"])
            self.params[k].lin_subspaces = 1 if s.get("lin_subspaces", True) else 0
        self.in_features = int(specs[0]["in_features"])
        self.out_features = int(specs[-1]["out_features"])
        self._key = None
        self._grad_layout = None
        self._ws_bytes = None
        self._saved_per_row = None
        self._sig_only = None

    def supported(self) -> bool:
        return bool(native.lib().csmpn_metric_supported(self.metric_arr, self.n))

    def sig_only(self) -> bool:
        """A signature the device serves through the run-time-signature kernels alone: not one of the six compiled algebras,
        but n in 2..5 and every entry +1 or -1 (csmpn_signature_supported)."""
        if self._sig_only is None:
            self._sig_only = (not self.supported()) and bool(native.lib().csmpn_signature_supported(self.metric_arr, self.n))
        return self._sig_only

    def bind(self, params: Sequence[Optional[torch.Tensor]]):
        assert len(params) == NP * self.nblk
        key = tuple(_ptr(p) for p in params)
        if key != self._key:
            for k in range(self.nblk):
                blk = self.params[k]
                for j, name in enumerate(PARAM_FIELDS):
                    p = params[k * NP + j]
                    if p is not None and not p.is_contiguous():
                        raise RuntimeError(f"parameter {name} of block {k} must be contiguous")
                    setattr(blk, name, key[k * NP + j])
            self._key = key
            self._grad_layout = None
        if self._ws_bytes is None:
            self._ws_bytes = int(native.lib().csmpn_cemlp_workspace_bytes(self.n, self.params, self.nblk))

    def new_saved(self, rows: int, device, save_state: bool = False) -> Optional[torch.Tensor]:
        """Buffer for the inputs of blocks 1.. (written by forward, read by backward). save_state: the forward / backward pair
        will be called with CSMPN_FLAG_SAVE_STATE - the buffer also holds the state regions (3-4x the block inputs on the
        D = 32 and 32-channel shapes)."""
        if self._saved_per_row is None:
            self._saved_per_row = int(native.lib().csmpn_cemlp_saved_floats_per_row(self.n, self.params, self.nblk))
        if self._saved_per_row == 0 or rows == 0:
            return None
        # the size of THIS launch: regions a launch of `rows` rows never touches are left out (csmpn_cemlp_saved_floats)
        return torch.empty(int(native.lib().csmpn_cemlp_saved_floats(self.n, self.params, self.nblk, rows,
                                                                     native.FLAG_SAVE_STATE if save_state else 0)),
                           dtype=torch.float32, device=device)

    def workspace(self, device) -> torch.Tensor:
        return torch.empty(max(self._ws_bytes, 16), dtype=torch.uint8, device=device)

    def grad_floats(self, params: Sequence[Optional[torch.Tensor]]) -> int:
        """Floats of the flat gradient buffer new_grads() lays out for these parameters."""
        self._layout(params)
        return max(self._grad_layout[1], 1)

    def _layout(self, params):
        if self._grad_layout is None:
            offs, total = [], 0
            for p in params:
                if p is None:
                    offs.append(None)
                else:
                    offs.append((total, p.numel(), tuple(p.shape)))
                    total += (p.numel() + 3) // 4 * 4
            self._grad_layout = (offs, total)

    def new_grads(self, params: Sequence[Optional[torch.Tensor]], device, flat=None, fused_into=None, dtype=torch.float32):
        """One zeroed flat buffer for all parameter gradients (a single memset; or the caller's
        already zeroed `flat` of grad_floats() elements); returns (flat, views) with views[i]
        shaped like params[i]."""
        self._layout(params)
        offs, total = self._grad_layout
        if fused_into is not None:
            # the kernels add into the parameters' own .grad tensors; nothing for autograd to accumulate
            for k in range(self.nblk):
                g = self.grads[k]
                for j, name in enumerate(PARAM_FIELDS):
                    p = fused_into[k * NP + j]
                    setattr(g, name, None if p is None else p.grad.data_ptr())
            return None, [None] * len(params)
        if flat is None:
            flat = torch.zeros(max(total, 1), dtype=dtype, device=device)
        base, itemsize = flat.data_ptr(), flat.element_size()
        views = []
        for k in range(self.nblk):
            g = self.grads[k]
            for j, name in enumerate(PARAM_FIELDS):
                o = offs[k * NP + j]
                if o is None:
                    setattr(g, name, None)
                    views.append(None)
                else:
                    setattr(g, name, base + itemsize * o[0])
                    views.append(flat[o[0]:o[0] + o[1]].view(o[2]))
        return flat, views


# --------------------------------------------------------------------------------- CEMLP


class _CemlpFn(torch.autograd.Function):
    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, binding: CemlpBinding, *params):
        _require_device(x, "CEMLP input")
        if x.dim() != 3 or x.shape[1] != binding.in_features or x.shape[2] != binding.D:
            raise RuntimeError(f"CEMLP input must be [rows, {binding.in_features}, {binding.D}], got {tuple(x.shape)}")
        x = x.contiguous()
        binding.bind(params)
        rows = x.shape[0]
        y = torch.empty(rows, binding.out_features, binding.D, dtype=torch.float32, device=x.device)
        ws = binding.workspace(x.device)
        # CSMPN_FLAG_SAVE_STATE: the library honours it for the standalone shapes whose saved buffer has state regions (the
        # 32-channel Cl(3,0) CEMLPs of the md17 model: csmpn_cemlp_saved_floats sizes them) and ignores it everywhere else
        # (asked for only where the standalone entry points honour it: other shapes would get state regions sized and never used)
        want_state = _SAVE_STATE and binding.n == 3 and binding.out_features == 32
        saved = binding.new_saved(rows, x.device, want_state) if any(ctx.needs_input_grad) else None
        ctx.flags = native.FLAG_SAVE_STATE if (want_state and saved is not None) else 0

        def call(flags):
            return native.lib().csmpn_cemlp_forward(binding.metric_arr, binding.n, binding.params, binding.nblk,
                                                    x.data_ptr(), rows, y.data_ptr(), _ptr(saved), ws.data_ptr(),
                                                    ws.numel(), flags, _stream(x.device))

        _det_call(call, ctx.flags)
        ctx.binding = binding
        ctx.param_refs = params          # the caller's parameter objects (their .grad, for fused accumulation)
        ctx.ws, ctx.saved = ws, saved   # packed weights / block inputs are reused by backward
        ctx.save_for_backward(x, *[p for p in params if p is not None])
        ctx.mask = [p is not None for p in params]
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        binding = ctx.binding
        x, *present = ctx.saved_tensors
        it = iter(present)
        params = [next(it) if m else None for m in ctx.mask]
        gy = gy.contiguous()
        binding.bind(params)
        fused = ctx.param_refs if _fusable(ctx.param_refs, x.device) else None
        flat, views = binding.new_grads(params, x.device, fused_into=fused)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ws = ctx.ws

        def call(flags):
            return native.lib().csmpn_cemlp_backward(binding.metric_arr, binding.n, binding.params, binding.grads,
                                                     binding.nblk, x.data_ptr(), gy.data_ptr(), x.shape[0], _ptr(gx),
                                                     _ptr(ctx.saved), ws.data_ptr(), ws.numel(), flags, _stream(x.device))

        _det_call(call, native.FLAG_WEIGHTS_PACKED | ctx.flags)
        return (gx, None, *views)


# ---------------------------------------------- float64 (csrc/cemlp_f64.hpp) and run-time signature (csrc/cemlp_sig.hpp)
# CEMLP and EGCL on float64 device tensors, and on float32 device tensors of a signature that is not one of the six compiled
# algebras: autograd functions of their own over the csmpn_*_f64 / csmpn_*_sig entry points (_RowFamily). The workspace
# comes from the query per call, nothing is saved but the inputs (the backward recomputes), the sums run in a fixed order:
# bit-reproducible whatever set_deterministic says. Out of scope here: fused gradient accumulation, the captured step.


def _on_device_like(x, others):
    """Every attribute tensor on the device of the input: the check and the message of the float32 path (_require_device),
    in front of any launch - a host pointer must never reach a kernel."""
    for name, t in others:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                f"{name} is on {t.device}: the csmpn HIP path runs on MI355X only and has no CPU fallback "
                f"(the CPU restatement lives in oracle/ and is test infrastructure).")
        if t.device != x.device:
            raise RuntimeError(f"{name} is on {t.device}, the input on {x.device}: one device per call")


def _same_dtype(x, others, what):
    """One dtype for the input, every parameter and the attributes of a fused module (no launch otherwise)."""
    for name, t in others:
        if t is not None and t.dtype != x.dtype:
            raise RuntimeError(f"{what}: mixed dtypes - the input is {x.dtype}, {name} is {t.dtype} (cast the module with "
                               f".double() / .float() or the tensors to match)")


class _RowFamily:
    """The entry points of one dtype that _CemlpF64Fn / _EgclF64Fn call: float64 -> csmpn_*_f64 (csrc/cemlp_f64.hpp, and
    cemlp_sig.hpp behind them for the signatures that are not compiled), float32 -> csmpn_*_sig (csrc/cemlp_sig.hpp). Same
    argument lists, same call sequence, same contracts."""

    def __init__(self, dtype, suffix, ws_query, what, kernels):
        self.dtype, self.suffix, self.ws_query, self.what, self.kernels = dtype, suffix, ws_query, what, kernels

    def fn(self, stem):
        return getattr(native.lib(), stem + self.suffix)

    def check_widths(self, binding: CemlpBinding):
        for k in range(binding.nblk):
            if binding.params[k].out_features > native.F64_MAX_WIDTH:
                raise native.CsmpnError(f"{self.what} CEMLP / EGCL: out_features {binding.params[k].out_features} of block {k} is above "
                                        f"the limit of {native.F64_MAX_WIDTH} channels of the {self.kernels} kernels")

    def ws(self, binding: CemlpBinding, rows: int, device) -> torch.Tensor:
        nbytes = int(getattr(native.lib(), self.ws_query)(binding.n, binding.params, binding.nblk, rows))
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)

    def segment_reduce(self, rows, out, add=None, sub=None, accumulate=True):
        return (segment_reduce_f64 if self.dtype == torch.float64 else segment_reduce)(rows, out, add, sub, accumulate)


_FAMILY = {torch.float64: _RowFamily(torch.float64, "_f64", "csmpn_cemlp_f64_workspace_bytes", "float64", "float64"),
           torch.float32: _RowFamily(torch.float32, "_sig", "csmpn_cemlp_sig_workspace_bytes", "run-time-signature",
                                     "run-time-signature")}


def _family_of(t: torch.Tensor, what: str) -> _RowFamily:
    if not t.is_cuda:
        _require_device(t, what)
    if t.dtype not in _FAMILY:
        raise RuntimeError(f"{what} must be float32 or float64, got {t.dtype}")
    return _FAMILY[t.dtype]


def segment_reduce_f64(rows, out, add=None, sub=None, accumulate=True):
    """segment_reduce on float64 tables."""
    ap, ao = add if add is not None else (None, None)
    sp, so = sub if sub is not None else (None, None)
    check(native.lib().csmpn_segment_reduce_f64(rows.data_ptr(), rows[0].numel(), out.shape[0], _ptr(ap), _ptr(ao), _ptr(sp),
                                                _ptr(so), out.data_ptr(), 1 if accumulate else 0, _stream(out.device)))
    return out


class _CemlpF64Fn(torch.autograd.Function):
    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, binding: CemlpBinding, *params):
        fam = _family_of(x, "CEMLP input")
        _on_device_like(x, [(f"parameter {j}", p) for j, p in enumerate(params)])
        if x.dim() != 3 or x.shape[1] != binding.in_features or x.shape[2] != binding.D:
            raise RuntimeError(f"CEMLP input must be [rows, {binding.in_features}, {binding.D}], got {tuple(x.shape)}")
        fam.check_widths(binding)
        x = x.contiguous()
        binding.bind(params)
        rows = x.shape[0]
        y = torch.empty(rows, binding.out_features, binding.D, dtype=fam.dtype, device=x.device)
        ws = fam.ws(binding, rows, x.device)
        check(fam.fn("csmpn_cemlp_forward")(binding.metric_arr, binding.n, binding.params, binding.nblk, x.data_ptr(), rows,
                                                   y.data_ptr(), ws.data_ptr(), ws.numel(), _stream(x.device)))
        ctx.binding = binding
        ctx.save_for_backward(x, *[p for p in params if p is not None])
        ctx.mask = [p is not None for p in params]
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        binding = ctx.binding
        x, *present = ctx.saved_tensors
        fam = _FAMILY[x.dtype]
        it = iter(present)
        params = [next(it) if m else None for m in ctx.mask]
        gy = gy.contiguous()
        binding.bind(params)
        _flat, views = binding.new_grads(params, x.device, dtype=fam.dtype)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ws = fam.ws(binding, x.shape[0], x.device)
        check(fam.fn("csmpn_cemlp_backward")(binding.metric_arr, binding.n, binding.params, binding.grads, binding.nblk,
                                                    x.data_ptr(), gy.data_ptr(), x.shape[0], _ptr(gx), ws.data_ptr(), ws.numel(),
                                                    _stream(x.device)))
        return (gx, None, *views)


class _EgclF64Fn(torch.autograd.Function):
    """The deterministic call sequence of HipBackend on the float64 entry points: edge rows -> fixed-order segment sum ->
    node stage; backward: node stage, edge rows, segment sum (+ by target, - by source order)."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, h, edge_attr, node_attr, spec: EgclSpec, csr: Csr, *params):
        fam = _family_of(h, "EGCL input h")
        _on_device_like(h, [("edge_attr", edge_attr), ("node_attr", node_attr)]
                        + [(f"parameter {j}", p) for j, p in enumerate(params)])
        _check_egcl_inputs(spec, csr, h, edge_attr, node_attr, csr.n_edges)
        if not isinstance(csr, Csr):
            raise native.CsmpnError(f"{fam.what} EGCL needs the whole adjacency (no sliced launches)")
        e, nd = spec.edge, spec.node
        fam.check_widths(e)
        fam.check_widths(nd)
        h = h.contiguous()
        edge_attr = edge_attr.contiguous() if edge_attr is not None else None
        node_attr = node_attr.contiguous() if node_attr is not None else None
        ne = e.nblk * NP
        pe, pn = params[:ne], params[ne:]
        e.bind(pe)
        nd.bind(pn)
        N, E, D, dev, lib = h.shape[0], csr.n_edges, e.D, h.device, native.lib()
        f64 = dict(dtype=fam.dtype, device=dev)
        agg = torch.zeros(N, spec.O, D, **f64)
        if E > 0:
            rows = torch.empty(E, spec.O, D, **f64)
            ws = fam.ws(e, E, dev)
            check(fam.fn("csmpn_egcl_edge_forward")(e.metric_arr, e.n, e.params, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr), spec.A,
                                                  csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), E, N, rows.data_ptr(),
                                                  ws.data_ptr(), ws.numel(), _stream(dev)))
            fam.segment_reduce(rows, agg, add=(csr.row_ptr, None), accumulate=False)
        out = torch.empty(N, nd.out_features, D, **f64)
        ws = fam.ws(nd, N, dev)
        check(fam.fn("csmpn_egcl_node_forward")(nd.metric_arr, nd.n, nd.params, nd.nblk, h.data_ptr(), spec.C, agg.data_ptr(), spec.O,
                                              _ptr(node_attr), spec.T, csr.deg.data_ptr(), spec.mean, spec.residual, N, out.data_ptr(),
                                              ws.data_ptr(), ws.numel(), _stream(dev)))
        ctx.spec, ctx.csr = spec, csr
        ctx.has_ea, ctx.has_na = edge_attr is not None, node_attr is not None
        ctx.mask = [p is not None for p in params]
        saved = [h, agg] + ([edge_attr] if ctx.has_ea else []) + ([node_attr] if ctx.has_na else [])
        ctx.save_for_backward(*saved, *[p for p in params if p is not None])
        return out

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gout):
        spec, csr = ctx.spec, ctx.csr
        saved = list(ctx.saved_tensors)
        h, agg = saved[0], saved[1]
        fam = _FAMILY[h.dtype]
        pos = 2
        edge_attr = node_attr = None
        if ctx.has_ea:
            edge_attr = saved[pos]; pos += 1
        if ctx.has_na:
            node_attr = saved[pos]; pos += 1
        it = iter(saved[pos:])
        params = [next(it) if m else None for m in ctx.mask]
        e, nd = spec.edge, spec.node
        ne = e.nblk * NP
        pe, pn = params[:ne], params[ne:]
        e.bind(pe)
        nd.bind(pn)
        gout = gout.contiguous()
        N, E, D, dev, lib = h.shape[0], csr.n_edges, e.D, h.device, native.lib()
        f64 = dict(dtype=fam.dtype, device=dev)
        _fn, views_n = nd.new_grads(pn, dev, dtype=fam.dtype)
        gh = torch.empty_like(h)
        g_agg = torch.empty(N, spec.O, D, **f64)
        g_na = torch.empty_like(node_attr) if (node_attr is not None and ctx.needs_input_grad[2]) else None
        ws = fam.ws(nd, N, dev)
        check(fam.fn("csmpn_egcl_node_backward")(nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, h.data_ptr(), spec.C, agg.data_ptr(),
                                               spec.O, _ptr(node_attr), spec.T, csr.deg.data_ptr(), spec.mean, spec.residual, N,
                                               gout.data_ptr(), gh.data_ptr(), g_agg.data_ptr(), _ptr(g_na), ws.data_ptr(), ws.numel(),
                                               _stream(dev)))
        _fe, views_e = e.new_grads(pe, dev, dtype=fam.dtype)
        g_ea = torch.empty_like(edge_attr) if (edge_attr is not None and ctx.needs_input_grad[1]) else None
        if E > 0:
            rows = torch.empty(E, spec.C, D, **f64)
            ws = fam.ws(e, E, dev)
            check(fam.fn("csmpn_egcl_edge_backward")(e.metric_arr, e.n, e.params, e.grads, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr),
                                                   spec.A, csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), E, N,
                                                   g_agg.data_ptr(), rows.data_ptr(), _ptr(g_ea), ws.data_ptr(), ws.numel(),
                                                   _stream(dev)))
            fam.segment_reduce(rows, gh, add=(csr.row_ptr, None), sub=csr.source_order())
        return (gh, g_ea, g_na, None, None, *views_e, *views_n)


def cemlp_apply(x, binding: CemlpBinding, params):
    if x.is_cuda:   # (a CPU tensor: _CemlpFn raises "no CPU fallback", first of all)
        _same_dtype(x, ((f"parameter {PARAM_FIELDS[j % NP]} of block {j // NP}", p) for j, p in enumerate(params)), "CEMLP")
        if x.dtype == torch.float64 or (x.dtype == torch.float32 and binding.sig_only()):
            return _CemlpF64Fn.apply(x, binding, *params)
    return _CemlpFn.apply(x, binding, *params)


_EMBED_LAUNCHES = 0


def embed_launches() -> int:
    """Forward launches of the fused embedding entry point so far (tests assert that the HIP path ran)."""
    return _EMBED_LAUNCHES


class _EmbedCemlpFn(torch.autograd.Function):
    """Fused simplex embedding (csmpn_embed_cemlp_*; hulls_cssmpnn.py:96-125): vertex features gathered in every vertex
    order -> CEMLP -> sum over the orders, without the [n_simplices * (d+1)!, ., D] input / output rows in memory.
    vertex_feat [S, K, D] (data: no gradient), verts [n_simplices * n_orders, d+1] int32."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, vertex_feat, verts, n_orders, validated, binding: CemlpBinding, *params):
        _require_device(vertex_feat, "embedding vertex features")
        binding.bind(params)
        rows = int(verts.shape[0])
        out = torch.empty(rows // n_orders, binding.out_features, binding.D, dtype=torch.float32, device=vertex_feat.device)
        ws = binding.workspace(vertex_feat.device)
        need_grad = any(ctx.needs_input_grad[5:])
        saved = binding.new_saved(rows, vertex_feat.device, _SAVE_STATE and binding.nblk > 1) if need_grad else None
        # the layer's own saved buffer, sized for exactly these rows: CSMPN_FLAG_SAVE_STATE (two-block modules: y, R, s)
        st_flag = native.FLAG_SAVE_STATE if (_SAVE_STATE and saved is not None and binding.nblk > 1) else 0
        # validated: the caller has range-checked verts against vertex_feat's rows once (the batch plan); otherwise the entry
        # point does, with one host round trip (not capturable)
        st_flag |= native.FLAG_NO_VALIDATE if validated else 0
        # no CSMPN_FLAG_DETERMINISTIC here, whatever deterministic_request() says: nothing in the wide parity-lane kernels'
        # MODE_PLAIN depends on the order of arrival (include/csmpn_hip.h at the flag), the entry points take no such flag
        check(native.lib().csmpn_embed_cemlp_forward(
            binding.metric_arr, binding.n, binding.params, binding.nblk, vertex_feat.data_ptr(), int(vertex_feat.shape[0]),
            int(vertex_feat.shape[1]),
            verts.data_ptr(), int(verts.shape[1]), int(n_orders), rows, out.data_ptr(), _ptr(saved), ws.data_ptr(), ws.numel(),
            st_flag, _stream(vertex_feat.device)))
        ctx.st_flag = st_flag
        global _EMBED_LAUNCHES
        _EMBED_LAUNCHES += 1
        ctx.binding, ctx.param_refs, ctx.ws, ctx.saved, ctx.n_orders = binding, params, ws, saved, int(n_orders)
        ctx.save_for_backward(vertex_feat, verts, *[p for p in params if p is not None])
        ctx.mask = [p is not None for p in params]
        return out

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gout):
        binding = ctx.binding
        vertex_feat, verts, *present = ctx.saved_tensors
        it = iter(present)
        params = [next(it) if m else None for m in ctx.mask]
        gout = gout.contiguous()
        binding.bind(params)
        fused = ctx.param_refs if _fusable(ctx.param_refs, vertex_feat.device) else None
        _flat, views = binding.new_grads(params, vertex_feat.device, fused_into=fused)
        check(native.lib().csmpn_embed_cemlp_backward(
            binding.metric_arr, binding.n, binding.params, binding.grads, binding.nblk, vertex_feat.data_ptr(),
            int(vertex_feat.shape[0]), int(vertex_feat.shape[1]), verts.data_ptr(), int(verts.shape[1]), ctx.n_orders,
            int(verts.shape[0]), gout.data_ptr(), _ptr(ctx.saved), ctx.ws.data_ptr(), ctx.ws.numel(),
            ctx.st_flag | native.FLAG_NO_VALIDATE,     # the forward has checked (or the caller vouched for) this table
            _stream(vertex_feat.device)))
        return (None, None, None, None, None, *views)


def embed_cemlp_supported(binding: CemlpBinding, verts_per_row: int, channels_per_vertex: int) -> bool:
    """Shapes the fused embedding serves - the two MODE_PLAIN programs of the wide parity-lane kernels (csrc/plw_inst.inc):
    Cl(5,0) / Cl(4,1), 28 output channels, 2 input channels in one block or 3 in two blocks. Everything else composes
    simplex_rows + CEMLP + sum (csmpn_embed_cemlp_forward returns CSMPN_ERR_UNSUPPORTED there)."""
    return (binding.n == 5 and binding.out_features == 28 and (binding.in_features, binding.nblk) in ((2, 1), (3, 2))
            and all(int(binding.params[k].out_features) == 28 for k in range(binding.nblk))
            and verts_per_row * channels_per_vertex == binding.in_features)


def embed_cemlp_apply(vertex_feat, verts_i32, n_orders, binding: CemlpBinding, params, validated=False):
    """validated=True: every entry of verts_i32 is known to lie in [0, vertex_feat.shape[0]) (checked once per batch by the
    caller); False: the C-ABI checks on every forward (one synchronous round trip)."""
    return _EmbedCemlpFn.apply(vertex_feat, verts_i32, n_orders, bool(validated), binding, *params)


# --------------------------------------------------------------------------------- CSR


_DETERMINISTIC = None   # None: follow CSMPN_DETERMINISTIC, else torch.are_deterministic_algorithms_enabled()
_warned_soft_det = False


def set_deterministic(flag):
    """True / False: force the atomic-free aggregation on / off; None: follow the environment
    (CSMPN_DETERMINISTIC=0|1) and otherwise torch.use_deterministic_algorithms, which the reference
    switches on (engineer/utils/seed.py:30). The request reaches the EGCL stages, standalone CEMLPs, the standalone
    MVLinear backward, the type-attribute backward (everything a step of the four task models runs) and the four
    standalone small layers (mvsilu / mvnorm / mvlayernorm / wgp _apply: the csmpn_*_det entry points, which serve every
    shape the default forms serve - no fallback, hard and soft requests alike). Nothing the modules launch ignores it."""
    global _DETERMINISTIC
    _DETERMINISTIC = None if flag is None else bool(flag)


def deterministic_request():
    """'hard' (explicitly requested: unsupported shapes raise), 'soft' (inherited from
    torch.use_deterministic_algorithms: unsupported shapes warn once and use float atomics) or None."""
    if _DETERMINISTIC is not None:
        return "hard" if _DETERMINISTIC else None
    env = os.environ.get("CSMPN_DETERMINISTIC")
    if env is not None and env != "":
        return "hard" if env != "0" else None
    return "soft" if torch.are_deterministic_algorithms_enabled() else None


def _soft_fallback(rc):
    """An unsupported shape under a 'soft' request: warn once, tell the caller to take the atomic path."""
    global _warned_soft_det
    if rc != native.ERR_UNSUPPORTED:
        return False
    if not _warned_soft_det:
        _warned_soft_det = True
        warnings.warn("csmpn_hip: deterministic aggregation is not available for this layer shape "
                      f"({native.lib().csmpn_last_error().decode()}); using float atomics")
    return True


def _det_call(call, flags):
    """call(flags) of an entry point that accepts CSMPN_FLAG_DETERMINISTIC, under deterministic_request(): a hard request
    raises on a shape without deterministic kernels, a soft one repeats the call without the flag (as the EGCL stages);
    no request: exactly call(flags)."""
    det = deterministic_request()
    rc = call(flags | (native.FLAG_DETERMINISTIC if det else 0))
    if det == "soft" and _soft_fallback(rc):
        rc = call(flags)
    check(rc)


_DET_LAUNCHES = 0


def det_launches() -> int:
    """Calls of the _det entry points so far: csmpn_mvlinear_backward_det, csmpn_type_attr_backward_det and the small
    layers' csmpn_mvsilu_backward_det, csmpn_mvnorm_backward_det, csmpn_mvlayernorm_forward_det / _backward_det and
    csmpn_wgp_backward_det (tests assert that the deterministic forms ran)."""
    return _DET_LAUNCHES


def _count_det():
    global _DET_LAUNCHES
    _DET_LAUNCHES += 1


def _det_scratch(nbytes, device):
    """Scratch for ONE call of a _det entry point (sized by its _bytes query; needs no initialisation); counts the call."""
    _count_det()
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _small_det_scratch(op, metric, x):
    """_det_scratch for the backward of a standalone small layer on x [rows, C, D]."""
    return _det_scratch(native.lib().csmpn_small_layer_det_bytes(op, len(metric), x.shape[0], x.shape[1]), x.device)


def _warn_soft_slice():
    global _warned_soft_det
    if not _warned_soft_det:
        _warned_soft_det = True
        warnings.warn("csmpn_hip: torch.use_deterministic_algorithms(True) is set, but this launch covers a slice of "
                      "the adjacency (graph-segment step): using float atomics (ops.set_deterministic(True) makes "
                      "this an error)")


def segment_reduce(rows, out, add=None, sub=None, accumulate=True):
    """out[v] (+)= sum rows[add segment of v] - sum rows[sub segment of v] in a fixed order.
    add / sub: (row_ptr, order or None) int32 device tensors."""
    ap, ao = add if add is not None else (None, None)
    sp, so = sub if sub is not None else (None, None)
    check(native.lib().csmpn_segment_reduce(rows.data_ptr(), rows[0].numel(), out.shape[0], _ptr(ap), _ptr(ao),
                                            _ptr(sp), _ptr(so), out.data_ptr(), 1 if accumulate else 0,
                                            _stream(out.device)))
    return out


class Csr:
    """Target-sorted adjacency of one complex (built once, reused by every layer and step)."""

    __slots__ = ("perm", "src", "dst", "deg", "row_ptr", "n_edges", "n_nodes", "build_ms", "_src_order", "_ws")

    def source_order(self):
        """(row_ptr_src, order): the sorted edge positions grouped by source (deterministic mode)."""
        if self._src_order is None:
            dev = self.src.device
            order = torch.empty(max(self.n_edges, 1), dtype=torch.int32, device=dev)
            rp = torch.empty(self.n_nodes + 1, dtype=torch.int32, device=dev)
            ws = torch.empty(int(native.lib().csmpn_csr_workspace_bytes(self.n_edges, self.n_nodes)),
                             dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev):
                check(native.lib().csmpn_csr_source_order(self.src.data_ptr(), self.n_edges, self.n_nodes,
                                                          order.data_ptr(), rp.data_ptr(), ws.data_ptr(), ws.numel(),
                                                          _stream(dev)))
            self._src_order = (rp, order)
        return self._src_order

    def __init__(self, edge_index: torch.Tensor, n_nodes: int):
        if not edge_index.is_cuda:
            raise RuntimeError("edge_index must live on the GPU (no CPU fallback)")
        if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
            raise RuntimeError("edge_index must be int64 [2, E]")
        ei = edge_index.contiguous()
        dev = ei.device
        E = ei.shape[1]
        i32 = dict(dtype=torch.int32, device=dev)
        self.n_edges, self.n_nodes = E, n_nodes
        self._src_order = None
        self._ws = None
        self.perm = torch.empty(max(E, 1), **i32)
        self.src = torch.empty(max(E, 1), **i32)
        self.dst = torch.empty(max(E, 1), **i32)
        self.deg = torch.empty(n_nodes, **i32)
        self.row_ptr = torch.empty(n_nodes + 1, **i32)
        ws = torch.empty(int(native.lib().csmpn_csr_workspace_bytes(E, n_nodes)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            # validates edge_index against [0, n_nodes) (raises CsmpnError); one host sync per complex
            check(native.lib().csmpn_csr_build(ei.data_ptr(), E, n_nodes, self.perm.data_ptr(), self.src.data_ptr(),
                                               self.dst.data_ptr(), self.deg.data_ptr(), self.row_ptr.data_ptr(),
                                               ws.data_ptr(), ws.numel(), 0, _stream(dev)))
            t1.record()
            t1.synchronize()
            self.build_ms = t0.elapsed_time(t1)


    def rebuild_(self, edge_index: torch.Tensor) -> "Csr":
        """The same five tensors - and the source order, if it exists - rebuilt IN PLACE for another adjacency of the same
        size (a batch of new topology under a captured step, csmpn_hip.graphed): same data_ptrs, no allocation after the
        first call (the workspace is kept from then on), no host synchronisation - the indices are NOT range-checked here
        (CSMPN_FLAG_NO_VALIDATE: the caller has validated them, csmpn.data.complexes.pad_batch; an entry outside
        [0, n_nodes) is mapped to node 0). Re-stamps the cache entry on `edge_index` (ops.get_csr) with its version."""
        if not edge_index.is_cuda or edge_index.device != self.src.device:
            raise RuntimeError("edge_index must live on the device of the CSR (no CPU fallback)")
        if edge_index.dtype != torch.int64 or tuple(edge_index.shape) != (2, self.n_edges) or not edge_index.is_contiguous():
            raise RuntimeError(f"Csr.rebuild_: edge_index must be contiguous int64 [2, {self.n_edges}] (the size it was built for)")
        dev = self.src.device
        lib = native.lib()
        if self._ws is None:
            self._ws = torch.empty(int(lib.csmpn_csr_workspace_bytes(self.n_edges, self.n_nodes)), dtype=torch.uint8, device=dev)
        ws = self._ws
        with torch.cuda.device(dev):
            check(lib.csmpn_csr_build(edge_index.data_ptr(), self.n_edges, self.n_nodes, self.perm.data_ptr(),
                                      self.src.data_ptr(), self.dst.data_ptr(), self.deg.data_ptr(), self.row_ptr.data_ptr(),
                                      ws.data_ptr(), ws.numel(), native.FLAG_NO_VALIDATE, _stream(dev)))
            if self._src_order is not None:
                rp, order = self._src_order
                check(lib.csmpn_csr_source_order(self.src.data_ptr(), self.n_edges, self.n_nodes, order.data_ptr(),
                                                 rp.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
        try:
            edge_index._csmpn_csr = (edge_index._version, self)
        except Exception:
            pass
        return self


class CsrSlice:
    """Rows [lo, hi) of a target-sorted adjacency (views; for launching the edge forward in pieces)."""

    __slots__ = ("perm", "src", "dst", "n_edges", "n_nodes")

    def __init__(self, csr: Csr, lo: int, hi: int):
        self.perm, self.src, self.dst = csr.perm[lo:hi], csr.src[lo:hi], csr.dst[lo:hi]
        self.n_edges, self.n_nodes = hi - lo, csr.n_nodes


def get_csr(edge_index: torch.Tensor, n_nodes: int) -> Csr:
    """CSR cached on the edge_index tensor object itself (complexes are static:
    every layer of a model and every epoch pass the same tensor)."""
    cached = getattr(edge_index, "_csmpn_csr", None)
    if cached is not None and cached[0] == edge_index._version and cached[1].n_nodes == n_nodes:
        return cached[1]
    csr = Csr(edge_index, n_nodes)
    try:
        edge_index._csmpn_csr = (edge_index._version, csr)
    except Exception:
        pass
    return csr


# --------------------------------------------------------------------------------- EGCL


class EgclSpec:
    """Static description of one EGCL layer for the autograd Function."""

    def __init__(self, edge: CemlpBinding, node: CemlpBinding, channels: int, out_channels: int,
                 edge_attr_channels: int, node_attr_channels: int, aggr: str, residual: bool):
        if aggr not in ("mean", "sum", "add"):
            raise native.CsmpnError(f"aggr={aggr!r} not supported by the HIP path (mean | sum | add)")
        self.edge, self.node = edge, node
        self.C, self.O = channels, out_channels
        self.A, self.T = edge_attr_channels, node_attr_channels
        self.mean = 1 if aggr == "mean" else 0
        self.residual = 1 if residual else 0


class HipBackend:
    """The four stages of one EGCL layer as C-ABI calls (device tensors in, device tensors out).
    The sharded layer (csmpn_hip.sharded) composes the same stages with collectives."""

    @staticmethod
    def build_csr(edge_index, n_nodes):
        return get_csr(edge_index, n_nodes)

    @staticmethod
    @_on_device_of(2)
    def edge_forward(spec, csr, h, edge_attr, pe, save=True, agg=None, saved=None):
        """Returns (agg, state); state = (workspace with packed weights, saved block inputs).
        agg: optional [N, O, D] buffer to accumulate into (zeroed by the caller); saved: optional
        buffer for the saved block inputs of these csr.n_edges rows."""
        e = spec.edge
        e.bind(pe)
        N, D = h.shape[0], e.D
        if agg is None:
            agg = torch.zeros(N, spec.O, D, dtype=torch.float32, device=h.device)
        ws = e.workspace(h.device)
        # CSMPN_FLAG_SAVE_STATE only for a buffer of our own, laid out for exactly these rows (a caller's buffer may be a
        # slice of a larger one: sharded split forward); the backward finds the flag on the tensor
        st_flag = 0
        if saved is None and save:
            saved = e.new_saved(csr.n_edges, h.device, _SAVE_STATE)
            if _SAVE_STATE and saved is not None:
                st_flag = native.FLAG_SAVE_STATE
                saved.csmpn_save_state = True
        det = deterministic_request()
        if det and not isinstance(csr, Csr):
            # a slice of the adjacency (graph-segment steps): only an explicit request is an error; the inherited
            # torch.use_deterministic_algorithms(True) of the reference's seeding warns once and keeps the atomics
            if det == "hard":
                raise native.CsmpnError("deterministic aggregation needs the whole adjacency (no sliced launches: "
                                        "set CSMPN_SPLIT_FWD=0)")
            _warn_soft_slice()
            det = None
        if det:
            rows = torch.empty(max(csr.n_edges, 1), spec.O, D, dtype=torch.float32, device=h.device)
            rc = native.lib().csmpn_egcl_edge_forward(
                e.metric_arr, e.n, e.params, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr), spec.A,
                csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), csr.n_edges, N, rows.data_ptr(),
                _ptr(saved), ws.data_ptr(), ws.numel(), native.FLAG_DETERMINISTIC | st_flag, _stream(h.device))
            if not (det == "soft" and _soft_fallback(rc)):
                check(rc)
                segment_reduce(rows, agg, add=(csr.row_ptr, None))
                return agg, (ws, saved)
        check(native.lib().csmpn_egcl_edge_forward(
            e.metric_arr, e.n, e.params, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr), spec.A,
            csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), csr.n_edges, N, agg.data_ptr(),
            _ptr(saved), ws.data_ptr(), ws.numel(), st_flag, _stream(h.device)))
        return agg, (ws, saved)

    @staticmethod
    @_on_device_of(2)
    def node_forward(spec, deg, h, agg, node_attr, pn, save=True):
        nd = spec.node
        nd.bind(pn)
        N, D = h.shape[0], nd.D
        out = torch.empty(N, nd.out_features, D, dtype=torch.float32, device=h.device)
        ws = nd.workspace(h.device)
        saved = nd.new_saved(N, h.device, _SAVE_STATE) if save else None
        st_flag = 0
        if _SAVE_STATE and saved is not None:
            st_flag = native.FLAG_SAVE_STATE
            saved.csmpn_save_state = True

        def call(flags):
            return native.lib().csmpn_egcl_node_forward(
                nd.metric_arr, nd.n, nd.params, nd.nblk, h.data_ptr(), spec.C, agg.data_ptr(), spec.O,
                _ptr(node_attr), spec.T, deg.data_ptr(), spec.mean, spec.residual, N, out.data_ptr(),
                _ptr(saved), ws.data_ptr(), ws.numel(), flags, _stream(h.device))

        det = deterministic_request()   # node stage: the flag only selects kernels with atomic-free parameter sums
        rc = call((native.FLAG_DETERMINISTIC if det else 0) | st_flag)
        if det == "soft" and _soft_fallback(rc):
            rc = call(st_flag)
        check(rc)
        return out, (ws, saved)

    @staticmethod
    @_on_device_of(2)
    def node_backward(spec, deg, h, agg, node_attr, pn, gout, want_gna, state=None, gflat=None, fused_into=None):
        """state: the workspace node_forward returned (its packed weights are reused);
        gflat: optional zeroed flat gradient buffer (CemlpBinding.grad_floats elements)."""
        nd = spec.node
        nd.bind(pn)
        N, D, dev = h.shape[0], nd.D, h.device
        _flat, views = nd.new_grads(pn, dev, gflat, fused_into=fused_into)
        gh = torch.empty_like(h)
        g_agg = torch.empty(N, spec.O, D, dtype=torch.float32, device=dev)
        g_na = torch.empty_like(node_attr) if (node_attr is not None and want_gna) else None
        ws, saved = state if state is not None else (nd.workspace(dev), None)
        flags = native.FLAG_WEIGHTS_PACKED if state is not None else 0
        if getattr(saved, "csmpn_save_state", False):
            flags |= native.FLAG_SAVE_STATE

        def call(fl):
            return native.lib().csmpn_egcl_node_backward(
                nd.metric_arr, nd.n, nd.params, nd.grads, nd.nblk, h.data_ptr(), spec.C, agg.data_ptr(), spec.O,
                _ptr(node_attr), spec.T, deg.data_ptr(), spec.mean, spec.residual, N, gout.data_ptr(),
                gh.data_ptr(), g_agg.data_ptr(), _ptr(g_na), _ptr(saved), ws.data_ptr(), ws.numel(), fl, _stream(dev))

        det = deterministic_request()
        rc = call(flags | (native.FLAG_DETERMINISTIC if det else 0))
        if det == "soft" and _soft_fallback(rc):
            rc = call(flags)
        check(rc)
        return gh, g_agg, g_na, views

    @staticmethod
    @_on_device_of(2)
    def edge_backward(spec, csr, h, edge_attr, pe, g_agg, gh, want_gea, state=None, gflat=None, fused_into=None):
        """gh is accumulated in place (+= scatter of +-d/d(h_i - h_j)); gflat as in node_backward."""
        e = spec.edge
        e.bind(pe)
        N, dev = h.shape[0], h.device
        _flat, views = e.new_grads(pe, dev, gflat, fused_into=fused_into)
        g_ea = torch.empty_like(edge_attr) if (edge_attr is not None and want_gea) else None
        ws, saved = state if state is not None else (e.workspace(dev), None)
        flags = native.FLAG_WEIGHTS_PACKED if state is not None else 0
        if getattr(saved, "csmpn_save_state", False):
            flags |= native.FLAG_SAVE_STATE
        det = deterministic_request()
        if det and not isinstance(csr, Csr):
            if det == "hard":
                raise native.CsmpnError("deterministic aggregation needs the whole adjacency (no sliced launches)")
            _warn_soft_slice()
            det = None
        if det:
            rows = torch.empty(max(csr.n_edges, 1), spec.C, e.D, dtype=torch.float32, device=dev)
            rc = native.lib().csmpn_egcl_edge_backward(
                e.metric_arr, e.n, e.params, e.grads, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr), spec.A,
                csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), csr.n_edges, N, g_agg.data_ptr(),
                rows.data_ptr(), _ptr(g_ea), _ptr(saved), ws.data_ptr(), ws.numel(),
                flags | native.FLAG_DETERMINISTIC, _stream(dev))
            if not (det == "soft" and _soft_fallback(rc)):
                check(rc)
                segment_reduce(rows, gh, add=(csr.row_ptr, None), sub=csr.source_order())
                return g_ea, views
        check(native.lib().csmpn_egcl_edge_backward(
            e.metric_arr, e.n, e.params, e.grads, e.nblk, h.data_ptr(), spec.C, _ptr(edge_attr), spec.A,
            csr.perm.data_ptr(), csr.src.data_ptr(), csr.dst.data_ptr(), csr.n_edges, N, g_agg.data_ptr(),
            gh.data_ptr(), _ptr(g_ea), _ptr(saved), ws.data_ptr(), ws.numel(), flags, _stream(dev)))
        return g_ea, views

    @staticmethod
    @_on_device_of(2)
    def layer_backward(spec, csr, h, agg, edge_attr, node_attr, pe, pn, gout, want_gea, want_gna, state_e=None, state_n=None,
                       gflat_e=None, gflat_n=None, fused_e=None, fused_n=None):
        """node_backward, then edge_backward, as ONE C-ABI call (csmpn_egcl_backward): same results, and the Cl(3,0)
        8-channel kernels sum both stages' gradient slices in one launch behind the edge stage. Whole adjacency, no
        deterministic request (the callers' business). Returns (gh, g_ea, g_na, views_e, views_n)."""
        e, nd = spec.edge, spec.node
        e.bind(pe)
        nd.bind(pn)
        N, D, dev = h.shape[0], nd.D, h.device
        _fe, views_e = e.new_grads(pe, dev, gflat_e, fused_into=fused_e)
        _fn, views_n = nd.new_grads(pn, dev, gflat_n, fused_into=fused_n)
        gh = torch.empty_like(h)
        g_agg = torch.empty(N, spec.O, D, dtype=torch.float32, device=dev)
        g_na = torch.empty_like(node_attr) if (node_attr is not None and want_gna) else None
        g_ea = torch.empty_like(edge_attr) if (edge_attr is not None and want_gea) else None

        def stage(binding, state):
            ws, saved = state if state is not None else (binding.workspace(dev), None)
            flags = native.FLAG_WEIGHTS_PACKED if state is not None else 0
            if getattr(saved, "csmpn_save_state", False):
                flags |= native.FLAG_SAVE_STATE
            return ws, saved, flags

        ws_e, saved_e, fl_e = stage(e, state_e)
        ws_n, saved_n, fl_n = stage(nd, state_n)
        check(native.lib().csmpn_egcl_backward(
            e.metric_arr, e.n, e.params, e.grads, e.nblk, nd.params, nd.grads, nd.nblk, h.data_ptr(), spec.C,
            agg.data_ptr(), spec.O, _ptr(edge_attr), spec.A, _ptr(node_attr), spec.T, csr.perm.data_ptr(),
            csr.src.data_ptr(), csr.dst.data_ptr(), csr.deg.data_ptr(), spec.mean, spec.residual, csr.n_edges, N,
            gout.data_ptr(), gh.data_ptr(), g_agg.data_ptr(), _ptr(g_ea), _ptr(g_na), None, _ptr(saved_e),
            ws_e.data_ptr(), ws_e.numel(), fl_e, _ptr(saved_n), ws_n.data_ptr(), ws_n.numel(), fl_n, _stream(dev)))
        return gh, g_ea, g_na, views_e, views_n


# CSMPN_FLAG_SAVE_STATE (round 4): the EGCL stage forwards also store every block's output in front of its layer norm and the
# backwards read it instead of recomputing linear_left + the geometric product. Honoured by the Cl(3,0) 8-channel kernels
# (S1: step 0.1915 -> 0.1866 ms), a no-op elsewhere; CSMPN_SAVE_STATE=0 turns it off (A/B runs).
_SAVE_STATE = os.environ.get("CSMPN_SAVE_STATE", "1") not in ("0", "")


def _check_egcl_inputs(spec, csr, h, edge_attr, node_attr, n_edges):
    D = spec.edge.D
    if h.dim() != 3 or h.shape[1] != spec.C or h.shape[2] != D:
        raise RuntimeError(f"h must be [N, {spec.C}, {D}], got {tuple(h.shape)}")
    if (edge_attr is None) != (spec.A == 0) or (node_attr is None) != (spec.T == 0):
        raise RuntimeError("edge_attr/node_attr presence does not match edge_attr_features/node_attr_features")
    if edge_attr is not None and tuple(edge_attr.shape) != (n_edges, spec.A, D):
        raise RuntimeError(f"edge_attr must be [{n_edges}, {spec.A}, {D}], got {tuple(edge_attr.shape)}")
    if node_attr is not None and tuple(node_attr.shape) != (h.shape[0], spec.T, D):
        raise RuntimeError(f"node_attr must be [{h.shape[0]}, {spec.T}, {D}], got {tuple(node_attr.shape)}")


class _EgclFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, edge_attr, node_attr, spec: EgclSpec, csr: Csr, *params):
        _require_device(h, "EGCL input h")
        _check_egcl_inputs(spec, csr, h, edge_attr, node_attr, csr.n_edges)
        h = h.contiguous()
        if edge_attr is not None:
            _require_device(edge_attr, "edge_attr")
            edge_attr = edge_attr.contiguous()
        if node_attr is not None:
            _require_device(node_attr, "node_attr")
            node_attr = node_attr.contiguous()
        ne = spec.edge.nblk * NP
        pe, pn = params[:ne], params[ne:]
        # one memset for everything that must start from zero: the aggregate and, when a backward
        # will follow, both models' flat gradient buffers
        spec.edge.bind(pe); spec.node.bind(pn)
        n_agg = h.shape[0] * spec.O * spec.edge.D
        ctx.param_refs = params
        fuse = _fusable(params, h.device)   # gradients go straight into p.grad: no flat buffers to zero
        n_ge, n_gn = (spec.edge.grad_floats(pe), spec.node.grad_floats(pn)) if (any(ctx.needs_input_grad) and not fuse) else (0, 0)
        zeros = torch.zeros(n_agg + n_ge + n_gn, dtype=torch.float32, device=h.device)
        agg = zeros[:n_agg].view(h.shape[0], spec.O, spec.edge.D)
        ctx.gflats = (zeros[n_agg:n_agg + n_ge], zeros[n_agg + n_ge:]) if n_ge else None
        agg, st_e = HipBackend.edge_forward(spec, csr, h, edge_attr, pe, agg=agg)
        out, st_n = HipBackend.node_forward(spec, csr.deg, h, agg, node_attr, pn)
        ctx.spec, ctx.csr, ctx.st_e, ctx.st_n = spec, csr, st_e, st_n
        ctx.has_ea, ctx.has_na = edge_attr is not None, node_attr is not None
        ctx.mask = [p is not None for p in params]
        saved = [h, agg]
        if ctx.has_ea:
            saved.append(edge_attr)
        if ctx.has_na:
            saved.append(node_attr)
        ctx.save_for_backward(*saved, *[p for p in params if p is not None])
        return out

    @staticmethod
    def backward(ctx, gout):
        spec, csr = ctx.spec, ctx.csr
        saved = list(ctx.saved_tensors)
        h, agg = saved[0], saved[1]
        pos = 2
        edge_attr = node_attr = None
        if ctx.has_ea:
            edge_attr = saved[pos]; pos += 1
        if ctx.has_na:
            node_attr = saved[pos]; pos += 1
        it = iter(saved[pos:])
        params = [next(it) if m else None for m in ctx.mask]
        ne = spec.edge.nblk * NP
        pe, pn = params[:ne], params[ne:]
        gout = gout.contiguous()
        gfe, gfn = ctx.gflats if ctx.gflats is not None else (None, None)
        ctx.gflats = None   # zeroed once: a second backward through the same graph allocates afresh
        refs = ctx.param_refs
        fuse = _fusable(refs, h.device)
        if isinstance(csr, Csr) and not deterministic_request():
            gh, g_ea, g_na, views_e, views_n = HipBackend.layer_backward(
                spec, csr, h, agg, edge_attr, node_attr, pe, pn, gout, ctx.needs_input_grad[1], ctx.needs_input_grad[2],
                ctx.st_e, ctx.st_n, gfe, gfn, refs[:ne] if fuse else None, refs[ne:] if fuse else None)
            return (gh, g_ea, g_na, None, None, *views_e, *views_n)
        gh, g_agg, g_na, views_n = HipBackend.node_backward(spec, csr.deg, h, agg, node_attr, pn, gout,
                                                            ctx.needs_input_grad[2], ctx.st_n, gfn,
                                                            fused_into=refs[ne:] if fuse else None)
        g_ea, views_e = HipBackend.edge_backward(spec, csr, h, edge_attr, pe, g_agg, gh, ctx.needs_input_grad[1],
                                                 ctx.st_e, gfe, fused_into=refs[:ne] if fuse else None)
        return (gh, g_ea, g_na, None, None, *views_e, *views_n)


def egcl_apply(h, edge_attr, node_attr, spec: EgclSpec, csr: Csr, params):
    if h.is_cuda:   # (a CPU tensor: _EgclFn raises "no CPU fallback", first of all)
        ne = spec.edge.nblk * NP
        row_family = h.dtype == torch.float64 or (h.dtype == torch.float32 and spec.edge.sig_only())
        if row_family:
            _on_device_like(h, (("edge_attr", edge_attr), ("node_attr", node_attr)))
        _same_dtype(h, (("edge_attr", edge_attr), ("node_attr", node_attr)), "EGCL")
        _same_dtype(h, ((f"parameter {PARAM_FIELDS[j % NP]} of block {j // NP} of the edge model", p) for j, p in enumerate(params[:ne])),
                    "EGCL")
        _same_dtype(h, ((f"parameter {PARAM_FIELDS[j % NP]} of block {j // NP} of the node model", p) for j, p in enumerate(params[ne:])),
                    "EGCL")
        if row_family:
            return _EgclF64Fn.apply(h, edge_attr, node_attr, spec, csr, *params)
    return _EgclFn.apply(h, edge_attr, node_attr, spec, csr, *params)


# --------------------------------------------------------------------------------- geometric product


class _GpFn(torch.autograd.Function):
    @staticmethod
    @_on_device_of(1)
    def forward(ctx, a, b, metric):
        _require_device(a, "geometric_product operand")
        _require_device(b, "geometric_product operand")
        shape = torch.broadcast_shapes(a.shape, b.shape)
        a2 = a.expand(shape).contiguous()
        b2 = b.expand(shape).contiguous()
        n = len(metric)
        D = 1 << n
        rows = a2.numel() // D
        out = torch.empty_like(a2)
        check(native.lib().csmpn_geometric_product_forward(native.metric_array(metric), n, a2.data_ptr(),
                                                           b2.data_ptr(), out.data_ptr(), rows, _stream(a.device)))
        ctx.save_for_backward(a2, b2)
        ctx.metric, ctx.shapes = metric, (a.shape, b.shape)
        return out

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gout):
        a2, b2 = ctx.saved_tensors
        metric = ctx.metric
        n = len(metric)
        D = 1 << n
        gout = gout.contiguous()
        ga, gb = torch.zeros_like(a2), torch.zeros_like(b2)
        check(native.lib().csmpn_geometric_product_backward(native.metric_array(metric), n, a2.data_ptr(),
                                                            b2.data_ptr(), gout.data_ptr(), ga.data_ptr(),
                                                            gb.data_ptr(), a2.numel() // D, _stream(a2.device)))
        sa, sb = ctx.shapes
        return ga.sum_to_size(sa), gb.sum_to_size(sb), None


# --------------------------------------------------------------------------------- standalone MVLinear


class _MVLinearFn(torch.autograd.Function):
    """y[b,o,d] = sum_i W[o,i,grade(d)] x[b,i,d] (+ bias on blade 0) through csmpn_mvlinear_*
    (cegnn_utils.py:326-338), for the MVLinear calls outside a CEMLP."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, weight, bias, n):
        _require_device(x, "MVLinear input")
        for name, t in (("weight", weight), ("bias", bias)):
            if t is not None and (t.device != x.device or t.dtype != torch.float32):
                raise RuntimeError(f"MVLinear {name} must be float32 on {x.device}, got {t.dtype} on {t.device}")
        x = x.contiguous()
        w = weight.contiguous()
        b = bias.contiguous() if bias is not None else None
        rows, I, D = x.shape
        O = w.shape[0]
        if D != (1 << n) or w.shape[1] != I:
            raise RuntimeError(f"MVLinear: input {tuple(x.shape)} does not match weight {tuple(w.shape)} (n={n})")
        y = torch.empty(rows, O, D, dtype=torch.float32, device=x.device)
        check(native.lib().csmpn_mvlinear_forward(n, x.data_ptr(), w.data_ptr(), _ptr(b), rows, I, O,
                                                  1 if w.dim() == 3 else 0, y.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(x, w)
        ctx.n, ctx.has_bias = n, bias is not None
        # the caller's parameter objects: with fused gradient accumulation the backward kernel adds into their .grad
        ctx.param_refs = (weight if weight.is_contiguous() else None, bias if (bias is None or bias.is_contiguous()) else False)
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        rows, I, D = x.shape
        O = w.shape[0]
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        pw, pb = ctx.param_refs
        sub = 1 if w.dim() == 3 else 0

        def run(gw_ptr, gb_ptr):
            if deterministic_request() and (gw_ptr is not None or gb_ptr is not None):
                # the atomic-free form: per-slab partial sums in scratch, added in a fixed order into the same targets
                ws = _det_scratch(native.lib().csmpn_mvlinear_backward_det_bytes(ctx.n, rows, I, O, sub), x.device)
                check(native.lib().csmpn_mvlinear_backward_det(ctx.n, x.data_ptr(), w.data_ptr(), gy.data_ptr(), rows, I, O, sub,
                                                               _ptr(gx), gw_ptr, gb_ptr, ws.data_ptr(), ws.numel(),
                                                               _stream(x.device)))
            else:
                check(native.lib().csmpn_mvlinear_backward(ctx.n, x.data_ptr(), w.data_ptr(), gy.data_ptr(), rows, I, O, sub,
                                                           _ptr(gx), gw_ptr, gb_ptr, _stream(x.device)))

        if (pw is not None and pb is not False and (need_w or need_b)
                and _fusable([pw if need_w else None, pb if need_b else None], x.device)
                and (not need_b or pb.grad.numel() == O)):
            # fused accumulation (set_fused_grad_accumulation): the kernel's atomics (under a deterministic request: the
            # fixed-order sum of the slabs) land in the parameters' own .grad - no zero fills, no AccumulateGrad adds
            # (6 + 6 launches per md17 step)
            run(pw.grad.data_ptr() if need_w else None, pb.grad.data_ptr() if need_b else None)
            return gx, None, None, None
        gw = torch.zeros_like(w) if need_w else None   # None: frozen weight (bias still gets its gradient)
        gb = torch.zeros(1, O, 1, dtype=torch.float32, device=x.device) if need_b else None
        run(_ptr(gw), _ptr(gb))
        return gx, gw, gb, None


# --------------------------------------------------------------------------------- the small layers on their own

_SMALL_LAUNCHES = 0


def small_layer_launches() -> int:
    """Launches of the standalone small-layer entry points so far (tests assert that the HIP path ran)."""
    return _SMALL_LAUNCHES


def _small_args(x, what, params):
    _require_device(x, f"{what} input")
    if x.dim() != 3:
        raise RuntimeError(f"{what}: the HIP path takes [rows, channels, D] inputs, got {tuple(x.shape)}")
    for t in params:
        if t.device != x.device or t.dtype != torch.float32:
            raise RuntimeError(f"{what} parameters must be float32 on {x.device}, got {t.dtype} on {t.device}")
    return x.contiguous()


def _count():
    global _SMALL_LAUNCHES
    _SMALL_LAUNCHES += 1


class _MVSiLUFn(torch.autograd.Function):
    """csmpn_mvsilu_* (cegnn_utils.py:53-83, invariant "mag2"); a, b [1, C, G]."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, a, b, metric):
        x = _small_args(x, "MVSiLU", (a, b))
        a2, b2 = a.contiguous(), b.contiguous()
        y = torch.empty_like(x)
        check(native.lib().csmpn_mvsilu_forward(native.metric_array(metric), len(metric), x.data_ptr(), a2.data_ptr(),
                                                b2.data_ptr(), x.shape[0], x.shape[1], y.data_ptr(), _stream(x.device)))
        _count()
        ctx.save_for_backward(x, a2, b2)
        ctx.metric = metric
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        x, a, b = ctx.saved_tensors
        gy = gy.contiguous()
        gx, ga, gb = torch.empty_like(x), torch.zeros_like(a), torch.zeros_like(b)
        args = (native.metric_array(ctx.metric), len(ctx.metric), x.data_ptr(), a.data_ptr(), b.data_ptr(), gy.data_ptr(),
                x.shape[0], x.shape[1], gx.data_ptr(), ga.data_ptr(), gb.data_ptr())
        if deterministic_request():   # the atomic-free form: parked contributions, per-workgroup partial rows in scratch
            ws = _small_det_scratch(native.LAYER_MVSILU, ctx.metric, x)
            check(native.lib().csmpn_mvsilu_backward_det(*args, ws.data_ptr(), ws.numel(), _stream(x.device)))
        else:
            check(native.lib().csmpn_mvsilu_backward(*args, _stream(x.device)))
        _count()
        return gx, ga, gb, None


class _RowParamFn(torch.autograd.Function):
    """NormalizationLayer (csmpn_mvnorm_*, a [C, G]) and MVLayerNorm (csmpn_mvlayernorm_*, a [1, C]): one
    parameter tensor, same call shape."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, a, metric, which):
        x = _small_args(x, which, (a,))
        a2 = a.contiguous()
        y = torch.empty_like(x)
        # MVLayerNorm sums a row's channel norms across lanes: its forward has a _det form too (no scratch)
        det = which == "mvlayernorm" and deterministic_request()
        fwd = getattr(native.lib(), f"csmpn_{which}_forward" + ("_det" if det else ""))
        check(fwd(native.metric_array(metric), len(metric), x.data_ptr(), a2.data_ptr(), x.shape[0], x.shape[1],
                  y.data_ptr(), _stream(x.device)))
        if det:
            _count_det()
        _count()
        ctx.save_for_backward(x, a2)
        ctx.metric, ctx.which = metric, which
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        x, a = ctx.saved_tensors
        gy = gy.contiguous()
        gx, ga = torch.empty_like(x), torch.zeros_like(a)
        args = (native.metric_array(ctx.metric), len(ctx.metric), x.data_ptr(), a.data_ptr(), gy.data_ptr(),
                x.shape[0], x.shape[1], gx.data_ptr(), ga.data_ptr())
        if deterministic_request():
            op = native.LAYER_MVNORM if ctx.which == "mvnorm" else native.LAYER_MVLAYERNORM
            ws = _small_det_scratch(op, ctx.metric, x)
            check(getattr(native.lib(), f"csmpn_{ctx.which}_backward_det")(*args, ws.data_ptr(), ws.numel(), _stream(x.device)))
        else:
            check(getattr(native.lib(), f"csmpn_{ctx.which}_backward")(*args, _stream(x.device)))
        _count()
        return gx, ga, None, None


class _WgpFn(torch.autograd.Function):
    """The path-weighted geometric product of SteerableGeometricProductLayer (csmpn_wgp_*,
    cegnn_utils.py:126-152): z, r [rows, C, D], weight [C, P]."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, z, r, weight, metric):
        z = _small_args(z, "weighted geometric product", (r, weight))
        r2, w2 = r.contiguous(), weight.contiguous()
        if r2.shape != z.shape or w2.shape[0] != z.shape[1]:
            raise RuntimeError(f"weighted geometric product: shapes {tuple(z.shape)}, {tuple(r2.shape)}, {tuple(w2.shape)}")
        y = torch.empty_like(z)
        check(native.lib().csmpn_wgp_forward(native.metric_array(metric), len(metric), z.data_ptr(), r2.data_ptr(),
                                             w2.data_ptr(), z.shape[0], z.shape[1], y.data_ptr(), _stream(z.device)))
        _count()
        ctx.save_for_backward(z, r2, w2)
        ctx.metric = metric
        return y

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, gy):
        z, r, w = ctx.saved_tensors
        gy = gy.contiguous()
        gz, gr, gw = torch.empty_like(z), torch.empty_like(r), torch.zeros_like(w)
        args = (native.metric_array(ctx.metric), len(ctx.metric), z.data_ptr(), r.data_ptr(), w.data_ptr(), gy.data_ptr(),
                z.shape[0], z.shape[1], gz.data_ptr(), gr.data_ptr(), gw.data_ptr())
        if deterministic_request():
            ws = _small_det_scratch(native.LAYER_WGP, ctx.metric, z)
            check(native.lib().csmpn_wgp_backward_det(*args, ws.data_ptr(), ws.numel(), _stream(z.device)))
        else:
            check(native.lib().csmpn_wgp_backward(*args, _stream(z.device)))
        _count()
        return gz, gr, gw, None


def _metric_of(algebra):
    mt = getattr(algebra, "metric_tuple", None)     # host copy: no device synchronisation per call
    return tuple(float(m) for m in (mt if mt is not None else algebra.metric.tolist()))


def small_layer_on_hip(algebra, x, *params) -> bool:
    """True when a standalone small layer takes the HIP entry points: float32 [rows, C, D] device input, a
    signature the kernels are compiled for, at most 256 channels, parameters on the same device."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[1] <= 256
            and getattr(algebra, "hip_supported", False) and all(p.is_cuda for p in params))


def mvsilu_apply(algebra, x, a, b):
    return _MVSiLUFn.apply(x, a, b, _metric_of(algebra))


def mvnorm_apply(algebra, x, a):
    return _RowParamFn.apply(x, a, _metric_of(algebra), "mvnorm")


def mvlayernorm_apply(algebra, x, a):
    return _RowParamFn.apply(x, a, _metric_of(algebra), "mvlayernorm")


def wgp_apply(algebra, z, r, weight):
    return _WgpFn.apply(z, r, weight, _metric_of(algebra))


def mvlinear_apply(x, weight, bias, n):
    return _MVLinearFn.apply(x, weight, bias, int(n))


def geometric_product_apply(a, b, metric):
    return _GpFn.apply(a, b, tuple(float(m) for m in metric))


# --------------------------------------------------------------------------------- callers either side (SURVEY §8(f)-1,2)


@_on_device_of(2)
def simplex_rows(n: int, blocks, verts: torch.Tensor) -> torch.Tensor:
    """Input rows of the simplex feature embedding (csmpn_simplex_rows). blocks: [(tensor [S, K, n_g], grade)],
    verts [rows, d+1] int64 batch rows of the vertices in one vertex order. The feature tensors are data
    (no gradient flows to them in the reference's models): tensors that require grad are refused."""
    if not verts.is_cuda:
        raise RuntimeError("simplex vertex table must live on the GPU (no CPU fallback)")
    if verts.dtype != torch.int64 or verts.dim() != 2:
        raise RuntimeError("verts must be int64 [rows, vertices]")
    verts = verts.contiguous()
    arr = (native.VertexBlock * len(blocks))()
    keep, ctot, S = [], 0, None
    for i, (t, grade) in enumerate(blocks):
        if t.requires_grad:
            raise RuntimeError("simplex_rows: feature tensors are inputs (no gradient); detach them")
        _require_device(t, "simplex feature block")
        t = t.contiguous()
        if t.dim() != 3 or t.dtype != torch.float32 or t.device != verts.device:
            raise RuntimeError(f"feature block {i} must be float32 [S, K, n_g] on {verts.device}")
        if t.shape[2] != _binom(n, int(grade)):
            raise RuntimeError(f"feature block {i}: last dimension {t.shape[2]} is not the size of grade {grade}")
        if S is None:
            S = t.shape[0]
        elif S != t.shape[0]:
            raise RuntimeError("feature blocks disagree on the number of rows")
        keep.append(t)
        arr[i].data, arr[i].channels, arr[i].grade = t.data_ptr(), t.shape[1], int(grade)
        ctot += verts.shape[1] * t.shape[1]
    out = torch.empty(verts.shape[0], ctot, 1 << n, dtype=torch.float32, device=verts.device)
    check(native.lib().csmpn_simplex_rows(n, arr, len(blocks), verts.data_ptr(), verts.shape[0], verts.shape[1], S,
                                          out.data_ptr(), _stream(verts.device)))
    return out


class _TypeAttrFn(torch.autograd.Function):
    """(node_attr [S, K, D], edge_attr [E, 2 K, D]) from a table of per-type features through csmpn_type_attr_* (one launch
    each way). table [T, K] float32; types [S], src / dst [E] int32 (constants of the batch)."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, table, types, src, dst, n):
        _require_device(table, "type-attribute table")
        tab = table.contiguous()
        T, K = tab.shape
        S, E, D = int(types.shape[0]), int(src.shape[0]), 1 << n
        node_attr = torch.empty(S, K, D, dtype=torch.float32, device=tab.device)
        edge_attr = torch.empty(E, 2 * K, D, dtype=torch.float32, device=tab.device)
        check(native.lib().csmpn_type_attr_forward(n, tab.data_ptr(), T, K, types.data_ptr(), S, src.data_ptr(), dst.data_ptr(), E,
                                                   node_attr.data_ptr(), edge_attr.data_ptr(), _stream(tab.device)))
        ctx.save_for_backward(types, src, dst)
        ctx.dims = (n, T, K)
        ctx.table_ref = table if table.is_contiguous() else None
        return node_attr, edge_attr

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, g_node, g_edge):
        types, src, dst = ctx.saved_tensors
        n, T, K = ctx.dims
        if not ctx.needs_input_grad[0] or (g_node is None and g_edge is None):
            return None, None, None, None, None
        g_node = g_node.contiguous() if g_node is not None else None
        g_edge = g_edge.contiguous() if g_edge is not None else None
        ref = ctx.table_ref
        fuse = ref is not None and _fusable([ref], types.device)
        g_tab = ref.grad if fuse else torch.zeros(T, K, dtype=torch.float32, device=types.device)
        S, E = int(types.shape[0]), int(src.shape[0])
        if deterministic_request() and S + E > 0:
            ws = _det_scratch(native.lib().csmpn_type_attr_backward_det_bytes(T, K, S, E), types.device)
            check(native.lib().csmpn_type_attr_backward_det(n, T, K, types.data_ptr(), S, src.data_ptr(), dst.data_ptr(), E,
                                                            _ptr(g_node), _ptr(g_edge), g_tab.data_ptr(), ws.data_ptr(),
                                                            ws.numel(), _stream(types.device)))
        else:
            check(native.lib().csmpn_type_attr_backward(n, T, K, types.data_ptr(), S, src.data_ptr(), dst.data_ptr(), E,
                                                        _ptr(g_node), _ptr(g_edge), g_tab.data_ptr(), _stream(types.device)))
        return (None if fuse else g_tab), None, None, None, None


def type_attr_apply(table, types_i32, src_i32, dst_i32, n):
    return _TypeAttrFn.apply(table, types_i32, src_i32, dst_i32, int(n))


def _binom(n, k):
    import math
    return math.comb(n, k)


class _ReadoutMseFn(torch.autograd.Function):
    """loss_g = (mean_{s in g} MVLinear(x)[s, 0, blade 0] - target_g)^2 (hulls_cssmpnn.py:93,155-164)."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, weight, bias, graph_ptr, target, n):
        _require_device(x, "readout input")
        x = x.contiguous()
        S, Cc, D = x.shape
        if weight.shape[0] != 1 or weight.shape[1] != Cc or D != (1 << n):
            raise RuntimeError(f"readout: weight {tuple(weight.shape)} does not fit input {tuple(x.shape)} with out_features = 1")
        w = weight.contiguous()
        stride = w.shape[2] if w.dim() == 3 else 1
        b = bias.contiguous() if bias is not None else None
        B = graph_ptr.shape[0] - 1
        tgt = target.contiguous().float()
        pred = torch.empty(B, dtype=torch.float32, device=x.device)
        loss = torch.empty(B, dtype=torch.float32, device=x.device)
        xs = torch.empty(B, Cc, dtype=torch.float32, device=x.device)
        check(native.lib().csmpn_readout_mse_forward(n, x.data_ptr(), w.data_ptr(), stride, _ptr(b), S, Cc,
                                                     graph_ptr.data_ptr(), B, tgt.data_ptr(), pred.data_ptr(),
                                                     loss.data_ptr(), xs.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(w, graph_ptr, pred, tgt, xs)
        ctx.n, ctx.shape, ctx.has_bias = n, (S, Cc, D), bias is not None
        ctx.mark_non_differentiable(pred)
        return loss, pred

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, g_loss, _g_pred):
        w, graph_ptr, pred, tgt, xs = ctx.saved_tensors
        S, Cc, D = ctx.shape
        B = graph_ptr.shape[0] - 1
        cnt = (graph_ptr[1:] - graph_ptr[:-1]).clamp(min=1).float()
        dpred = g_loss.contiguous() * 2.0 * (pred - tgt)            # d/d pred_g
        coef = (dpred / cnt).contiguous()
        gx = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty(S, Cc, D, dtype=torch.float32, device=w.device)
            stride = w.shape[2] if w.dim() == 3 else 1
            check(native.lib().csmpn_readout_mse_backward(ctx.n, w.data_ptr(), stride, S, Cc, graph_ptr.data_ptr(), B,
                                                          coef.data_ptr(), gx.data_ptr(), _stream(w.device)))
        gw = None
        if ctx.needs_input_grad[1]:
            gw = torch.zeros_like(w)
            gc = coef @ xs                                           # [C]
            if w.dim() == 3:
                gw[0, :, 0] = gc
            else:
                gw[0, :] = gc
        gb = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            nonempty = ((graph_ptr[1:] - graph_ptr[:-1]) > 0).float()
            gb = (dpred * nonempty).sum().reshape(1, 1, 1)
        return gx, gw, gb, None, None, None


class _ReadoutTrajFn(torch.autograd.Function):
    """Vector readout + loss of the trajectory models (csmpn_readout_traj_*; md17_cssmpnn.py:165-176,
    motion_cssmpnn.py:150-168, nba_cssmpnn.py:176-191). Returns (per_graph [B, 3] = MSE / ADE / FDE, per_vertex [V] MSE,
    pred [V, O, n]); gradients w.r.t. x and the MVLinear weight (its grade-1 entries)."""

    @staticmethod
    @_on_device_of(1)
    def forward(ctx, x, weight, loc, target, tables, n):
        _require_device(x, "readout input")
        x = x.contiguous()
        S, Cc, D = x.shape
        w = weight.contiguous()
        if w.dim() != 3 or w.shape[1] != Cc or w.shape[2] < 2 or D != (1 << n):
            raise RuntimeError(f"trajectory readout: weight {tuple(weight.shape)} does not fit input {tuple(x.shape)}")
        O = int(w.shape[0])
        vrows, vof, trow, gov, vptr = tables["vrows"], tables["vertex_of_row"], tables["trow"], tables["graph_of_vertex"], tables["vptr"]
        V, B = int(gov.shape[0]), int(vptr.shape[0]) - 1
        if vrows is None and S != V:
            raise RuntimeError("trajectory readout: identity vertex rows need one input row per vertex")
        tgt = target.contiguous().float().reshape(-1, O, n)
        lc = None if loc is None else loc.contiguous().float().reshape(V, O, n)
        pred = torch.empty(V, O, n, dtype=torch.float32, device=x.device)
        per_graph = torch.empty(B, 3, dtype=torch.float32, device=x.device)
        per_vertex = torch.empty(V, dtype=torch.float32, device=x.device)
        check(native.lib().csmpn_readout_traj_forward(n, x.data_ptr(), Cc, _ptr(vrows), V, w.data_ptr(), O, int(w.shape[2]), _ptr(lc),
                                                      tgt.data_ptr(), _ptr(trow), vptr.data_ptr(), B, pred.data_ptr(),
                                                      per_graph.data_ptr(), per_vertex.data_ptr(), _stream(x.device)))
        ctx.save_for_backward(x, w, pred, tgt)
        ctx.tables, ctx.n = tables, n
        ctx.mark_non_differentiable(pred)
        return per_graph, per_vertex, pred

    @staticmethod
    @_on_device_of(1)
    def backward(ctx, g_graph, g_vertex, _g_pred):
        x, w, pred, tgt = ctx.saved_tensors
        t = ctx.tables
        S, Cc, D = x.shape
        V, O, n = pred.shape
        gg = None if g_graph is None else g_graph.contiguous().float()
        gv = None if g_vertex is None else g_vertex.contiguous().float()
        gx = torch.empty_like(x)
        gw = torch.zeros_like(w)
        scratch = torch.empty(V, O, n, dtype=torch.float32, device=x.device)
        check(native.lib().csmpn_readout_traj_backward(
            ctx.n, x.data_ptr(), Cc, S, _ptr(t["vrows"]), _ptr(t["vertex_of_row"]), V, w.data_ptr(), O, int(w.shape[2]),
            pred.data_ptr(), tgt.data_ptr(), _ptr(t["trow"]), t["graph_of_vertex"].data_ptr(), t["vptr"].data_ptr(), _ptr(gg),
            _ptr(gv), scratch.data_ptr(), gx.data_ptr(), gw.data_ptr(), _stream(x.device)))
        return gx, gw, None, None, None, None


def readout_traj_tables(graph_of_vertex, n_graphs, vertex_rows=None, n_rows=None, unscored_last=0, out=None,
                        vertices_per_graph=None):
    """Index tables of csmpn_readout_traj_* (int32, on the device of graph_of_vertex), built once per batch:
    vptr [B + 1] (the vertices of a graph are contiguous in the vertex list), graph_of_vertex [V]; with `vertex_rows` (rows of
    the layer output that are vertices) also its inverse vertex_of_row [n_rows]; unscored_last = k: the last k vertices of
    every graph are not scored (NBA: the ball) and the target rows number the scored ones consecutively.
    out = the dict of an earlier call with the same shapes and options: its tensors are refilled IN PLACE for another batch
    (same data_ptrs) with fixed-shape device ops only - no host round trip, so the contiguity check of the first build is
    not repeated, and `vertices_per_graph` [B] (the histogram of graph_of_vertex) must then be given: bincount would
    synchronise."""
    gov = graph_of_vertex.to(torch.int64)
    dev = gov.device
    V = int(gov.shape[0])
    if out is None:
        if V > 1 and bool((gov[1:] < gov[:-1]).any()):
            raise RuntimeError("trajectory readout: the vertices of a graph must be contiguous in the vertex list")
        cnt = torch.bincount(gov, minlength=n_graphs)
    else:
        cnt = vertices_per_graph.to(torch.int64)
    vptr = torch.zeros(n_graphs + 1, dtype=torch.int64, device=dev)
    vptr[1:] = torch.cumsum(cnt, 0)
    trow = None
    if unscored_last:
        pos = torch.arange(V, device=dev) - vptr[:-1].index_select(0, gov)   # position inside the graph
        scored = pos < (cnt.index_select(0, gov) - unscored_last)
        first = torch.cumsum(torch.cat([cnt.new_zeros(1), (cnt - unscored_last).clamp(min=0)[:-1]]), 0)
        trow = torch.where(scored, first.index_select(0, gov) + pos, torch.full_like(pos, -1)).to(torch.int32).contiguous()
    vrows = vof = None
    if vertex_rows is not None:
        vrows = vertex_rows.to(torch.int32).contiguous()
        vof = torch.full((int(n_rows),), -1, dtype=torch.int32, device=dev)
        vof.index_copy_(0, vertex_rows.long(), torch.arange(V, dtype=torch.int32, device=dev))
    new = {"vrows": vrows, "vertex_of_row": vof, "trow": trow, "graph_of_vertex": gov.to(torch.int32).contiguous(),
           "vptr": vptr.to(torch.int32).contiguous()}
    if out is None:
        return new
    for k, v in new.items():
        if (v is None) != (out[k] is None):
            raise RuntimeError(f"readout_traj_tables: table {k!r} exists on one side only (other options than the first build?)")
        if v is not None:
            out[k].copy_(v)
    return out


def readout_traj(x, weight, loc, target, tables, n):
    """(per_graph [B, 3] = (MSE, ADE, FDE), per_vertex [V] MSE, pred [V, O, n]); tables = readout_traj_tables(...)."""
    return _ReadoutTrajFn.apply(x, weight, loc, target, tables, int(n))


def readout_traj_supported(head, x) -> bool:
    """MVLinear(subspaces=True) heads on device float32 rows within the kernel's limits."""
    w = getattr(head, "weight", None)
    return (x.is_cuda and x.dtype == torch.float32 and w is not None and w.dim() == 3 and w.shape[1] <= 64
            and w.shape[0] <= 1024 and w.shape[0] * w.shape[1] <= 4096)


def readout_mse(x, weight, bias, graph_ptr_i32, target, n):
    """(loss per graph, prediction per graph); graph_ptr_i32 [B+1] int32 device tensor (rows of a graph are contiguous)."""
    return _ReadoutMseFn.apply(x, weight, bias, graph_ptr_i32, target, int(n))


# --------------------------------------------------------------------------------- per-batch index tables on the device

STATUS_TYPE_OUTSIDE, STATUS_CLAMPED = 16, 32   # bits of the status word of simplex_tables; bit d = the count of dimension d


def simplex_tables_workspace(n_rows: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of simplex_tables for batches of n_rows rows (uninitialised device bytes)."""
    return torch.empty(max(int(native.lib().csmpn_simplex_tables_workspace_bytes(int(n_rows), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def simplex_tables(x_ind, node_types, x_ind_batch, x_ind_ptr, max_dim, rows, verts, verts_i32, graph_of_vertex,
                   vertices_per_graph, types_i32, status, workspace):
    """csmpn_simplex_tables: the tables of SimplicialBatch.plan() written into the given buffers (rows[d] int64 [n_d],
    verts[d] int64 [n_d (d+1)!, d+1], verts_i32 = None or a list with None / int32 tensors of verts' shapes, graph_of_vertex
    int64 [n_0], vertices_per_graph int64 [B], types_i32 = None or int32 [S], status = None or a uint32 / int32 device word)
    on the current stream: no allocation, no host round trip. The expected counts n_d are the lengths of rows[d]."""
    if not x_ind.is_cuda:
        raise RuntimeError("simplex_tables needs device tensors (no CPU fallback)")
    for name, t in (("x_ind", x_ind), ("node_types", node_types), ("x_ind_batch", x_ind_batch), ("x_ind_ptr", x_ind_ptr),
                    ("graph_of_vertex", graph_of_vertex), ("vertices_per_graph", vertices_per_graph)):
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != x_ind.device:
            raise RuntimeError(f"simplex_tables: {name} must be a contiguous int64 tensor on the device of x_ind")
    nd = int(max_dim) + 1
    if len(rows) != nd or len(verts) != nd or (verts_i32 is not None and len(verts_i32) != nd):
        raise RuntimeError(f"simplex_tables: max_dim = {max_dim} needs {nd} tables of each kind")
    S, B = int(node_types.shape[0]), int(x_ind_ptr.shape[0]) - 1
    if x_ind.dim() != 2 or x_ind.shape[0] != S or x_ind_batch.shape[0] != S or vertices_per_graph.shape[0] != B:
        raise RuntimeError("simplex_tables: x_ind [S, M], node_types [S], x_ind_batch [S], x_ind_ptr [B + 1], vertices_per_graph [B]")
    fact = 1
    for d in range(nd):
        fact *= d + 1
        n_d = int(rows[d].shape[0])
        ok = rows[d].dtype == torch.int64 and verts[d].dtype == torch.int64 and tuple(verts[d].shape) == (n_d * fact, d + 1) \
            and rows[d].is_contiguous() and verts[d].is_contiguous()
        vi = None if verts_i32 is None else verts_i32[d]
        if vi is not None:
            ok = ok and vi.dtype == torch.int32 and vi.shape == verts[d].shape and vi.is_contiguous()
        if not ok and nd <= 4:   # (max_dim > 3: the entry point refuses before it reads a table)
            raise RuntimeError(f"simplex_tables: tables of dimension {d} must be rows int64 [n], verts int64 [n * {fact}, {d + 1}] (+ int32 copy)")
    if graph_of_vertex.shape[0] != rows[0].shape[0]:
        raise RuntimeError("simplex_tables: graph_of_vertex must have the length of rows[0]")
    if types_i32 is not None and (types_i32.dtype != torch.int32 or types_i32.shape[0] != S or not types_i32.is_contiguous()):
        raise RuntimeError("simplex_tables: types_i32 must be contiguous int32 [S]")
    if status is not None and (status.element_size() != 4 or status.numel() < 1 or not status.is_cuda):
        raise RuntimeError("simplex_tables: status must be a 4-byte device word")
    dev = x_ind.device
    arr = lambda ts: (C.c_void_p * nd)(*[None if t is None or t.numel() == 0 else t.data_ptr() for t in ts])
    expected = (C.c_int64 * nd)(*[int(r.shape[0]) for r in rows])
    r_arr, v_arr, i_arr = arr(rows), arr(verts), None if verts_i32 is None else arr(verts_i32)   # host arrays: alive over the call
    with torch.cuda.device(dev):
        check(native.lib().csmpn_simplex_tables(
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), x_ind_batch.data_ptr(), x_ind_ptr.data_ptr(), S, B,
            int(max_dim), C.addressof(expected), C.addressof(r_arr), C.addressof(v_arr),
            None if i_arr is None else C.addressof(i_arr), graph_of_vertex.data_ptr(),
            vertices_per_graph.data_ptr(), _ptr(types_i32), _ptr(status), workspace.data_ptr(), workspace.numel(), _stream(dev)))


# --------------------------------------------------------------------------------- the Rips lift of a batch on the device

# bits of the status word of rips_lift / knn_lift / hull_lift; bit d (d = 1, 2) = more d-simplices than the capacity
LIFT_STATUS_EDGES, LIFT_STATUS_NO_FILLER_ROW = 8, 16


def rips_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of rips_lift (uninitialised device bytes)."""
    return torch.empty(max(int(native.lib().csmpn_rips_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def _lift_arguments(what, points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
                    x_ind_ptr, edge_index, edge_types, counts, status):
    """The tensor validation rips_lift, knn_lift, hull_lift, clique_lift, cloud_lift and cloud_knn_lift share; returns (B, V, E, the capacity rows as a C array)."""
    if not points.is_cuda:
        raise RuntimeError(f"{what} needs device tensors (no CPU fallback)")
    if points.dtype != torch.float32 or points.dim() != 2 or not points.is_contiguous():
        raise RuntimeError(f"{what}: points must be a contiguous float32 tensor [B * V, n]")
    B, rows = int(n_graphs), [int(r) for r in capacity_rows]
    if B <= 0 or points.shape[0] % B:
        raise RuntimeError(f"{what}: {points.shape[0]} points do not divide into {B} graphs")
    S, E, nd = sum(rows), int(capacity_edges), int(max_dim) + 1
    if len(rows) != nd:
        raise RuntimeError(f"{what}: max_dim = {max_dim} needs {nd} row capacities")
    shapes = (("x_ind", x_ind, None), ("node_types", node_types, (S,)), ("batch", batch, (S,)), ("x_ind_batch", x_ind_batch, (S,)),
              ("ptr", ptr, (B + 1,)), ("x_ind_ptr", x_ind_ptr, (B + 1,)), ("edge_index", edge_index, (2, E)),
              ("edge_types", edge_types, (E, 2)), ("counts", counts, (nd + 1,)))
    for name, t, shape in shapes:
        if t is None and name in ("edge_types", "counts"):
            continue
        if t.dtype != torch.int64 or not t.is_contiguous() or t.device != points.device or (shape is not None and tuple(t.shape) != shape):
            raise RuntimeError(f"{what}: {name} must be a contiguous int64 tensor{'' if shape is None else ' ' + str(list(shape))} on the device of points")
    if x_ind.dim() != 2 or int(x_ind.shape[0]) != S:
        raise RuntimeError(f"{what}: x_ind must be [{S}, M]")
    if status is not None and (status.element_size() != 4 or status.numel() < 1 or status.device != points.device):
        raise RuntimeError(f"{what}: status must be a 4-byte device word")
    return B, int(points.shape[0]) // B, E, (C.c_int64 * nd)(*rows)


def rips_lift(points, n_graphs, dis, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
              x_ind_ptr, edge_index, edge_types, counts, status, workspace):
    """csmpn_rips_lift: the structure tensors of pad_batch(collate([rips_complex(points of graph g, dis, max_dim)]), capacity)
    written into the given int64 buffers of the capacity's shapes (x_ind [S, M], node_types / batch / x_ind_batch [S],
    ptr / x_ind_ptr [B + 1], edge_index [2, E], edge_types = None or [E, 2], counts = None or [max_dim + 2]) from
    points float32 [B * V, n] on the current stream: no allocation, no host round trip. A batch that does not fit leaves the
    buffers as they were and sets bits of `status` (None or a 4-byte device word)."""
    B, V, E, cap = _lift_arguments("rips_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    with torch.cuda.device(dev):
        check(native.lib().csmpn_rips_lift(
            points.data_ptr(), int(points.shape[1]), B, V, float(dis), int(max_dim), C.addressof(cap), E,
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(), x_ind_batch.data_ptr(), ptr.data_ptr(),
            x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts), _ptr(status), workspace.data_ptr(),
            workspace.numel(), _stream(dev)))


def knn_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of knn_lift (uninitialised device bytes)."""
    return torch.empty(max(int(native.lib().csmpn_knn_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def knn_lift(points, n_graphs, k, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
             x_ind_ptr, edge_index, edge_types, counts, status, workspace):
    """csmpn_knn_lift: rips_lift for the clique complex of the k-nearest-neighbour graph - the structure tensors of
    pad_batch(collate([knn_clique_complex(points of graph g, k, max_dim)]), capacity), same buffers, same status bits."""
    B, V, E, cap = _lift_arguments("knn_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    with torch.cuda.device(dev):
        check(native.lib().csmpn_knn_lift(
            points.data_ptr(), int(points.shape[1]), B, V, int(k), int(max_dim), C.addressof(cap), E,
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(), x_ind_batch.data_ptr(), ptr.data_ptr(),
            x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts), _ptr(status), workspace.data_ptr(),
            workspace.numel(), _stream(dev)))


def hull_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of hull_lift (uninitialised device bytes)."""
    return torch.empty(max(int(native.lib().csmpn_hull_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def hull_lift(points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr, x_ind_ptr,
              edge_index, edge_types, counts, status, workspace, volume=None):
    """csmpn_hull_lift: rips_lift for the convex-hull complex - the structure tensors of
    pad_batch(collate([hull_complex(points of graph g, max_dim, method="exact")]), capacity), same buffers, same status bits -
    and the hulls' volumes (csmpn.data.complexes.hull_facets) into `volume` (None or a contiguous float32 device tensor
    [B]), which a batch that does not fit leaves as it was, too. Points in R^2 .. R^5, at most 16 per graph."""
    B, V, E, cap = _lift_arguments("hull_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    if volume is not None and (volume.dtype != torch.float32 or not volume.is_contiguous() or volume.device != dev
                               or tuple(volume.shape) != (B,)):
        raise RuntimeError(f"hull_lift: volume must be a contiguous float32 tensor [{B}] on the device of points")
    with torch.cuda.device(dev):
        check(native.lib().csmpn_hull_lift(
            points.data_ptr(), int(points.shape[1]), B, V, int(max_dim), C.addressof(cap), E,
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(), x_ind_batch.data_ptr(), ptr.data_ptr(),
            x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts), _ptr(status), _ptr(volume),
            workspace.data_ptr(), workspace.numel(), _stream(dev)))


def clique_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of clique_lift (uninitialised device bytes); at least as large as those of the other three lifts."""
    return torch.empty(max(int(native.lib().csmpn_clique_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


LIFT_STATUS_BAD_LIST = 32          # bit 5 of the status word of clique_lift: an end outside the batch or across two graphs


def clique_lift(points, n_graphs, source, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
                x_ind_ptr, edge_index, edge_types, counts, status, workspace, edge_th=float("inf"), tri_th=float("inf")):
    """csmpn_clique_lift: rips_lift for the thresholded clique complex of any graph - the structure tensors of
    pad_batch(collate([clique_complex(points of graph g, its edges, edge_th, tri_th, max_dim)]), capacity), same buffers, same
    status bits. `source` names the graph: an int k >= 1 (the k-nearest-neighbour graph of knn_lift) or a contiguous int64
    device tensor [2, n] of GLOBAL vertex ids g V + a ((-1, -1) entries are padding; an end outside the batch or two ends in
    different graphs set LIFT_STATUS_BAD_LIST and leave the buffers as they were)."""
    B, V, E, cap = _lift_arguments("clique_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    if torch.is_tensor(source):
        if source.dtype != torch.int64 or source.dim() != 2 or int(source.shape[0]) != 2 or not source.is_contiguous() or source.device != dev:
            raise RuntimeError("clique_lift: the edge list must be a contiguous int64 tensor [2, n] on the device of points")
        # an empty list is a list all the same: any non-null address stands for it (n_list = 0: never read)
        k, list_ptr, n_list = 0, source.data_ptr() if source.numel() else workspace.data_ptr(), int(source.shape[1])
    else:
        k, list_ptr, n_list = int(source), None, 0
    with torch.cuda.device(dev):
        check(native.lib().csmpn_clique_lift(
            points.data_ptr(), int(points.shape[1]), B, V, k, list_ptr, n_list, float(edge_th), float(tri_th), int(max_dim),
            C.addressof(cap), E, x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(),
            x_ind_batch.data_ptr(), ptr.data_ptr(), x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts),
            _ptr(status), workspace.data_ptr(), workspace.numel(), _stream(dev)))


def cloud_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of cloud_lift (uninitialised device bytes): the mask words and ranks of every vertex, V^2 (1 / 8 + 1 / 16) bytes
    per graph."""
    return torch.empty(max(int(native.lib().csmpn_cloud_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def cloud_lift(points, n_graphs, dis, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
               x_ind_ptr, edge_index, edge_types, counts, status, workspace, vertex_block=False):
    """csmpn_cloud_lift: rips_lift for point clouds of up to 4096 vertices per graph - the structure tensors of
    pad_batch(collate([rips_complex(points of graph g, dis, max_dim, vertex_block)]), capacity), same buffers, same status
    bits. vertex_block=True: the adjacencies of rips_lift (the 0_0 block over the non-edges included); False: those of
    knn_lift, 6 n1 + 12 n2."""
    B, V, E, cap = _lift_arguments("cloud_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    with torch.cuda.device(dev):
        check(native.lib().csmpn_cloud_lift(
            points.data_ptr(), int(points.shape[1]), B, V, float(dis), int(vertex_block), int(max_dim), C.addressof(cap), E,
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(), x_ind_batch.data_ptr(), ptr.data_ptr(),
            x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts), _ptr(status), workspace.data_ptr(),
            workspace.numel(), _stream(dev)))


def cloud_knn_lift_workspace(n_graphs: int, verts_per_graph: int, max_dim: int, device) -> torch.Tensor:
    """Workspace of cloud_knn_lift (uninitialised device bytes): that of cloud_lift and V^2 / 8 bytes per graph more, the
    neighbour masks before they are made symmetric."""
    return torch.empty(max(int(native.lib().csmpn_cloud_knn_lift_workspace_bytes(int(n_graphs), int(verts_per_graph), int(max_dim))), 16),
                       dtype=torch.uint8, device=device)


def cloud_knn_lift(points, n_graphs, k, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch, x_ind_batch, ptr,
                   x_ind_ptr, edge_index, edge_types, counts, status, workspace):
    """csmpn_cloud_knn_lift: knn_lift for point clouds of up to 4096 vertices per graph - the structure tensors of
    pad_batch(collate([knn_clique_complex(points of graph g, k, max_dim)]), capacity), same buffers, same status bits."""
    B, V, E, cap = _lift_arguments("cloud_knn_lift", points, n_graphs, max_dim, capacity_rows, capacity_edges, x_ind, node_types, batch,
                                   x_ind_batch, ptr, x_ind_ptr, edge_index, edge_types, counts, status)
    dev = points.device
    with torch.cuda.device(dev):
        check(native.lib().csmpn_cloud_knn_lift(
            points.data_ptr(), int(points.shape[1]), B, V, int(k), int(max_dim), C.addressof(cap), E,
            x_ind.data_ptr(), int(x_ind.shape[1]), node_types.data_ptr(), batch.data_ptr(), x_ind_batch.data_ptr(), ptr.data_ptr(),
            x_ind_ptr.data_ptr(), edge_index.data_ptr(), _ptr(edge_types), _ptr(counts), _ptr(status), workspace.data_ptr(),
            workspace.numel(), _stream(dev)))
