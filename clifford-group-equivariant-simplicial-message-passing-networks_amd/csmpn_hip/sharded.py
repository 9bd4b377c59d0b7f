"""Edge-sharded EGCL over the GPUs of one node (one process per GPU, RCCL over xGMI).

The reference never shards a layer (its only multi-GPU mode is whole-model DDP,
csmpn/md17.py:15-20); this is the partitioning BASELINE.json's north_star names:

  * the edge / simplex-adjacency list is split into contiguous shards, one per rank;
    node features h, node_attr and all parameters are replicated;
  * forward: every rank runs the fused edge kernel on its shard -> partial
    agg[N, O, D]; ONE all-reduce (sum) over the per-node aggregated features; the
    node update then runs replicated (identical on every rank);
  * backward: node backward replicated; edge backward on the shard -> partial
    d/dh[N, C, D] and partial edge-model parameter gradients; ONE all-reduce over
    [d/dh | edge-model gradients] packed in a single buffer.
  * mean aggregation uses the GLOBAL in-degree (all-reduced once per complex).

The data path of a shard has no other exchange step. The compute backend is
injectable so that the collective plumbing is testable on CPU with gloo (tests
inject the oracle there); the default backend is the HIP C-ABI.

Partitioning B (`DstPartitionedEGCL`): rank r owns the nodes
[r N/W, (r+1) N/W) and ALL edges into them. Its aggregate is complete without any
reduction and the node update runs on its own nodes only, so nothing is computed
twice (partitioning A replicates the node update: an Amdahl bound of ~4x at 8 GPUs
with the S2 stage times). Exchanges per layer: forward ONE all-gather of the updated
node slices, backward ONE reduce-scatter of d/dh (the -g -> source half lands on any
node) plus an all-reduce of the parameter gradients (a few thousand floats) - half
the bytes of A, and both collectives use all xGMI links at once.
"""
from __future__ import annotations

import math
import os

import torch
import torch.distributed as dist

from . import ops


def shard_bounds(n: int, world: int, rank: int):
    """Contiguous, balanced part [lo, hi) of `n` items (the edge list) for `rank`: the first n % world parts are one longer."""
    base, rem = divmod(n, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


node_bounds = shard_bounds     # partitioning B without balancing: the same cut of the node range


# ===================================================================================== bookkeeping shared by both partitionings


def _split_params(spec, lp):
    """A layer's flat parameter list -> (edge-model part, node-model part)."""
    ne = spec.edge.nblk * ops.NP
    return lp[:ne], lp[ne:]


def _offsets(counts):
    """[0, c0, c0 + c1, ...]: where every layer's parameters start in the flat list of a chain."""
    offs = [0]
    for cnt in counts:
        offs.append(offs[-1] + cnt)
    return offs


def _acc(a, b):
    """a + b where either may be None."""
    return b if a is None else (a if b is None else a + b)


def _save(ctx, tensors, optional, params, counts=()):
    """What a Function keeps for its backward: `tensors`, the entries of `optional` (the attributes) and of `params` that
    are not None, and the per-layer parameter offsets of a chain."""
    ctx.n_tensors = len(tensors)
    ctx.has = [t is not None for t in optional]
    ctx.mask = [p is not None for p in params]
    ctx.offs = _offsets(counts)
    ctx.save_for_backward(*tensors, *[t for t in optional if t is not None], *[p for p in params if p is not None])


def _restore(ctx):
    """(tensors, optional, params) as given to _save, None where None was given."""
    it = iter(ctx.saved_tensors)
    tensors = [next(it) for _ in range(ctx.n_tensors)]
    optional = [next(it) if m else None for m in ctx.has]
    return tensors, optional, [next(it) if m else None for m in ctx.mask]


def _pack(views, lead=None):
    """[lead | the views that are not None] as one flat tensor."""
    return torch.cat(([] if lead is None else [lead.reshape(-1)]) + [v.reshape(-1) for v in views if v is not None])


def _cut_views(flat, shapes, off=0):
    """Views of `flat` laid end to end from `off`, one per shape (None stays None): the inverse of _pack."""
    out = []
    for shp in shapes:
        if shp is None:
            out.append(None)
        else:
            cnt = math.prod(shp)
            out.append(flat[off:off + cnt].view(shp))
            off += cnt
    return out


def _all_reduce_views(views, group, lead=None):
    """ONE all-reduce (sum) of [lead | views] as a flat tensor -> (reduced lead, views of the result)."""
    if lead is None and all(v is None for v in views):
        return None, views
    flat = _pack(views, lead)
    dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
    off = 0 if lead is None else lead.numel()
    return (None if lead is None else flat[:off].view_as(lead),
            _cut_views(flat, [None if v is None else v.shape for v in views], off))


class _Capture:
    """HIP-graph capture of a step's segments. The constructor runs `warm_up` once on a side stream, outside capture
    (kernel attributes, workspaces, allocator); every call then captures one function into a graph of its own, all in one
    memory pool, and returns (graph, what the function returned). Thread-local capture mode: the process group's
    watchdog thread polls events while we capture."""

    def __init__(self, warm_up):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            warm_up()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.pool = None

    def __call__(self, fn):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.pool, capture_error_mode="thread_local"):
            res = fn()
        self.pool = self.pool or g.pool()
        return g, res


# ===================================================================================== partitioning A


class ShardPlan:
    """Per-complex state of one rank: local CSR + global in-degree."""

    def __init__(self, edge_index_local, n_nodes, backend=ops.HipBackend, group=None):
        self.csr = backend.build_csr(edge_index_local, n_nodes)
        deg = self.csr.deg.clone()
        if _multi(group):
            dist.all_reduce(deg, op=dist.ReduceOp.SUM, group=group)
        self.deg = deg
        self.n_nodes = n_nodes


def _shard_backward(be, spec, plan: ShardPlan, h, agg, attrs, lp, gout, want, st):
    """Backward of the edge-sharded layer up to its collective: node backward on all nodes (replicated), edge backward
    on the shard. attrs = (edge_attr, node_attr), want = (d/d edge_attr?, d/d node_attr?), st = (edge, node) states.
    -> d/dh of the node stage, partial d/dh of the shard's edges, d/d edge_attr, d/d node_attr, edge-model and node-model
    parameter gradients. (Its forward is one backend call on either side of the all-reduce of agg: nothing to share.)"""
    pe, pn = _split_params(spec, lp)
    gh_node, g_agg, g_na, views_n = be.node_backward(spec, plan.deg, h, agg, attrs[1], pn, gout, want[1], st[1])
    # partial d/dh of this shard starts from zero so that the all-reduce sums shards only
    gh_edge = torch.zeros_like(h)
    g_ea, views_e = be.edge_backward(spec, plan.csr, h, attrs[0], pe, g_agg, gh_edge, want[0], st[0])
    return gh_node, gh_edge, g_ea, g_na, views_e, views_n


class _ShardedEgclFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, edge_attr, node_attr, spec, plan: ShardPlan, backend, group, *params):
        h = h.contiguous()
        pe, pn = _split_params(spec, params)
        agg, st_e = backend.edge_forward(spec, plan.csr, h, edge_attr, pe)
        if _multi(group):
            dist.all_reduce(agg, op=dist.ReduceOp.SUM, group=group)
        out, st_n = backend.node_forward(spec, plan.deg, h, agg, node_attr, pn)
        ctx.st = (st_e, st_n)
        ctx.spec, ctx.plan, ctx.backend, ctx.group = spec, plan, backend, group
        _save(ctx, [h, agg], [edge_attr, node_attr], params)
        return out

    @staticmethod
    def backward(ctx, gout):
        (h, agg), attrs, params = _restore(ctx)
        gh_node, gh_edge, g_ea, g_na, views_e, views_n = _shard_backward(
            ctx.backend, ctx.spec, ctx.plan, h, agg, attrs, params, gout.contiguous(), ctx.needs_input_grad[1:3], ctx.st)
        if _multi(ctx.group):
            # one collective: [d/dh | edge-model parameter gradients]
            gh_edge, views_e = _all_reduce_views(views_e, ctx.group, lead=gh_edge)
        gh = gh_node + gh_edge
        return (gh, g_ea, g_na, None, None, None, None, *views_e, *views_n)


def _layer_params(layer):
    return layer.edge_model.flat_params() + layer.node_model.flat_params()


class ShardedEGCL(torch.nn.Module):
    """Wraps an EGCL module; forward takes this rank's shard of the edge list."""

    def __init__(self, layer, backend=ops.HipBackend, group=None):
        super().__init__()
        self.layer = layer
        self.backend = backend
        self.group = group

    def plan(self, edge_index_local, n_nodes) -> ShardPlan:
        return ShardPlan(edge_index_local, n_nodes, self.backend, self.group)

    def forward(self, h, plan: ShardPlan, edge_attr_local=None, node_attr=None):
        return _ShardedEgclFn.apply(h, edge_attr_local, node_attr, self.layer.spec(), plan, self.backend, self.group,
                                    *_layer_params(self.layer))


class GraphedShardedStep:
    """Forward + backward of the sharded layer on FIXED buffers, for steady-state training loops
    and the multi-GPU benchmark: the compute stages are captured in two HIP graphs, the two
    collectives of the partitioning are launched eagerly between them (no collective inside a
    captured graph):

        [graph 1: edge forward] -> all_reduce(agg)
        -> [graph 2: node forward, node backward, edge backward, pack] -> all_reduce([d/dh | edge grads])
        -> d/dh = node part + reduced edge part

    Same stage calls, same collectives and same results as `_ShardedEgclFn`; what it removes is
    the per-step Python / autograd launch path (0.54 ms per step eager vs 0.47 ms of GPU time on
    S1), which would otherwise bound the N-GPU step. Inputs are read from the tensors given here:
    update them in place between `run()` calls."""

    def __init__(self, sharded_layer: "ShardedEGCL", plan: ShardPlan, h, edge_attr_local, node_attr, gout):
        layer, be = sharded_layer.layer, sharded_layer.backend
        self.group = sharded_layer.group
        self.spec = spec = layer.spec()
        self.pe = layer.edge_model.flat_params()
        self.pn = layer.node_model.flat_params()
        self.h, self.ea, self.na, self.gout = h.detach(), edge_attr_local, node_attr, gout
        self._multi = _multi(self.group)
        h_, ea, na, pe, pn = self.h, self.ea, self.na, self.pe, self.pn

        # N > 1: the edge forward runs as two launches over the two halves of the target-sorted
        # shard (targets < N/2 | >= N/2), so that the all-reduce of the first half of the aggregate
        # travels while the second half is still being computed. Needs the saved block inputs to be
        # one [rows, O, D] array (two-block edge model) and the default backend.
        self._split = None
        if (self._multi and be is ops.HipBackend and spec.edge.nblk == 2
                and os.environ.get("CSMPN_SPLIT_FWD", "1") != "0"):
            n_half = plan.n_nodes // 2
            e1 = int(plan.csr.row_ptr[n_half].item())
            # the choice changes which collectives a rank issues (two half-size all-reduces or one
            # whole one): it must be the same on every rank - split only if EVERY shard straddles N/2
            if agree_all(0 < e1 < plan.csr.n_edges, self.group, h.device):
                self._split = (n_half, e1)

        def part1():
            return be.edge_forward(spec, plan.csr, h_, ea, pe)

        def part1_lo():
            n_half, e1 = self._split
            spec.edge.bind(pe)
            agg = torch.zeros(h_.shape[0], spec.O, spec.edge.D, dtype=torch.float32, device=h_.device)
            saved = spec.edge.new_saved(plan.csr.n_edges, h_.device)
            # floats of one saved block-1 input row (NOT numel / rows: the buffer may carry a backward scratch region
            # behind the [rows, O, D] inputs, see csmpn_cemlp_saved_floats_per_row)
            per_row = int(spec.edge.params[0].out_features) * spec.edge.D
            _, (ws, _s) = be.edge_forward(spec, ops.CsrSlice(plan.csr, 0, e1), h_, ea, pe, agg=agg,
                                          saved=saved[:e1 * per_row])
            return agg, (ws, saved), per_row

        def part1_hi(agg, saved, per_row):
            n_half, e1 = self._split
            be.edge_forward(spec, ops.CsrSlice(plan.csr, e1, plan.csr.n_edges), h_, ea, pe, agg=agg,
                            saved=saved[e1 * per_row:])

        def part2(agg, st_e):
            out, st_n = be.node_forward(spec, plan.deg, h_, agg, na, pn)
            gh_node, gh_edge, _g_ea, _g_na, views_e, views_n = _shard_backward(
                be, spec, plan, h_, agg, (ea, na), pe + pn, self.gout, (False, False), (st_e, st_n))
            return out, gh_node, _pack(views_e, lead=gh_edge), views_e, views_n

        def warm_up():
            if self._split:
                agg, st_e, per_row = part1_lo()
                part1_hi(agg, st_e[1], per_row)
            else:
                agg, st_e = part1()
            part2(agg, st_e)

        capture = _Capture(warm_up)
        self.g1b = None
        if self._split:
            self.g1, (self.agg, self._st_e, per_row) = capture(part1_lo)
            self.g1b, _ = capture(lambda: part1_hi(self.agg, self._st_e[1], per_row))
        else:
            self.g1, (self.agg, self._st_e) = capture(part1)
        self.g2, (self.out, self.gh_node, self.packed, views_e, self.views_n) = capture(
            lambda: part2(self.agg, self._st_e))
        self._edge_shapes = [None if v is None else tuple(v.shape) for v in views_e]
        self.gh = torch.empty_like(h_)

    def run(self):
        self.g1.replay()
        if self._split:
            n_half = self._split[0]
            w_lo = dist.all_reduce(self.agg[:n_half], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            self.g1b.replay()   # writes rows >= n_half only
            w_hi = dist.all_reduce(self.agg[n_half:], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            w_lo.wait()
            w_hi.wait()
        elif self._multi:
            dist.all_reduce(self.agg, op=dist.ReduceOp.SUM, group=self.group)
        self.g2.replay()
        if self._multi:
            dist.all_reduce(self.packed, op=dist.ReduceOp.SUM, group=self.group)
        n = self.h.numel()
        torch.add(self.gh_node, self.packed[:n].view_as(self.h), out=self.gh)

    def results(self):
        """(out, d/dh, edge-model parameter gradients, node-model parameter gradients) of the last run()."""
        return self.out, self.gh, _cut_views(self.packed, self._edge_shapes, self.h.numel()), list(self.views_n)


# ===================================================================================== partitioning B


def balanced_node_cuts(in_degree: torch.Tensor, world: int, boundaries=None):
    """W + 1 cut points of the node range such that every slice receives about E / W adjacencies (prefix sum of the
    in-degree): the edge stage is the expensive one, so slices are balanced by incoming edges, not by node count. A hub
    may leave a slice empty; cuts are non-decreasing and cover [0, N].
    boundaries (sorted node positions, e.g. the `ptr` of a collated batch of complexes): every inner cut moves to the
    nearest allowed position - no graph straddles two slices, so every adjacency has its source in the slice of its
    target and partition B exchanges nothing between layers (DstPlan.local_share == 1)."""
    n = int(in_degree.shape[0])
    if world == 1:
        return [0, n]
    csum = torch.cumsum(in_degree.to(torch.int64).cpu(), 0)
    total = int(csum[-1]) if n else 0
    if total == 0:
        return [node_bounds(n, world, r)[0] for r in range(world)] + [n]
    targets = torch.tensor([total * r // world for r in range(1, world)], dtype=torch.int64)
    inner = torch.searchsorted(csum, targets, right=False).tolist()   # first node whose prefix reaches the target
    cuts = [0] + [min(max(int(c), 0), n) for c in inner] + [n]
    if boundaries is not None:
        b = torch.as_tensor(boundaries, dtype=torch.int64).cpu().flatten()
        b = torch.unique(torch.cat([b, torch.tensor([0, n], dtype=torch.int64)]))
        for i in range(1, len(cuts) - 1):
            j = int(torch.searchsorted(b, torch.tensor(cuts[i])))
            lo, hi = int(b[max(j - 1, 0)]), int(b[min(j, len(b) - 1)])
            cuts[i] = lo if cuts[i] - lo <= hi - cuts[i] else hi
    for i in range(1, len(cuts)):
        cuts[i] = max(cuts[i], cuts[i - 1])
    return cuts


def locality_order(edge_index: torch.Tensor, n_nodes: int) -> torch.Tensor:
    """A node order for partition B on ONE large complex: reverse Cuthill-McKee over the (symmetrised) adjacency, so that
    the two ends of an adjacency get nearby numbers and contiguous node slices keep most sources local (the overlapped
    stack hides the exchange under exactly those edges). Returns perm with new_id = perm[old_id]; apply it to edge_index
    (perm[edge_index]) and scatter the node rows (h_new[perm] = h). Host-side, once per complex (scipy). Collated batches
    of small complexes need none of this: their nodes are grouped by graph already - cut at graph boundaries instead."""
    import numpy as np
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import reverse_cuthill_mckee
    ei = edge_index.detach().cpu().numpy()
    a = coo_matrix((np.ones(ei.shape[1], dtype=np.int8), (ei[0], ei[1])), shape=(n_nodes, n_nodes)).tocsr()
    order = reverse_cuthill_mckee((a + a.T).tocsr(), symmetric_mode=True)   # order[new] = old
    perm = np.empty(n_nodes, dtype=np.int64)
    perm[order] = np.arange(n_nodes, dtype=np.int64)
    return torch.from_numpy(perm)


def _world(group):
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group), dist.get_rank(group)
    return 1, 0


def _multi(group=None) -> bool:
    """True when the collectives have to be issued: a process group of more than one rank - or of ONE rank with
    CSMPN_FORCE_COLLECTIVES=1. The second form is the RCCL rehearsal of tests/test_sharded_gpu.py (round 4): a one-GPU box
    cannot hold two RCCL ranks, but with a world-size-1 `nccl` group every all_reduce / all_gather_into_tensor /
    reduce_scatter_tensor of this module is posted to RCCL exactly as it would be on N ranks (padded layouts included)."""
    if not (dist.is_available() and dist.is_initialized()):
        return False
    return dist.get_world_size(group) > 1 or os.environ.get("CSMPN_FORCE_COLLECTIVES", "0") == "1"


def _collective_device(group, fallback):
    """Device a small bookkeeping tensor must live on to go through the group's collectives: NCCL = RCCL moves device
    memory only (a CPU edge_index would otherwise fail in DstPlan / ShardPlan), gloo takes either."""
    if dist.is_available() and dist.is_initialized() and "nccl" in str(dist.get_backend(group)).lower():
        return torch.device("cuda", torch.cuda.current_device())
    return fallback


def _fused_collectives(group) -> bool:
    """The single-tensor collectives (all_gather_into_tensor / reduce_scatter_tensor) exist on NCCL = RCCL; gloo takes the
    list / all-reduce forms. Decided ONCE from the backend name: a per-call try / except would let a rank-local
    error (an OOM, an asynchronous failure) send one rank to a different collective than its peers."""
    return "nccl" in str(dist.get_backend(group)).lower()


class _Pending:
    """Handle of a collective in flight (async_op=True): wait() orders the current stream behind it, then runs the
    epilogue of the collective (gloo's reduce-scatter stand-in slices the all-reduced rows). The blocking forms go
    through wait() too; their work object is None."""

    def __init__(self, work, epilogue=None):
        self.work, self.epilogue = work, epilogue

    def wait(self):
        if self.work is not None:
            self.work.wait()
        if self.epilogue is not None:
            self.epilogue()


def _all_gather_rows(full, part, group, async_op=False):
    """full[W * n] <- concat over ranks of part[n] (rows). async_op=True: returns the _Pending to wait for."""
    if _fused_collectives(group):
        pending = _Pending(dist.all_gather_into_tensor(full, part, group=group, async_op=async_op))
    else:
        chunks = list(full.chunk(dist.get_world_size(group), dim=0))
        pending = _Pending(dist.all_gather(chunks, part, group=group, async_op=async_op))
    return pending if async_op else pending.wait()


def _reduce_scatter_rows(part, full, group, async_op=False):
    """part[n] <- this rank's row slice of the sum over ranks of full[W * n]. async_op=True: returns the _Pending."""
    if _fused_collectives(group):
        pending = _Pending(dist.reduce_scatter_tensor(part, full, op=dist.ReduceOp.SUM, group=group, async_op=async_op))
    else:   # gloo has no reduce-scatter: all-reduce and slice
        w, r = dist.get_world_size(group), dist.get_rank(group)
        pending = _Pending(dist.all_reduce(full, op=dist.ReduceOp.SUM, group=group, async_op=async_op),
                           lambda: part.copy_(full.chunk(w, dim=0)[r]))
    return pending if async_op else pending.wait()


def agree_all(local_ok: bool, group=None, device=None) -> bool:
    """True iff the condition holds on EVERY rank (all-reduce MIN of a flag). For choices that change which
    collectives a rank issues: they must come out the same everywhere, or the ranks post mismatched collectives."""
    if not _multi(group):
        return bool(local_ok)
    flag = torch.tensor([1 if local_ok else 0], dtype=torch.int32, device=device)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
    return int(flag.item()) == 1


class DstPlan:
    """Per-complex state of one rank for partitioning B: the edges into its node slice (global node ids), their ids in
    the caller's edge order (for edge_attr), the slice cuts of every rank (balanced by in-degree unless `balance=False`)
    and the index tables that move rows between the natural layout [N] and the padded layout [W * per] the
    equal-size collectives need (per = longest slice; pad rows read a zero row / are dropped)."""

    def __init__(self, edge_index, n_nodes, backend=ops.HipBackend, group=None, balance=True, max_pad=1.5, boundaries=None):
        self.world, self.rank = _world(group)
        self.multi = _multi(group)      # collectives are issued (world > 1, or the forced world-size-1 rehearsal)
        dev = edge_index.device
        dst = edge_index[1]
        if balance and self.world > 1:
            deg_all = torch.bincount(dst, minlength=n_nodes)
            self.cuts = balanced_node_cuts(deg_all, self.world, boundaries)
            # The collectives move the padded layout W x per (per = longest slice in NODES): on complexes whose in-degree
            # is skewed (vertex / edge / triangle rows) cuts by in-degree alone let per grow towards N. Bound it: no slice
            # longer than max_pad x N / W nodes (round-3 ADVICE) - the edge balance gives way first.
            cap = max(1, int(-(-n_nodes * max_pad // self.world)))
            if boundaries is None:   # (graph-aligned cuts stay where the graphs end)
                for r in range(1, self.world):          # left to right: a slice that is too long hands nodes to the next one
                    self.cuts[r] = min(self.cuts[r], self.cuts[r - 1] + cap)
                for r in range(self.world - 1, 0, -1):  # ... and right to left for the last slices
                    self.cuts[r] = max(self.cuts[r], self.cuts[r + 1] - cap)
        else:
            self.cuts = [node_bounds(n_nodes, self.world, r)[0] for r in range(self.world)] + [n_nodes]
        self.lo, self.hi = self.cuts[self.rank], self.cuts[self.rank + 1]
        self.per = max(1, max(self.cuts[r + 1] - self.cuts[r] for r in range(self.world)))
        self.pad_ratio = self.world * self.per / max(1, n_nodes)   # rows the collectives move / rows that exist
        mine = (dst >= self.lo) & (dst < self.hi)
        self.edge_ids = torch.nonzero(mine, as_tuple=False).squeeze(1)
        self.csr = backend.build_csr(edge_index[:, self.edge_ids].contiguous(), n_nodes)
        self.deg = self.csr.deg     # every edge into an owned node is local: the local in-degree is the global one
        self.n_nodes = n_nodes
        # The owned edges split by SOURCE locality (positions in the owned list): an edge whose source is owned too needs
        # no row of another rank - the layer's edge stage on these runs under the all-gather of the previous layer's
        # output, their d/dh stays out of the reduce-scatter (DstPartitionedStack(overlap=True))
        src_own = edge_index[0, self.edge_ids]
        loc = (src_own >= self.lo) & (src_own < self.hi)
        self.idx_loc = torch.nonzero(loc, as_tuple=False).squeeze(1)
        self.idx_rem = torch.nonzero(~loc, as_tuple=False).squeeze(1)
        # share of the owned adjacencies whose source row is owned too (1.0: the layer needs no row of another rank)
        self.local_share = float(self.idx_loc.numel()) / max(1, int(self.edge_ids.numel()))
        self._split = None
        self._backend = backend
        self._edge_index_owned = edge_index[:, self.edge_ids]
        # padded position of every node row / node row (or N = the zero row) of every padded position
        pos = torch.empty(n_nodes, dtype=torch.int64)
        src = torch.full((self.world * self.per,), n_nodes, dtype=torch.int64)
        for r in range(self.world):
            lo, hi = self.cuts[r], self.cuts[r + 1]
            pos[lo:hi] = torch.arange(r * self.per, r * self.per + (hi - lo))
            src[r * self.per: r * self.per + (hi - lo)] = torch.arange(lo, hi)
        self.pos_of_node = pos.to(dev)
        self.node_of_pos = src.to(dev)
        self.edges_per_rank = None
        if self.multi:   # a collective: plan() must be called on every rank of the group
            cnt = torch.zeros(self.world, dtype=torch.int64, device=_collective_device(group, dev))
            cnt[self.rank] = int(self.edge_ids.numel())
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
            self.edges_per_rank = cnt.tolist()

    def split(self):
        """(csr of the local-source edges, csr of the remote-source edges), built on first use."""
        if self._split is None:
            ei = self._edge_index_owned
            self._split = (self._backend.build_csr(ei[:, self.idx_loc].contiguous(), self.n_nodes),
                           self._backend.build_csr(ei[:, self.idx_rem].contiguous(), self.n_nodes))
        return self._split

    # ---- rows between the layouts (one index kernel each)
    def pad_slice(self, rows_loc):
        """[hi - lo, ...] -> [per, ...] (zero pad rows)."""
        n = self.hi - self.lo
        if n == self.per:
            return rows_loc.contiguous()
        out = rows_loc.new_zeros((self.per,) + tuple(rows_loc.shape[1:]))
        out[:n] = rows_loc
        return out

    def to_padded(self, rows_all):
        """[N, ...] -> [W * per, ...] (pad positions zero): the input layout of the reduce-scatter."""
        z = torch.cat([rows_all, rows_all.new_zeros((1,) + tuple(rows_all.shape[1:]))], dim=0)
        return z.index_select(0, self.node_of_pos)

    def from_padded(self, padded):
        """[W * per, ...] -> [N, ...]: the output layout of the all-gather."""
        return padded.index_select(0, self.pos_of_node)


class _Own:
    """What the stages of partitioning B read of this rank's slice: its bounds, the CSR of the owned edges, and the
    in-degree and node_attr rows of [lo, hi)."""

    def __init__(self, plan: DstPlan, node_attr):
        self.lo, self.hi, self.csr = plan.lo, plan.hi, plan.csr
        self.na = None if node_attr is None else node_attr[self.lo:self.hi].contiguous()
        self.deg = plan.deg[self.lo:self.hi].contiguous()


def _dst_node_forward(be, spec, own: _Own, x, agg, pn):
    """Node update of the owned slice -> (out_loc [hi - lo, ...], node state)."""
    lo, hi = own.lo, own.hi
    return be.node_forward(spec, own.deg, x[lo:hi].contiguous(), agg[lo:hi].contiguous(), own.na, pn)


def _dst_forward(be, spec, own: _Own, x, edge_attr, lp):
    """Forward of ONE destination-partitioned layer on this rank's slice, x [N, C, D] replicated in: edge stage on the
    owned edges, node update of the owned nodes -> (agg, out_loc, (edge state, node state)). No collective."""
    pe, pn = _split_params(spec, lp)
    agg, st_e = be.edge_forward(spec, own.csr, x, edge_attr, pe)      # complete on [lo, hi)
    out_loc, st_n = _dst_node_forward(be, spec, own, x, agg, pn)
    return agg, out_loc, (st_e, st_n)


def _dst_node_backward(be, spec, own: _Own, x, agg, pn, g_loc, want_gna, st_n):
    """Node backward on the slice, g_loc = d/d(output slice) -> (d/dh of the node stage [hi - lo], d/d agg [N] (zero
    outside the slice), d/d node_attr of the slice, node-model parameter gradients)."""
    lo, hi = own.lo, own.hi
    gh_node, g_agg_loc, g_na_loc, views_n = be.node_backward(
        spec, own.deg, x[lo:hi].contiguous(), agg[lo:hi].contiguous(), own.na, pn, g_loc, want_gna, st_n)
    g_agg = torch.zeros_like(agg)
    g_agg[lo:hi] = g_agg_loc
    return gh_node, g_agg, g_na_loc, views_n


def _dst_backward(be, spec, own: _Own, x, agg, edge_attr, lp, g_loc, want, st):
    """Backward of ONE destination-partitioned layer up to its collectives. want = (d/d edge_attr?, d/d node_attr?),
    st = what _dst_forward returned. -> (d/dh of the node stage [hi - lo], d/dh of the edge stage [N]: rows of any rank,
    d/d edge_attr, d/d node_attr of the slice, the layer's parameter gradients in flat_params() order)."""
    pe, pn = _split_params(spec, lp)
    gh_node, g_agg, g_na_loc, views_n = _dst_node_backward(be, spec, own, x, agg, pn, g_loc, want[1], st[1])
    gh_edge = torch.zeros_like(x)          # +g -> owned targets, -g -> any source
    g_ea, views_e = be.edge_backward(spec, own.csr, x, edge_attr, pe, g_agg, gh_edge, want[0], st[0])
    return gh_node, gh_edge, g_ea, g_na_loc, list(views_e) + list(views_n)


def _all_gather_slices(plan: DstPlan, rows_loc, group):
    """[hi - lo, ...] of every rank -> [N, ...] replicated (through the padded layout)."""
    padded = rows_loc.new_empty((plan.world * plan.per,) + tuple(rows_loc.shape[1:]))
    _all_gather_rows(padded, plan.pad_slice(rows_loc), group)
    return plan.from_padded(padded)


class _DstPartStackFn(torch.autograd.Function):
    """L chained EGCL layers, destination-partitioned. h [N, C, D] replicated in, the last layer's output replicated out.
    Forward, per layer: edge stage on the owned edges -> node update of the owned slice -> ONE all-gather. Backward, per
    layer: node backward on the slice -> edge backward on the owned edges -> ONE reduce-scatter of d/dh, whose result
    (+ the node stage's d/dh) is exactly the slice of d/d(previous layer's output) the next step needs - no all-gather
    between chained layers; the replicated d/dh of the chain's input is all-gathered once, if anybody asks for it. The
    parameter gradients of all layers travel in ONE all-reduce.

    overlap=True (world > 1) hides the collectives of the chain under edge work. Every layer's edge stage runs in two
    launches: the owned edges whose source is owned too (they read rows of the own slice only) and the rest.
    Forward: the all-gather of layer k's output slice is in flight while layer k + 1 runs its local-source edges on the
    slice it already has; the remote-source edges follow the wait. Backward: the remote-source edges go first, the
    reduce-scatter of THEIR d/dh (the only part with rows of other ranks) travels while the local-source edges run; the
    local part lands on owned rows and is added behind the wait. Same results as the blocking chain up to the order of
    two float additions per row. The two forms differ in the edge launches and in where the collectives are waited for,
    and in nothing else."""

    @staticmethod
    def forward(ctx, h, edge_attr_local, node_attr, specs, plan: DstPlan, backend, group, counts, overlap, *params):
        lo, hi = plan.lo, plan.hi
        eas = (edge_attr_local,)
        if overlap:
            csr_l, csr_r = plan.split()
            eas = tuple(None if edge_attr_local is None else edge_attr_local.index_select(0, idx)
                        for idx in (plan.idx_loc, plan.idx_rem))
        own = _Own(plan, node_attr)
        offs = _offsets(counts)
        hs, aggs, st = [], [], []
        x = h.contiguous()
        pending, padded, x_own = None, None, None
        for k, spec in enumerate(specs):
            lp = params[offs[k]:offs[k + 1]]
            if overlap:
                pe, pn = _split_params(spec, lp)
                # rows outside [lo, hi) of x_own are never read by the local-source edges
                agg_l, st_l = backend.edge_forward(spec, csr_l, x if pending is None else x_own, eas[0], pe)
                if pending is not None:
                    pending.wait()
                    x = plan.from_padded(padded)
                agg_r, st_r = backend.edge_forward(spec, csr_r, x, eas[1], pe)
                agg = agg_l + agg_r                                                   # complete on [lo, hi)
                out_loc, st_n = _dst_node_forward(backend, spec, own, x, agg, pn)
                st_k = ((st_l, st_r), st_n)
            else:
                agg, out_loc, st_k = _dst_forward(backend, spec, own, x, eas[0], lp)
            hs.append(x); aggs.append(agg); st.append(st_k)
            if overlap:
                padded = out_loc.new_empty((plan.world * plan.per,) + tuple(out_loc.shape[1:]))
                pending = _all_gather_rows(padded, plan.pad_slice(out_loc), group, async_op=True)
                x_own = out_loc.new_zeros((plan.n_nodes,) + tuple(out_loc.shape[1:]))
                x_own[lo:hi] = out_loc
            else:
                x = _all_gather_slices(plan, out_loc, group) if plan.multi else out_loc
        if overlap:
            pending.wait()
            x = plan.from_padded(padded)
        ctx.st = st
        ctx.specs, ctx.plan, ctx.backend, ctx.group, ctx.overlap = specs, plan, backend, group, overlap
        _save(ctx, hs + aggs, [*eas, node_attr], params, counts)
        return x

    @staticmethod
    def backward(ctx, gout):
        specs, plan, backend, group, overlap, offs = ctx.specs, ctx.plan, ctx.backend, ctx.group, ctx.overlap, ctx.offs
        L = len(specs)
        saved, (*eas, node_attr), params = _restore(ctx)
        hs, aggs = saved[:L], saved[L:]
        lo, hi = plan.lo, plan.hi
        if overlap:
            csr_l, csr_r = plan.split()
        own = _Own(plan, node_attr)
        want = ctx.needs_input_grad[1:3]
        g_loc = gout[lo:hi].contiguous()          # d/d(output slice) of the layer being processed
        views_all = [None] * len(params)
        g_ea_total, g_na_loc_total = [None] * len(eas), None      # d/d edge_attr: one total per edge launch
        gh_full_single = None
        for k in range(L - 1, -1, -1):
            spec, h, agg = specs[k], hs[k], aggs[k]
            lp = params[offs[k]:offs[k + 1]]
            if overlap:
                pe, pn = _split_params(spec, lp)
                (st_l, st_r), st_n = ctx.st[k]
                gh_node, g_agg, g_na_loc, views_n = _dst_node_backward(backend, spec, own, h, agg, pn, g_loc, want[1], st_n)
                gh_r = torch.zeros_like(h)             # +g -> owned targets, -g -> sources on OTHER ranks
                g_ea_r, views_r = backend.edge_backward(spec, csr_r, h, eas[1], pe, g_agg, gh_r, want[0], st_r)
                g_pad = gh_r.new_empty((plan.per,) + tuple(gh_r.shape[1:]))
                pending = _reduce_scatter_rows(g_pad, plan.to_padded(gh_r), group, async_op=True)
                gh_l = torch.zeros_like(h)             # both ends owned: rows of [lo, hi) only
                g_ea_l, views_l = backend.edge_backward(spec, csr_l, h, eas[0], pe, g_agg, gh_l, want[0], st_l)
                g_eas = (g_ea_l, g_ea_r)
                views = [_acc(a, b) for a, b in zip(views_l, views_r)] + list(views_n)
            else:
                gh_node, gh_edge, g_ea, g_na_loc, views = _dst_backward(backend, spec, own, h, agg, eas[0], lp, g_loc,
                                                                        want, ctx.st[k])
                g_eas = (g_ea,)
            for i, v in enumerate(views):
                views_all[offs[k] + i] = v
            g_ea_total = [_acc(t, g) for t, g in zip(g_ea_total, g_eas)]
            g_na_loc_total = _acc(g_na_loc_total, g_na_loc)
            if overlap:
                pending.wait()
                g_loc = g_pad[:hi - lo] + gh_l[lo:hi] + gh_node
            elif plan.multi:
                g_pad = gh_edge.new_empty((plan.per,) + tuple(gh_edge.shape[1:]))
                _reduce_scatter_rows(g_pad, plan.to_padded(gh_edge), group)
                g_loc = g_pad[:hi - lo] + gh_node
            else:
                gh_edge[lo:hi] += gh_node
                gh_full_single = gh_edge
                g_loc = gh_edge[lo:hi]
        gh = None
        if ctx.needs_input_grad[0]:
            gh = _all_gather_slices(plan, g_loc, group) if plan.multi else gh_full_single
        g_ea = g_ea_total[0]
        if overlap and any(t is not None for t in g_ea_total):     # the two launches' rows back in the caller's order
            ref = g_ea_total[0] if g_ea_total[0] is not None else g_ea_total[1]
            g_ea = ref.new_zeros((plan.edge_ids.numel(),) + tuple(ref.shape[1:]))
            for idx, t in zip((plan.idx_loc, plan.idx_rem), g_ea_total):
                if t is not None:
                    g_ea[idx] = t
        g_na = g_na_loc_total
        if plan.multi:
            _, views_all = _all_reduce_views(views_all, group)
            if g_na_loc_total is not None:
                g_na = torch.zeros_like(node_attr)
                g_na[lo:hi] = g_na_loc_total
                dist.all_reduce(g_na, op=dist.ReduceOp.SUM, group=group)
        return (gh, g_ea, g_na, None, None, None, None, None, None, *views_all)


class _DstPartitioned(torch.nn.Module):
    """Partitioning B behind a module: `plan(edge_index, n_nodes)` takes the WHOLE edge list (replicated topology);
    forward takes the whole h / node_attr and this rank's rows of edge_attr (`edge_attr[plan.edge_ids]`) and runs the
    layers of `self._chain()` as one destination-partitioned chain."""

    def __init__(self, backend, group, balance, overlap=False):
        super().__init__()
        self.backend = backend
        self.group = group
        self.balance = balance
        self.overlap = overlap     # collectives in flight under the local-source edges

    def plan(self, edge_index, n_nodes, boundaries=None) -> DstPlan:
        """boundaries: allowed cut positions (the `ptr` of a collated batch): graphs stay whole, see balanced_node_cuts."""
        return DstPlan(edge_index, n_nodes, self.backend, self.group, balance=self.balance, boundaries=boundaries)

    def forward(self, h, plan: DstPlan, edge_attr_local=None, node_attr=None):
        layers = self._chain()
        lps = [_layer_params(layer) for layer in layers]
        specs, counts = tuple(layer.spec() for layer in layers), tuple(len(lp) for lp in lps)
        return _DstPartStackFn.apply(h, edge_attr_local, node_attr, specs, plan, self.backend, self.group, counts,
                                     bool(self.overlap and plan.multi), *[p for lp in lps for p in lp])


class DstPartitionedEGCL(_DstPartitioned):
    """Wraps ONE EGCL module (partitioning B): the chain of one layer."""

    def __init__(self, layer, backend=ops.HipBackend, group=None, balance=True):
        super().__init__(backend, group, balance)
        self.layer = layer

    def _chain(self):
        return [self.layer]


class DstPartitionedStack(_DstPartitioned):
    """L chained EGCL layers on ONE destination partition of the complex: h stays resident, every
    layer costs one all-gather forward and one reduce-scatter backward, the parameter gradients of all layers one
    all-reduce. All layers share edge_attr / node_attr, as the reference's models do (hulls_cssmpnn.py:89-94).
    overlap=True: the collectives travel under the edges whose source is owned too (two edge launches per stage)."""

    def __init__(self, layers, backend=ops.HipBackend, group=None, balance=True, overlap=False):
        super().__init__(backend, group, balance, overlap)
        self.layers = torch.nn.ModuleList(layers)

    def _chain(self):
        return list(self.layers)


class GraphedDstStep:
    """Forward + backward of the destination-partitioned layer on fixed buffers (multi-GPU benchmark):
    [graph 1: edge forward on the owned targets, node forward on the owned nodes, slice padded] -> all-gather(out)
    -> [graph 2: rows back to the natural layout, node backward, edge backward, d/dh rows to the padded layout] ->
    reduce-scatter(d/dh) + all-reduce(parameter gradients). `compute_only=True` skips the collectives (the
    compute-only rate of the bench). World size 1: no padded-layout copies at all."""

    def __init__(self, part: "DstPartitionedEGCL", plan: DstPlan, h, edge_attr_local, node_attr, gout):
        layer, be = part.layer, part.backend
        self.group, self.plan = part.group, plan
        self.spec = spec = layer.spec()
        lp = _layer_params(layer)
        self.h = h_ = h.detach()
        self._multi = plan.multi
        own = _Own(plan, node_attr)
        gout_loc = gout[plan.lo:plan.hi].contiguous()
        self.out_all = h_.new_empty((plan.world * plan.per,) + tuple(h_.shape[1:]))   # all-gather target (padded layout)

        def part1():
            agg, out_loc, st = _dst_forward(be, spec, own, h_, edge_attr_local, lp)
            return agg, st, plan.pad_slice(out_loc)

        def part2(agg, st):
            out = plan.from_padded(self.out_all) if self._multi else None   # the layer's replicated output
            gh_node, gh_edge, _g_ea, _g_na, views = _dst_backward(be, spec, own, h_, agg, edge_attr_local, lp, gout_loc,
                                                                   (False, False), st)
            return gh_node, gh_edge, plan.to_padded(gh_edge) if self._multi else None, _pack(views), out

        capture = _Capture(lambda: part2(*part1()[:2]))
        self.g1, (self.agg, self._st, self.out_pad) = capture(part1)
        self.g2, (self.gh_node, self.gh_edge, self.gh_pad, self.flat, self.out) = capture(lambda: part2(self.agg, self._st))
        self.gh_rs = h_.new_empty((plan.per,) + tuple(h_.shape[1:]))   # reduce-scatter target: this rank's padded slice
        self.gh_loc = torch.empty_like(self.gh_node)
        self.bytes_per_step = 0
        if self._multi:
            w = plan.world
            # bytes every rank sends per step: all-gather and reduce-scatter move (W-1)/W of the padded tensor
            self.bytes_per_step = int(2 * w * plan.per * h_[0].numel() * 4 * (w - 1) / w + 2 * self.flat.numel() * 4 * (w - 1) / w)

    def run(self, compute_only=False):
        self.g1.replay()
        if self._multi and not compute_only:
            _all_gather_rows(self.out_all, self.out_pad, self.group)
        self.g2.replay()
        n = self.plan.hi - self.plan.lo
        if self._multi and not compute_only:
            _reduce_scatter_rows(self.gh_rs, self.gh_pad, self.group)
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
            torch.add(self.gh_rs[:n], self.gh_node, out=self.gh_loc)
        else:
            torch.add(self.gh_edge[self.plan.lo:self.plan.hi], self.gh_node, out=self.gh_loc)


class GraphedDstStackStep:
    """Forward + backward of L chained destination-partitioned layers on fixed buffers, h resident:
    2 L HIP graphs with one collective between consecutive graphs and nothing else on the host -
      forward  k = 0 .. L-1:  [rows of layer k's input back from the padded layout (k > 0), edge forward on the owned
                               edges, node forward on the owned slice, slice padded]  -> all-gather
      backward k = L-1 .. 0:  [d/d(output slice) = reduce-scattered rows + the node stage's d/dh of layer k + 1, node
                               backward, edge backward, d/dh rows to the padded layout] -> reduce-scatter
    and ONE all-reduce of the parameter gradients of all layers at the end. `out` = the replicated output of the last
    layer, `gh_loc` = this rank's slice of d/dh, `flat` = the parameter gradients (layer by layer, edge model then
    node model, in flat_params() order). World size 1: the collectives are copies."""

    def __init__(self, stack: "DstPartitionedStack", plan: DstPlan, h, edge_attr_local, node_attr, gout):
        be, self.group, self.plan = stack.backend, stack.group, plan
        layers = list(stack.layers)
        self.L = L = len(layers)
        specs = [l.spec() for l in layers]
        lps = [_layer_params(l) for l in layers]
        n = plan.hi - plan.lo
        self._multi = plan.multi
        h0 = h.detach().contiguous()
        own = _Own(plan, node_attr)
        gout_loc = gout[plan.lo:plan.hi].contiguous()
        row = tuple(h0.shape[1:])
        self.out_all = [h0.new_empty((plan.world * plan.per,) + row) for _ in range(L)]   # all-gather targets
        self.gh_rs = [h0.new_empty((plan.per,) + row) for _ in range(L)]                  # reduce-scatter targets

        def fwd(k):     # -> (x, agg, states, padded output slice)
            x = h0 if k == 0 else plan.from_padded(self.out_all[k - 1])
            agg, out_loc, st = _dst_forward(be, specs[k], own, x, edge_attr_local, lps[k])
            return x, agg, st, plan.pad_slice(out_loc)

        def bwd(k, x, agg, st, gh_node_next):     # -> (d/dh of the node stage, padded d/dh of the edge stage, gradients)
            g_loc = gout_loc if k == L - 1 else self.gh_rs[k + 1][:n] + gh_node_next
            gh_node, gh_edge, _g_ea, _g_na, views = _dst_backward(be, specs[k], own, x, agg, edge_attr_local, lps[k], g_loc,
                                                                   (False, False), st)
            return gh_node, plan.to_padded(gh_edge), _pack(views)

        def gather(k, pad):
            if self._multi:
                _all_gather_rows(self.out_all[k], pad, self.group)
            else:
                self.out_all[k].copy_(pad)

        def scatter(k, pad):
            if self._multi:
                _reduce_scatter_rows(self.gh_rs[k], pad, self.group)
            else:
                self.gh_rs[k].copy_(pad)
        self._gather, self._scatter = gather, scatter

        def chain(segment):
            """The 2 L segments in step order, each through `segment` (which runs it plainly, or captures it) and
            followed by its collective, so that the next segment reads a buffer of the right content."""
            self.gf, self.gb = [None] * L, [None] * L
            self._st, self._bw = [None] * L, [None] * L
            for k in range(L):
                self.gf[k], self._st[k] = segment(lambda: fwd(k))
                gather(k, self._st[k][3])
            ghn = None
            for k in range(L - 1, -1, -1):
                self.gb[k], self._bw[k] = segment(lambda: bwd(k, *self._st[k][:3], ghn))
                ghn = self._bw[k][0]
                scatter(k, self._bw[k][1])

        capture = _Capture(lambda: chain(lambda fn: (None, fn())))     # warm-up: no graph
        chain(capture)
        self.flat = torch.cat([self._bw[k][2] for k in range(L)])
        self.gh_loc = torch.empty_like(self._bw[0][0])
        self.out = None
        self.bytes_per_step = 0
        if self._multi:
            w = plan.world
            self.bytes_per_step = int(L * 2 * w * plan.per * h0[0].numel() * 4 * (w - 1) / w + 2 * self.flat.numel() * 4 * (w - 1) / w)

    def run(self):
        L, n = self.L, self.plan.hi - self.plan.lo
        for k in range(L):
            self.gf[k].replay()
            self._gather(k, self._st[k][3])
        for k in range(L - 1, -1, -1):
            self.gb[k].replay()
            self._scatter(k, self._bw[k][1])
        torch.add(self.gh_rs[0][:n], self._bw[0][0], out=self.gh_loc)
        torch.cat([self._bw[k][2] for k in range(L)], out=self.flat)
        if self._multi:
            dist.all_reduce(self.flat, op=dist.ReduceOp.SUM, group=self.group)
        self.out = self.plan.from_padded(self.out_all[L - 1])
