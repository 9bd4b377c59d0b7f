"""Whole-model training step replayed from ONE HIP graph (multi-layer step).

A step of the reference's trainer (engineer/trainer/trainer.py:204-227) is
    optimizer.zero_grad(); loss, _ = model(batch); loss.backward(); optimizer.step()
i.e. for the hulls model ~3 x 4 fused CEMLP launches between ~150 small PyTorch launches (embedding
gathers, attribute concatenation, pooling, Adam). On complexes of the reference's sizes (a few thousand
simplices per batch) the GPU work of a step is shorter than the host time to launch it, so the step is
launch-bound. For batches of FIXED topology (same complexes, new vertex features / targets: MD17
trajectories of one molecule, repeated epochs over cached batches) this module captures the whole step -
embedding, every EGCL layer forward and backward, readout, loss and the optimizer update - once and replays
it; per step the host copies the new features into the captured buffers and launches one graph.

Batches of CHANGING topology (a shuffled training loop: another complex in every batch) replay the same graph when the
step is built with a `capacity` (csmpn.data.complexes.BatchCapacity): every batch is padded to the capacity's shapes on the
host (pad_batch: filler simplices and self-loop adjacencies that no real row hears of), copied into the captured buffers,
and the tables derived from the topology - the target-sorted CSR, the index tables of the embedding and of the readout -
are rebuilt in place on the device (SimplicialBatch.refresh_: csmpn_simplex_tables, csmpn_csr_build) in front of the replay.
Where the complex is the Vietoris-Rips complex of the current positions, step(points=...) builds it on the device as well
(SimplicialBatch.relift_: csmpn_rips_lift writes the structure tensors at the capacity), so a step takes no host lift at all;
step(points=..., knn=k) does the same for the clique complex of the k-nearest-neighbour graph (csmpn_knn_lift), and
step(points=..., hull=True) for the convex-hull complex with the hull's volume as the target (csmpn_hull_lift), and
step(points=..., edges=list | knn=k, edge_th=..., tri_th=...) for the thresholded clique complex of a listed graph or of the
k-nearest-neighbour graph (csmpn_clique_lift).

The kernels launched inside are the same C-ABI calls as in eager mode (they take the current stream); the
CSR and the embedding index tables are built before capture (their only host round trips).
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch


LIFT_STATUS_SHIFT = 8     # status(): the word of the device lift sits above the bits of the table rebuild


def flatten_parameters(module: torch.nn.Module) -> torch.nn.Parameter:
    """Re-homes the module's trainable float32 parameters - and their .grad - as views of ONE flat buffer each and returns the
    flat parameter (its .grad is the flat gradient buffer). An optimizer built over `[flat]` then updates every parameter of
    the module with ONE fused launch and zeroes all gradients with one fill: the task models carry 700-1 100 small parameter
    tensors (226 per EGCL layer), which torch's multi-tensor Adam walks in 5-7 launches of ~9 us each, its zero_grad in 3.
    Names, shapes and state_dict() of the module are unchanged (the parameters stay the module's own objects; only their
    storage moves). Elementwise optimizers only (Adam, SGD, ...): per-tensor statistics would see one tensor.

    ZEROING THE GRADIENTS: the aliasing lives in the .grad attributes. `optimizer.zero_grad()` / `module.zero_grad()` with
    PyTorch's default `set_to_none=True` REPLACE them - the optimizer then sees `flat.grad is None` and skips the only
    parameter it has while the module's gradients accumulate elsewhere: training stops silently. Use
    `zero_flat_grad(flat)` (one fill) or `zero_grad(set_to_none=False)`; `flat_gradients_intact(flat)` tells whether the
    views still alias (GraphedTrainStep checks it before it captures)."""
    params = [p for p in module.parameters() if p.requires_grad]
    if not params:
        raise ValueError("module has no trainable parameters")
    dev, dt = params[0].device, params[0].dtype
    if any(p.device != dev or p.dtype != dt for p in params):
        raise ValueError("flatten_parameters: all trainable parameters must share device and dtype")
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4      # 16-byte aligned starts
    flat = torch.zeros(total, dtype=dt, device=dev)
    gflat = torch.zeros(total, dtype=dt, device=dev)
    with torch.no_grad():
        for p, o in zip(params, offs):
            n = p.numel()
            flat[o:o + n].copy_(p.detach().reshape(-1))
            if p.grad is not None:
                gflat[o:o + n].copy_(p.grad.reshape(-1))
            p.data = flat[o:o + n].view(p.shape)
            p.grad = gflat[o:o + n].view(p.shape)
    flat_param = torch.nn.Parameter(flat)
    flat_param.grad = gflat
    flat_param._csmpn_flat = (gflat, params, offs)
    return flat_param


def zero_flat_grad(flat_param: torch.nn.Parameter) -> None:
    """Zero every gradient of a flatten_parameters() module with one fill, keeping the views (the safe zero_grad)."""
    flat_param._csmpn_flat[0].zero_()


def flat_gradients_intact(flat_param: torch.nn.Parameter) -> bool:
    """True while flat.grad is the flat gradient buffer and every parameter's .grad is still its view of it (False after a
    zero_grad(set_to_none=True) on the optimizer or the module)."""
    gflat, params, offs = flat_param._csmpn_flat
    if flat_param.grad is not gflat:
        return False
    esz = gflat.element_size()
    return all(p.grad is not None and p.grad.data_ptr() == gflat.data_ptr() + o * esz for p, o in zip(params, offs))


class GraphedTrainStep:
    """step(features) -> loss (a device scalar that the next replay overwrites).

    model(batch) must return (loss, aux) like the reference's task models; `optimizer` must be
    graph-capturable (torch.optim.Adam(..., capturable=True)); `batch` is a device SimplicialBatch
    whose tensors become the captured input buffers. `feature_names`: the batch attributes that change
    from step to step (everything else - topology, types - is part of the captured graph).

    capacity (a csmpn.data.complexes.BatchCapacity, e.g. capacity_of(batches, slack)): the step serves batches of any
    topology that fits. `batch` (CPU or device, padded or not) is padded to the capacity and moved to `device` (default: the
    batch's own if it is a GPU, else the current one); `simplex_features` names its per-simplex tensors, which get zero
    filler rows (default: those of `feature_names` with one row per simplex). step(batch=collated_cpu_batch) then pads that
    batch (ValueError BEFORE anything is launched if it does not fit or its indices are out of range - run it eagerly),
    refreshes the captured batch in place and replays. The refresh runs eagerly on the current stream in front of the
    replay; it is not part of the captured graph. status(): the device status word of the table rebuild (0 = every batch
    so far had the row counts of the capacity; one small copy with a synchronisation - read it where the loop syncs
    anyway).

    step(points=device points [B * V, n], vertex_features={name: per-vertex tensor}) lifts the Vietoris-Rips complexes of the
    points at threshold `rips_dis` (or dis=...) ON THE DEVICE into the captured batch (SimplicialBatch.relift_:
    csmpn_rips_lift + the same in-place rebuild), eagerly in front of the replay like the refresh; the per-simplex tensors
    named in vertex_features get the given rows at the new vertex rows and zeros elsewhere. Nothing is checked on the host:
    a complex over the capacity leaves the previous structure in place and sets bits in status(). With `knn` (the step's
    default, as `rips_dis` is for dis) or knn=... in the call, the complexes are the clique complexes of the
    k-nearest-neighbour graphs instead (csmpn.data.complexes.knn_clique_complex; csmpn_knn_lift). A threshold AND a k, as
    defaults or in one call, are a ValueError; a call that names one of the two does not read the defaults. `hull=True` (as a
    default or in the call) is the third choice under the same rules: the convex-hull complexes of the points
    (hull_complex(method="exact"); csmpn_hull_lift), with the points as the vertex feature `input` and the hulls' volumes
    written into `target` where the batch has these tensors - a hulls step from nothing but device points.

    `edges=True` (or an int: the columns of the list buffer; True = every ordered pair of every graph) is the fourth choice:
    step(points=..., edges=int64 [2, n] of GLOBAL vertex ids) lifts the thresholded clique complexes of the listed graph
    (csmpn.data.complexes.clique_complex; csmpn_clique_lift). The list is copied into ONE static device buffer behind a fill of
    (-1, -1) padding, so lists of changing length replay through the same addresses. `edge_th` / `tri_th` (defaults of the step,
    or in the call; +infinity where neither names one) go with edges or knn: a k with a threshold lifts the thresholded
    cliques of the k-nearest-neighbour graph through the same entry; with dis or hull they are a ValueError. A list with an end
    outside the batch or across two graphs leaves the batch as it was and shows as bit 5 of the lift's word in status().

    A `batch` built by csmpn.data.complexes.cloud_batch_device (the Rips complexes of point clouds of up to 4096 vertices per
    graph; csmpn_cloud_lift) is taken as it is - it lives on the device at `capacity` already, and its plan says which lift
    re-lifts it: step(points=..., dis=...) is the only device lift of such a step; knn, hull, edges and the thresholds are a
    ValueError there. A batch of knn_cloud_batch_device (the clique complexes of their k-nearest-neighbour graphs;
    csmpn_cloud_knn_lift) is taken the same way: step(points=..., knn=k), or the step's `knn`, is its only device lift."""

    hull = False
    edges = False
    edge_th = tri_th = None
    _edge_buffer = None

    def __init__(self, model, optimizer, batch, feature_names: Iterable[str], warmup: int = 2, max_dim: Optional[int] = None,
                 capacity=None, simplex_features: Optional[Iterable[str]] = None, device=None, rips_dis: Optional[float] = None,
                 knn: Optional[int] = None, hull: bool = False, edges=False, edge_th: Optional[float] = None,
                 tri_th: Optional[float] = None):
        if (rips_dis is not None) + (knn is not None) + bool(hull) + bool(edges) > 1:
            raise ValueError("GraphedTrainStep: rips_dis (Rips), knn (k-nearest-neighbour cliques), hull (convex hulls) and edges "
                             "(the thresholded cliques of a listed graph) exclude each other")
        if (edge_th is not None or tri_th is not None) and (rips_dis is not None or hull):
            raise ValueError("GraphedTrainStep: edge_th / tri_th go with edges or knn, not with rips_dis or hull")
        self.capacity = capacity
        self.simplex_features = None
        self.rips_dis, self.knn, self.hull = rips_dis, knn, bool(hull)
        self.edges, self.edge_th, self.tri_th = edges, edge_th, tri_th
        if capacity is not None:
            from csmpn.data.complexes import pad_batch
            if device is None:
                device = batch.edge_index.device if batch.edge_index.is_cuda else torch.device("cuda", torch.cuda.current_device())
            if simplex_features is None:
                rows = int(batch.node_types.shape[0])
                simplex_features = [k for k in feature_names if hasattr(batch, k) and getattr(batch, k).dim() >= 1
                                    and int(getattr(batch, k).shape[0]) == rows]
            self.simplex_features = tuple(simplex_features)
            batch_plan = getattr(batch, "_plan", None) or {}
            if batch_plan.get("cloud") is not None or batch_plan.get("cloud_knn") is not None:
                # a batch of cloud_batch_device or knn_cloud_batch_device is on the device at its capacity already, and its plan
                # says which lift re-lifts it (csmpn_cloud_lift / csmpn_cloud_knn_lift: more than 64 vertices per graph) -
                # padding would make a plain batch of it
                if int(batch.node_types.shape[0]) != capacity.rows or int(batch.edge_index.shape[1]) != capacity.edges:
                    raise ValueError("GraphedTrainStep: the cloud batch was not built at `capacity`")
            else:
                batch = pad_batch(batch, capacity, self.simplex_features).to(device)
        dev = batch.edge_index.device
        if dev.type != "cuda":
            raise RuntimeError("GraphedTrainStep needs a device batch (no CPU fallback)")
        self.model, self.optimizer, self.batch = model, optimizer, batch
        self.feature_names = list(feature_names)
        for name in self.feature_names:
            if not hasattr(batch, name):
                raise AttributeError(f"batch has no feature {name!r}")
        batch.plan(getattr(model, "max_dim", 2) if max_dim is None else max_dim)
        batch.csr()
        # warm-up steps run eagerly on a side stream (allocator pools, lazily built workspaces, Adam state
        # tensors); parameters and optimizer state are restored afterwards, so the first replayed step is
        # step 1 of the trajectory
        params = [p for g in optimizer.param_groups for p in g["params"]]
        for p in params:
            if hasattr(p, "_csmpn_flat") and not flat_gradients_intact(p):
                raise RuntimeError("flatten_parameters(): the gradient views no longer alias the flat buffer (a zero_grad with "
                                   "set_to_none=True ran?) - the optimizer would skip every update; use zero_flat_grad()")
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        saved_params = [p.detach().clone() for p in params]
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(max(warmup, 1)):
                self._eager_step()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        with torch.no_grad():
            for p, s in zip(params, saved_params):
                p.copy_(s)
            # optimizer state (exp_avg, exp_avg_sq, step) exists now: reset it in place, the captured
            # graph updates these very tensors
            for st in optimizer.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()
        if capacity is not None:
            # every table the models have added to the plan exists now: one refresh onto itself allocates the workspaces of
            # the in-place rebuild and leaves the tables as the rebuild writes them - the state every later step starts from
            batch.refresh_(batch)
            torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.aux = self._eager_step()
        if edges:
            self._edge_list_buffer(None)
        # the capture itself executes nothing: parameters and optimizer state are still those of step 0

    def _eager_step(self):
        self.optimizer.zero_grad(set_to_none=False)
        loss, aux = self.model(self.batch)
        loss.backward()
        self.optimizer.step()
        return loss, aux

    def load(self, features: Dict[str, torch.Tensor]):
        """Copy new feature tensors (same shapes) into the captured buffers."""
        for name, value in features.items():
            if name not in self.feature_names:
                raise KeyError(f"{name!r} was not declared as a changing feature")
            getattr(self.batch, name).copy_(value, non_blocking=True)

    def load_batch(self, batch):
        """Pad `batch` (collated, CPU or device) to the capacity and make the captured batch hold it. ValueError - before
        anything is launched - if it does not fit or its indices are out of range."""
        if self.capacity is None:
            raise RuntimeError("GraphedTrainStep was built without a capacity: it replays ONE topology (load(features))")
        from csmpn.data.complexes import pad_batch
        self.batch.refresh_(pad_batch(batch, self.capacity, self.simplex_features))

    def _edge_list_buffer(self, edges: Optional[torch.Tensor]) -> torch.Tensor:
        """The static list buffer [2, columns] (allocated on first use: `edges` of the constructor as an int, else every ordered
        pair of every graph), filled with (-1, -1) and then with `edges` (None: the buffer as it is)."""
        plan = self.batch._plan
        if self._edge_buffer is None:
            B, V = self.batch.num_graphs, int(plan["rows"][0].shape[0]) // self.batch.num_graphs
            columns = B * V * (V - 1) if self.edges is True or not self.edges else int(self.edges)
            self._edge_buffer = torch.full((2, max(columns, 1)), -1, dtype=torch.int64, device=self.batch.x_ind.device)
        if edges is None:
            return self._edge_buffer
        if edges.dtype != torch.int64 or edges.dim() != 2 or int(edges.shape[0]) != 2:
            raise ValueError(f"step(points=..., edges=...): the list must be an int64 tensor [2, n], got {edges.dtype} {tuple(edges.shape)}")
        if int(edges.shape[1]) > int(self._edge_buffer.shape[1]):
            raise ValueError(f"step(points=..., edges=...): {int(edges.shape[1])} entries, the list buffer holds "
                             f"{int(self._edge_buffer.shape[1])} (GraphedTrainStep(edges=columns))")
        self._edge_buffer.fill_(-1)
        self._edge_buffer[:, :int(edges.shape[1])].copy_(edges, non_blocking=True)
        return self._edge_buffer

    def load_points(self, points: torch.Tensor, dis: Optional[float] = None, vertex_features: Optional[Dict[str, torch.Tensor]] = None,
                    knn: Optional[int] = None, hull: Optional[bool] = None, edges: Optional[torch.Tensor] = None,
                    edge_th: Optional[float] = None, tri_th: Optional[float] = None):
        """Make the captured batch hold the Vietoris-Rips complexes of the device points [B * V, n] at threshold `dis`
        (default: the step's `rips_dis`) - or, with knn (default: the step's `knn`), the clique complexes of their
        k-nearest-neighbour graphs, or with hull=True (default: the step's `hull`) their convex hulls - lifted on the device (SimplicialBatch.relift_): no host work per batch. A complex
        over the capacity leaves the structure of the captured batch as it was and shows in status(). With edges=list
        (int64 [2, n] of global vertex ids, copied into the step's static list buffer) the thresholded clique complexes of the
        listed graph; edge_th / tri_th (defaults: the step's) go with edges or knn."""
        if self.capacity is None:
            raise RuntimeError("GraphedTrainStep was built without a capacity: it replays ONE topology (load(features))")
        if (dis is not None) + (knn is not None) + bool(hull) + (edges is not None) > 1:
            raise ValueError("step(points=...): dis=... (Rips), knn=... (k-nearest-neighbour cliques), hull=True (convex "
                             "hulls) and edges=... (a listed graph) exclude each other")
        if dis is None and knn is None and not hull and edges is None:
            dis, knn, hull = self.rips_dis, self.knn, self.hull
            if self.edges and dis is None and knn is None and not hull:
                raise ValueError("step(points=...): pass edges=... (the step was built with edges: every call names its list)")
        if dis is None and knn is None and not hull and edges is None:
            raise ValueError("step(points=...): pass dis=... or knn=... or hull=True or edges=..., or set the step's rips_dis, knn or hull")
        if edges is not None or knn is not None:
            edge_th = self.edge_th if edge_th is None else edge_th
            tri_th = self.tri_th if tri_th is None else tri_th
        if edges is not None:
            edges = self._edge_list_buffer(edges)
        self.batch.relift_(points, dis, vertex_features, knn=knn, hull=bool(hull), edges=edges, edge_th=edge_th, tri_th=tri_th)

    def status(self) -> int:
        """The status words of the table rebuilds (ops.simplex_tables) and of the device lifts (ops.rips_lift / knn_lift / hull_lift: its bits
        1..4 are reported as bits 9..12, bit 5 of clique_lift - a refused edge list - as bit 13) so far; 0 = fine. Synchronises."""
        plan = self.batch._plan
        word, lift = plan.get("status"), plan.get("lift_status")
        return (0 if word is None else int(word.item())) | (0 if lift is None else int(lift.item()) << LIFT_STATUS_SHIFT)

    def step(self, features: Optional[Dict[str, torch.Tensor]] = None, batch=None, points: Optional[torch.Tensor] = None,
             vertex_features: Optional[Dict[str, torch.Tensor]] = None, dis: Optional[float] = None,
             knn: Optional[int] = None, hull: Optional[bool] = None, edges: Optional[torch.Tensor] = None,
             edge_th: Optional[float] = None, tri_th: Optional[float] = None) -> torch.Tensor:
        if batch is not None and points is not None:
            raise ValueError("step: pass batch=... (lifted on the host) or points=... (lifted on the device), not both")
        if batch is not None:
            self.load_batch(batch)
        if points is not None:
            self.load_points(points, dis, vertex_features, knn, hull, edges, edge_th, tri_th)
        if features:
            self.load(features)
        self.graph.replay()
        return self.loss
