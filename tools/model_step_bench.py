"""Whole-model training step, eager vs one HIP graph (csmpn_hip.graphed.GraphedTrainStep).

    python tools/model_step_bench.py [--batch 16] [--steps 30]
    python tools/model_step_bench.py --model md17 --varying 8 [--slack 0.0] [--pkg-root OTHER_TREE]

The convex-hulls task model at the reference's configuration (csmpn/configs/hulls.yaml: Cl(5,0), 28
hidden channels, 3 layers, batch size 16, 8 points per hull, Adam lr 1e-3) on synthetic hulls. Prints one
JSON line with the step times and the simplices / adjacencies of the batch.

--varying K: K different batches of the model (another complex in every graph), as a shuffled training loop sees them:
  eager_varying_ms_per_step    the eager step on a FRESH device batch per step - host-to-device copy, plan() and csr()
                               included: what such a loop costs without a capacity
  graphed_varying_ms_per_step  GraphedTrainStep(capacity=capacity_of(batches, slack)).step(batch=...) cycling through the K
                               batches: pad on the host, copy, rebuild the tables on the device, replay
  graphed_fixed_ms_per_step    the same captured step replayed on one topology (no refresh): the floor at this capacity
  fill_rows / fill_adjacencies real / padded, mean over the K batches
--device-lift (with --varying, Rips models): the same K point sets in the same run through step(points=...)
  graphed_device_lift_ms_per_step   csmpn_rips_lift + the in-place rebuild + the feature scatter + replay
  graphed_host_lifted_ms_per_step   step(batch=pre-lifted host batch) again, measured right behind it
  host_lift_ms_per_batch            rips_complex + collate + pad_batch of one batch on the host (what step(batch=...) leaves out)
--knn K (with --device-lift, md17): the batches are the clique complexes of the K-nearest-neighbour graphs
  (knn_clique_complex: the reference's aspirin configuration has K = 3) instead of Rips complexes, lifted on the device by
  step(points=..., knn=K) (csmpn_knn_lift); the same four figures, and the capacity's rows / adjacencies
--edge-th X / --tri-th Y (with --knn K): the batches are the THRESHOLDED clique complexes of the K-nearest-neighbour graphs
  (clique_complex(points, knn_edges(points, K), X, Y)), lifted on the device by step(points=..., knn=K, edge_th=X, tri_th=Y)
  (csmpn_clique_lift: the kNN masks, the filter, the table scatter); `inf` for both gives the very complexes of --knn K
  through the new entry - the kNN device-lift step plus the filter launch
--model hulls --varying K --device-lift: the K batches of convex hulls through step(points=..., hull=True) (csmpn_hull_lift:
  the complex, `input` and the volume target all from the device points); the host figure is qhull + lift + collate +
  pad_batch of one batch
--pkg-root: import the package from another tree (a build of another commit) with this same tool file; a tree without
  the capacity interface reports the eager figure only.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "clifford-group-equivariant-simplicial-message-passing-networks_amd"


def op_sites(eager, steps=2):
    """GPU time of an eager step by (innermost frame of this repo, autograd node, kernel): where the small launches
    come from. Chrome trace of torch.profiler: kernels -> launching runtime call by correlation id -> enclosing
    python_function / cpu_op events of the same thread by time."""
    import bisect
    import collections
    import tempfile
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
        for _ in range(steps):
            eager()
        torch.cuda.synchronize()
    path = os.path.join(tempfile.mkdtemp(), "trace.json")
    prof.export_chrome_trace(path)
    ev = json.load(open(path))["traceEvents"]
    launches, spans = {}, collections.defaultdict(list)
    for e in ev:
        if e.get("ph") != "X":
            continue
        cat = e.get("cat", "")
        if cat in ("cuda_runtime", "cuda_driver") and "correlation" in e.get("args", {}):
            launches[e["args"]["correlation"]] = e
        elif cat in ("python_function", "cpu_op", "user_annotation"):
            spans[(e["pid"], e["tid"])].append((e["ts"], e["ts"] + e["dur"], cat, e["name"]))
    for v in spans.values():
        v.sort()
    starts = {k: [s[0] for s in v] for k, v in spans.items()}
    table = collections.defaultdict(lambda: [0.0, 0])
    for e in ev:
        if e.get("ph") != "X" or e.get("cat") not in ("kernel", "gpu_memcpy", "gpu_memset"):
            continue
        la = launches.get(e.get("args", {}).get("correlation"))
        site, node = "?", ""
        if la is not None:
            key = (la["pid"], la["tid"])
            v, ts = spans.get(key, []), la["ts"]
            i = bisect.bisect_right(starts.get(key, []), ts)
            best_py, best_op = None, None
            for s0, s1, cat, name in reversed(v[max(0, i - 4000):i]):
                if s1 < ts:
                    continue
                if cat == "python_function" and best_py is None and ("csmpn" in name or "tools/" in name) and "<" not in name.split(":")[-1][:1]:
                    best_py = name
                if cat == "cpu_op" and (name.startswith("autograd::engine") or best_op is None):
                    best_op = name
            site = (best_py or "?").split("networks_amd/")[-1]
            node = (best_op or "").replace("autograd::engine::evaluate_function: ", "bwd:")
        k = (site[-70:], node[:40], e["name"][:60])
        table[k][0] += e["dur"]
        table[k][1] += 1
    tot = sum(v[0] for v in table.values())
    print(f"GPU time per step {tot / steps:.0f} us, {sum(v[1] for v in table.values()) / steps:.0f} launches")
    for k, (us, n) in sorted(table.items(), key=lambda kv: -kv[1][0])[:90]:
        print(f"{us / steps:8.1f} us {n / steps:5.1f}x  {k[0]:70s} {k[1]:40s} {k[2]}")


def thresholds(args):
    """None, or (edge_th, tri_th) where --edge-th or --tri-th is given (the other one: +infinity)."""
    if args.edge_th is None and args.tri_th is None:
        return None
    return (float("inf") if args.edge_th is None else args.edge_th, float("inf") if args.tri_th is None else args.tri_th)


def make_batch(args, rng, cx):
    """One collated CPU batch of the chosen model and the names of its changing tensors. The Rips models' batches carry the
    points they were lifted from and the threshold (lift_points float32 [B * V, n], lift_dis) for --device-lift."""
    points, dis = [], None
    if args.model == "hulls":
        points = [rng.standard_normal((args.points, 5)).astype(np.float32) for _ in range(args.batch)]
        batch = cx.collate([cx.hulls_example(p) for p in points])
        features = ["input", "target"]
    elif args.model == "motion":
        # motion-capture-shaped batch (motion_cssmpnn.py: Cl(3,0), 16 channels, 4 layers, aggr = mean): 31 joints per
        # skeleton, Vietoris-Rips complex of the joint positions, one frame of positions / velocities
        V, graphs, dis = 31, [], 1.6
        for _ in range(args.batch):
            base = (1.6 * rng.standard_normal((V, 3))).astype(np.float32)
            points.append(base)
            c = cx.rips_complex(base, dis=dis, max_dim=2)
            S = c.n_simplices
            pos, vel = torch.zeros(S, 3), torch.zeros(S, 3)
            pos[:V] = torch.from_numpy(base)
            vel[:V] = 0.1 * torch.from_numpy(rng.standard_normal((V, 3)).astype(np.float32))
            c.features.update(pos=pos, vel=vel)
            graphs.append(c)
        batch = cx.collate(graphs)
        batch.y = torch.cat([g.features["pos"][: g.n_vertices] + 0.1 * torch.randn(g.n_vertices, 3) for g in graphs], dim=0)
        batch._names.append("y")
        features = ["pos", "vel", "y"]
    elif args.model == "nba":
        # NBA-shaped batch (nba_cssmpnn.py:12-190: Cl(2,0), 40 channels, 4 layers, aggr = sum): 6 agents in the plane (5 players +
        # the ball), 10 frames, Vietoris-Rips complex of the first frame; the target: 40 future frames of the 5 players
        V, F, graphs, ys, dis = 6, 10, [], [], 1.6
        for _ in range(args.batch):
            base = rng.standard_normal((V, 2)).astype(np.float32)
            points.append(base)
            c = cx.rips_complex(base, dis=dis, max_dim=2)
            S = c.n_simplices
            pos, vel = torch.zeros(S, F, 2), torch.zeros(S, F, 2)
            pos[:V] = torch.from_numpy(base)[:, None, :] + 0.05 * torch.from_numpy(rng.standard_normal((V, F, 2)).astype(np.float32))
            vel[:V] = 0.1 * torch.from_numpy(rng.standard_normal((V, F, 2)).astype(np.float32))
            c.features.update(pos=pos, vel=vel)
            graphs.append(c)
            ys.append(torch.from_numpy(rng.standard_normal((V - 1, 4 * F, 2)).astype(np.float32)))
        batch = cx.collate(graphs)
        batch.y = torch.cat(ys, dim=0)
        batch._names.append("y")
        features = ["pos", "vel", "y"]
    else:
        # MD17-shaped batch (md17_cssmpnn.py; csmpn/configs/md17.yaml: Cl(3,0), 32 channels, 5 layers): 21 atoms
        # (aspirin), 10 frames, Vietoris-Rips complex of the first frame (--knn K: the clique complex of its K-nearest-neighbour
        # graph), random positions / velocities / charges
        V, F, graphs, dis = 21, 10, [], 1.8
        for _ in range(args.batch):
            base = (1.6 * rng.standard_normal((V, 3))).astype(np.float32)
            points.append(base)
            if args.knn and thresholds(args):
                c = cx.clique_complex(base, cx.knn_edges(base, args.knn), *thresholds(args), max_dim=2)
            else:
                c = cx.knn_clique_complex(base, args.knn, max_dim=2) if args.knn else cx.rips_complex(base, dis=dis, max_dim=2)
            S = c.n_simplices
            loc = torch.zeros(S, F, 3); vel = torch.zeros(S, F, 3); ch = torch.zeros(S, F, 1)
            loc[:V] = torch.from_numpy(base)[:, None, :] + 0.05 * torch.from_numpy(rng.standard_normal((V, F, 3)).astype(np.float32))
            vel[:V] = 0.1 * torch.from_numpy(rng.standard_normal((V, F, 3)).astype(np.float32))
            ch[:V] = torch.from_numpy(rng.integers(1, 9, size=(V, 1, 1)).astype(np.float32)).expand(V, F, 1)
            c.features.update(loc=loc, vel=vel, charges=ch)
            graphs.append(c)
        batch = cx.collate(graphs)
        batch.y = torch.cat([g.features["loc"][: g.n_vertices] + 0.1 * torch.randn(g.n_vertices, F, 3) for g in graphs], dim=0)
        batch._names.append("y")
        features = ["loc", "vel", "charges", "y"]
    if points:
        batch.lift_points, batch.lift_dis = np.concatenate(points, axis=0), dis
        if args.knn:
            batch.lift_knn, batch.lift_thresholds = args.knn, thresholds(args)
        if args.model == "hulls":
            batch.lift_hull = True
    return batch, features


LABELS = {"hulls": "hulls (Cl(5,0), 28 channels, 3 layers)", "md17": "md17 (Cl(3,0), 32 channels, 5 layers)",
          "motion": "motion (Cl(3,0), 16 channels, 4 layers)", "nba": "nba (Cl(2,0), 40 channels, 4 layers)"}


def timed(fn, steps, warm=5):
    """ms per call of fn(i), the device drained before and behind the window."""
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        fn(warm + i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def varying(args, rng, cx, M, GraphedTrainStep, dev):
    from csmpn_hip.graphed import flatten_parameters
    K = args.varying
    made = [make_batch(args, rng, cx) for _ in range(K)]
    batches, features = [m[0] for m in made], made[0][1]
    torch.manual_seed(0)
    model = {"hulls": M.HullsSimplicialMPNN, "md17": M.MD17SimplicialMPNN, "motion": M.MotionSimplicialMPNN,
             "nba": M.NBASimplicialMPNN}[args.model]().to(dev)
    opt_params = model.parameters() if args.no_flat_params else [flatten_parameters(model)]
    opt = torch.optim.Adam(opt_params, lr=1e-3, capturable=True, **({"foreach": True} if args.no_fused_adam else {"fused": True}))

    def eager(i):
        batch = batches[i % K].to(dev)          # a fresh device batch: its plan() and csr() are built inside the step
        opt.zero_grad(set_to_none=False)
        loss, _ = model(batch)
        loss.backward()
        opt.step()
        return loss

    out = {"model": LABELS[args.model], "graphs_per_batch": args.batch, "varying": K, "steps": args.steps,
           "simplices": [int(b.x_ind.shape[0]) for b in batches], "adjacencies": [int(b.edge_index.shape[1]) for b in batches],
           "eager_varying_ms_per_step": round(timed(eager, args.steps), 3)}
    if hasattr(cx, "capacity_of"):
        cap = cx.capacity_of(batches, args.slack)
        gs = GraphedTrainStep(model, opt, batches[0], features, capacity=cap)
        out["graphed_varying_ms_per_step"] = round(timed(lambda i: gs.step(batch=batches[i % K]), args.steps), 3)
        out["graphed_fixed_ms_per_step"] = round(timed(lambda i: gs.step(), args.steps), 3)
        out.update(capacity={"simplices": list(cap.simplices), "adjacencies": cap.edges}, slack=args.slack, status=gs.status(),
                   fill_rows=round(float(np.mean([b.x_ind.shape[0] for b in batches])) / cap.rows, 4),
                   fill_adjacencies=round(float(np.mean([b.edge_index.shape[1] for b in batches])) / cap.edges, 4),
                   loss=float(gs.loss.detach()))
        if args.device_lift:
            device_lift(args, out, cx, gs, batches, features, cap, dev)
    print(json.dumps(out))


def device_lift(args, out, cx, gs, batches, features, cap, dev):
    """--device-lift: the same K point sets through step(points=...) - the complexes lifted on the device in front of the
    replay - beside step(batch=pre-lifted host batch) of the same run, and what the host lift of such a batch costs."""
    if not hasattr(gs, "load_points") or not hasattr(batches[0], "lift_points"):
        raise SystemExit("--device-lift needs a tree with the device lift")
    K, dis, knn = len(batches), batches[0].lift_dis, getattr(batches[0], "lift_knn", None)
    hull = getattr(batches[0], "lift_hull", False)
    if hull and not hasattr(cx, "hull_batch_device"):
        raise SystemExit("--model hulls --device-lift needs a tree with the hull lift")
    ths = getattr(batches[0], "lift_thresholds", None)
    if ths and not hasattr(cx, "clique_complex"):
        raise SystemExit("--edge-th / --tri-th need a tree with the thresholded clique lift")
    how = dict(hull=True) if hull else dict(dis=dis) if knn is None else dict(knn=knn)
    host = (lambda g: cx.hull_complex(g, max_dim=2)) if hull else (lambda g: cx.rips_complex(g, dis=dis, max_dim=2)) if knn is None \
        else (lambda g: cx.knn_clique_complex(g, knn, max_dim=2))
    if ths:
        how.update(edge_th=ths[0], tri_th=ths[1])
        host = lambda g: cx.clique_complex(g, cx.knn_edges(g, knn), ths[0], ths[1], max_dim=2)
        out["thresholds"] = [str(t) for t in ths]
    names = [] if hull else [k for k in features if k != "y"]      # the hull lift fills `input` and `target` itself
    on_dev = []
    for b in batches:
        vertex = b.node_types == 0
        on_dev.append((torch.from_numpy(b.lift_points).to(dev), {k: getattr(b, k)[vertex].to(dev) for k in names},
                       None if hull else b.y.to(dev)))

    def lifted(i):
        pts, vf, y = on_dev[i % K]
        return gs.step(features=None if hull else {"y": y}, points=pts, vertex_features=vf, **how)

    out["graphed_device_lift_ms_per_step"] = round(timed(lifted, args.steps), 3)
    out["graphed_host_lifted_ms_per_step"] = round(timed(lambda i: gs.step(batch=batches[i % K]), args.steps), 3)
    out["status_after_device_lift"] = gs.status()
    t0 = time.perf_counter()
    for b in batches:
        p = b.lift_points.reshape(b.num_graphs, -1, b.lift_points.shape[-1])
        cx.pad_batch(cx.collate([host(g) for g in p]), cap)
    out["host_lift_ms_per_batch"] = round((time.perf_counter() - t0) * 1e3 / K, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--model", default="hulls", choices=["hulls", "md17", "motion", "nba"])
    ap.add_argument("--no-fused-adam", action="store_true", help="torch.optim.Adam(foreach) instead of fused=True")
    ap.add_argument("--no-fused-grads", action="store_true", help="hand parameter gradients to autograd (one add kernel per tensor)")
    ap.add_argument("--profile-ops", action="store_true", help="torch.profiler over 3 eager steps: the small GPU kernels by Python call site")
    ap.add_argument("--no-flat-params", action="store_true", help="optimizer over the module's ~1 000 parameter tensors instead of ONE flat buffer (csmpn_hip.graphed.flatten_parameters)")
    ap.add_argument("--op-sites", action="store_true", help="GPU kernels of one eager step by the package line that launched them")
    ap.add_argument("--varying", type=int, default=0, metavar="K", help="K batches of different topology: the eager loop on fresh device batches against ONE captured step with a capacity")
    ap.add_argument("--slack", type=float, default=0.0, help="--varying: capacity_of(batches, slack)")
    ap.add_argument("--device-lift", action="store_true", help="--varying: also step(points=...), the complexes lifted on the device, and the host time of the lift")
    ap.add_argument("--knn", type=int, default=0, metavar="K", help="--device-lift, md17: clique complexes of the K-nearest-neighbour graphs instead of Rips complexes")
    ap.add_argument("--edge-th", type=float, default=None, metavar="X", help="--knn K: drop the edges longer than X (thresholded clique lift; inf keeps all)")
    ap.add_argument("--tri-th", type=float, default=None, metavar="Y", help="--knn K: drop the triangles of area above Y (thresholded clique lift; inf keeps all)")
    ap.add_argument("--pkg-root", default=None, help="import the package from this tree instead of the tool's own")
    args = ap.parse_args()
    if args.knn and (args.model != "md17" or not args.device_lift or args.knn < 1):
        raise SystemExit("--knn K (K >= 1) goes with --model md17 --varying ... --device-lift")
    if (args.edge_th is not None or args.tri_th is not None) and not args.knn:
        raise SystemExit("--edge-th / --tri-th go with --knn K")
    if args.pkg_root:
        sys.path.insert(0, os.path.abspath(args.pkg_root))
    importlib.import_module(PKG)
    from csmpn.data import complexes as cx
    from csmpn.models import simplicial_mpnn as M
    from csmpn_hip.graphed import GraphedTrainStep
    from csmpn_hip import ops
    ops.set_fused_grad_accumulation(not args.no_fused_grads)

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    if args.varying:
        return varying(args, rng, cx, M, GraphedTrainStep, dev)
    batch, features = make_batch(args, rng, cx)
    batch = batch.to(dev)
    torch.manual_seed(0)
    model = {"hulls": M.HullsSimplicialMPNN, "md17": M.MD17SimplicialMPNN, "motion": M.MotionSimplicialMPNN,
             "nba": M.NBASimplicialMPNN}[args.model]().to(dev)
    # the reference trains with torch.optim.Adam (csmpn/configs/hulls.yaml); fused=True is the same update in one
    # multi-tensor kernel (the default foreach path with capturable=True issues ~300 per-tensor div kernels: 1.5 ms)
    from csmpn_hip.graphed import flatten_parameters
    opt_params = model.parameters() if args.no_flat_params else [flatten_parameters(model)]
    opt = torch.optim.Adam(opt_params, lr=1e-3, capturable=True,
                           **({"foreach": True} if args.no_fused_adam else {"fused": True}))

    def eager():
        opt.zero_grad(set_to_none=False)
        loss, _ = model(batch)
        loss.backward()
        opt.step()
        return loss

    for _ in range(5):
        eager()
    torch.cuda.synchronize()
    if args.op_sites:
        op_sites(eager)
        return
    if args.profile_ops:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
            for _ in range(3):
                eager()
            torch.cuda.synchronize()
        print(prof.key_averages(group_by_stack_n=6).table(sort_by="self_cuda_time_total", row_limit=45, max_name_column_width=50,
                                                            max_src_column_width=110))
        return
    t0 = time.perf_counter()
    for _ in range(args.steps):
        eager()
    torch.cuda.synchronize()
    eager_ms = (time.perf_counter() - t0) * 1e3 / args.steps

    gs = GraphedTrainStep(model, opt, batch, features)
    for _ in range(5):
        gs.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        gs.step()
    torch.cuda.synchronize()
    graph_ms = (time.perf_counter() - t0) * 1e3 / args.steps
    label = LABELS[args.model]
    print(json.dumps({"model": label, "graphs_per_batch": args.batch,
                      "simplices": int(batch.x_ind.shape[0]), "adjacencies": int(batch.edge_index.shape[1]),
                      "fused_grad_accumulation": not args.no_fused_grads, "fused_adam": not args.no_fused_adam, "flat_parameters": not args.no_flat_params, "eager_ms_per_step": round(eager_ms, 3), "graphed_ms_per_step": round(graph_ms, 3),
                      "loss": float(gs.loss.detach())}))


if __name__ == "__main__":
    main()
