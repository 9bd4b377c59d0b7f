#!/usr/bin/env python3
"""Rate of one float64 EGCL layer (forward + backward) on the device against the float64 C++ twin on the host CPUs, at S1's
size (Cl(3,0), 8 channels, 10 k nodes, 100 k edges) and at H28's (Cl(5,0), 28 channels, same graph size): a warm-up, then
the median of the timed repeats; one process on the card. The twin is what the suite pays today for the same truth.

    python tools/f64_rate.py [--repeats 5] [--threads 16] [--sizes S1,H28] [--no-twin]
Prints one JSON line per size.
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

SIZES = {"S1": ((1.0, 1.0, 1.0), 8, 10_000, 100_000), "H28": ((1.0,) * 5, 28, 10_000, 100_000)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--sizes", default="S1,H28")
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    pkg = importlib.import_module("clifford-group-equivariant-simplicial-message-passing-networks_amd")
    from oracle import cpu_twin, ref_path as O
    dev = torch.device("cuda:0")
    for name in a.sizes.split(","):
        metric, C, N, E = SIZES[name]
        o = O.Algebra(list(metric), torch.float64)
        h, ei, ea, na = O.synthetic_complex(o, N, E, C, seed=0, dtype=torch.float64)
        torch.manual_seed(0)
        layer = pkg.EGCL(pkg.CliffordAlgebra(metric), C, C, C, edge_attr_features=6, node_attr_features=3, aggr="mean").double()
        params = {k: v.detach().numpy() for k, v in layer.named_parameters()}
        layer = layer.to(dev)
        hd, eid, ead, nad = h.to(dev).requires_grad_(True), ei.to(dev), ea.to(dev), na.to(dev)
        gout = torch.ones(N, C, o.D, dtype=torch.float64, device=dev)

        def step():
            layer.zero_grad(set_to_none=True)
            hd.grad = None
            layer(hd, eid, ead, nad).backward(gout)

        step()
        step()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        res = {"size": name, "device_ms": 1e3 * statistics.median(times), "repeats": a.repeats}
        if not a.no_twin:
            run = lambda: cpu_twin.egcl_layer(metric, params, h.numpy(), ei.numpy(), ea.numpy(), na.numpy(), aggr="mean",
                                              gout=gout.cpu().numpy(), threads=a.threads, real64=True)
            run()
            tt = []
            for _ in range(max(3, a.repeats // 2)):
                t0 = time.perf_counter()
                run()
                tt.append(time.perf_counter() - t0)
            res.update(twin_ms=1e3 * statistics.median(tt), twin_threads=a.threads)
            res["speedup"] = res["twin_ms"] / res["device_ms"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
