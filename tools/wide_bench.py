"""EGCL forward + backward time on the wide row-tile kernel (65..256 channels, csrc/cemlp_wide.hpp) against the 64-channel
general kernel, on a synthetic complex of 10 k nodes / 100 k edges (6 edge / 3 node attribute channels, aggr="mean").

    python tools/wide_bench.py [--steps 20] [--warmup 5] [--shapes cl30:64,cl30:96,cl30:128,cl50:96]

One JSON line per shape: median / min milliseconds of one forward + backward of the layer (CUDA events), and the
kernel each stage ran (csmpn_last_kernel of the forward on this thread)."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
METRICS = {"cl20": (1.0, 1.0), "cl30": (1.0, 1.0, 1.0), "cl40": (1.0,) * 4, "cl50": (1.0,) * 5, "cl41": (1.0, 1.0, 1.0, 1.0, -1.0)}


def run(pkg, name, C, N, E, steps, warmup):
    from oracle import ref_path as O
    from csmpn_hip import native
    metric = METRICS[name]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    layer = pkg.EGCL(pkg.CliffordAlgebra(metric), C, C, C, edge_attr_features=6, node_attr_features=3, aggr="mean").to(dev)
    h, ei, ea, na = (t.to(dev) for t in O.synthetic_complex(O.Algebra(list(metric)), N, E, C, seed=1))
    h.requires_grad_(True)
    gout = torch.randn(N, C, 1 << len(metric), device=dev)
    times = []
    kernel = ""
    for it in range(warmup + steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        y = layer(h, ei, ea, na)
        kernel = native.lib().csmpn_last_kernel().decode()
        (y * gout).sum().backward()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            times.append(a.elapsed_time(b))
        layer.zero_grad(set_to_none=True)
        h.grad = None
    times.sort()
    return {"shape": f"{name}:{C}", "nodes": N, "edges": E, "ms_median": times[len(times) // 2], "ms_min": times[0],
            "node_forward_kernel": kernel}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--edges", type=int, default=100_000)
    ap.add_argument("--shapes", default="cl30:64,cl30:96,cl30:128,cl50:96")
    args = ap.parse_args()
    pkg = importlib.import_module("clifford-group-equivariant-simplicial-message-passing-networks_amd")
    for s in args.shapes.split(","):
        name, C = s.split(":")
        print(json.dumps(run(pkg, name, int(C), args.nodes, args.edges, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
