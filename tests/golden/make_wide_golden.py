"""Generate the wide-channel EGCL fixture from the IMPORTED reference (modelled on make_golden.py).

Runs only where the reference is present; the resulting ``egcl_wide_cl30.npz`` is data and is committed. Usage:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_wide_golden.py

One EGCL of the reference (csmpn/models/cegnn_utils.py) at Cl(3,0), 96 channels (in = hidden = out = 96, 6 edge and 3 node
attribute channels, aggr="mean", residual) on the small complex of make_golden.py (duplicate edges, a self loop, a
high in-degree node, an isolated node). To stay within the size limit of a committed file (~480 k parameters):
  * the parameters are not stored: `param_value` draws each of them from a generator seeded by its name and rounds it
    to a float16 value (exact in float32 and float64); the GPU test restates the rule, `psum/<name>` pins it;
  * the float64 run (the truth) is stored rounded to float32 (7 digits, far below the 1e-5 bar);
  * of the [O, I, G] weight-matrix gradients only the output channels ROWS are kept: the first and the last channel
    tile and the rows around the 64-channel boundary (channel tiles 3 and 4);
  * the float32 run is stored as its error only: `yard/<tensor>` = max|f32 - f64| / max|f64| per tensor.
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np
import torch

import pyg_standin

pyg_standin.install()
REF = os.environ.get("CSMPN_REFERENCE", "/root/reference")
if not os.path.isdir(REF):
    print("reference not present: nothing to do")
    sys.exit(0)
sys.path.insert(0, REF)

from csmpn.algebra.cliffordalgebra import CliffordAlgebra  # noqa: E402
from csmpn.models import cegnn_utils as R  # noqa: E402

METRIC = (1.0, 1.0, 1.0)
C = 96
ROWS = np.r_[0:8, 60:72, 88:96]


def npy(t):
    return t.detach().cpu().numpy()


def param_value(name, shape):
    """Parameter `name` of the layer: a seeded draw around the reference's initial value, rounded to float16."""
    g = torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31))
    r = torch.randn(shape, generator=g, dtype=torch.float32)
    leaf = name.split(".")[-1]
    if leaf == "weight":
        v = r / (float(shape[1]) ** 0.5) if len(shape) == 3 else 0.5 * r   # [O, I, G] mixing / [O, P] path weights
    elif leaf == "a" and "normalization" not in name:
        v = 1.0 + 0.3 * r                                                 # MVSiLU / MVLayerNorm scales
    else:
        v = 0.3 * r                                                       # biases, MVSiLU shifts, normalization a
    return v.half().float()


def main():
    N, E, T = 12, 40, 3
    torch.set_default_dtype(torch.float32)
    gen = torch.Generator().manual_seed(37)
    ei = torch.randint(0, N - 1, (2, E), generator=gen)  # node N-1 is isolated
    ei[:, 5] = ei[:, 4]            # duplicate edge
    ei[:, 9] = ei[:, 4]            # triplicate
    ei[1, 12] = ei[0, 12]          # self loop
    ei[1, 20:28] = 3               # high in-degree node
    types = torch.randint(0, T, (N,), generator=gen)
    D = 1 << len(METRIC)
    h0 = torch.randn(N, C, D, generator=gen, dtype=torch.float32)
    node_attr = torch.zeros(N, T, D)
    node_attr[torch.arange(N), types, 0] = 1.0
    edge_attr = torch.cat([node_attr[ei[0]], node_attr[ei[1]]], dim=1)
    gout = torch.randn(N, C, D, generator=torch.Generator().manual_seed(47), dtype=torch.float32)

    layer32 = R.EGCL(CliffordAlgebra(METRIC), C, C, C, edge_attr_features=2 * T, node_attr_features=T, aggr="mean")
    params = {k: param_value(k, tuple(v.shape)) for k, v in layer32.named_parameters()}

    def run(dtype):
        torch.set_default_dtype(dtype)
        layer = R.EGCL(CliffordAlgebra(METRIC), C, C, C, edge_attr_features=2 * T, node_attr_features=T, aggr="mean")
        sd = layer.state_dict()
        for k, v in params.items():
            sd[k] = v.to(dtype)
        layer.load_state_dict(sd, strict=True)
        h = h0.to(dtype).clone().requires_grad_(True)
        y = layer(h, ei, edge_attr.to(dtype), node_attr.to(dtype))
        (y * gout.to(dtype)).sum().backward()
        res = {"y": npy(y).astype(np.float64), "gh": npy(h.grad).astype(np.float64)}
        for k, v in layer.named_parameters():
            res["g/" + k] = npy(v.grad).astype(np.float64)
        torch.set_default_dtype(torch.float32)
        return res

    truth, r32 = run(torch.float64), run(torch.float32)
    out = {"h": npy(h0), "edge_index": npy(ei), "edge_attr": npy(edge_attr), "node_attr": npy(node_attr), "gout": npy(gout)}
    for k, v in params.items():
        out["psum/" + k] = np.float64(npy(v).astype(np.float64).sum())
    out["rows"] = ROWS.astype(np.int64)
    for k, v in truth.items():
        w = r32[k]
        if k.startswith("g/") and v.ndim == 3 and v.shape[0] == C:   # weight matrix [O, I, G]
            v, w = v[ROWS], w[ROWS]
        out["f64/" + k] = v.astype(np.float32)
        out["yard/" + k] = np.float64(np.abs(w - v).max() / max(np.abs(v).max(), 1e-30))
    path = os.path.join(HERE, "egcl_wide_cl30.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
