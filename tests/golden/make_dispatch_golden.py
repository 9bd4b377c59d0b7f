"""Snapshot of the dispatch and launch geometry of the library (needs the GPU): which kernel serves every stage of a set of
EGCL layers, standalone CEMLPs and fused embeddings (csmpn_last_kernel) and the launch line CSMPN_DEBUG=1 prints for it
(family, mode, grid, threads, LDS bytes, variant, RT / MT / H, share / phased, mirror), at two sizes - N = 37 / E = 101 and
N = 600 / E = 9000, the second past both phased-backward thresholds - under the default environment and under the switches
that move a shape to another family. The switches are read once per process: one child process per environment.

    python tests/golden/make_dispatch_golden.py          # rewrites tests/golden/dispatch_snapshot.json

tests/test_dispatch_snapshot_gpu.py compares the built library with the stored strings, verbatim. The fixture in the tree
was recorded from the library of commit f7329ee (the parent of the change that split csrc/capi.hip). A shape the library
refuses is recorded as its error (code and csmpn_last_error text).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "dispatch_snapshot.json")

CL20, CL30, CL40, CL31 = (1.0, 1.0), (1.0, 1.0, 1.0), (1.0,) * 4, (1.0, 1.0, 1.0, -1.0)
CL50, CL41 = (1.0,) * 5, (1.0, 1.0, 1.0, 1.0, -1.0)
SIZES = {"small": (37, 101), "large": (600, 9000)}

# name -> (kind, metric, ...): "egcl" (channels, deterministic), "cemlp" (block widths), "embed" (vertices per row, channels
# per vertex, vertex orders, blocks, channels)
CASES = {}
for _tag, _metric, _widths in (("cl30", CL30, (5, 8, 12, 16, 32, 96)), ("cl20", CL20, (40,)), ("cl40", CL40, (8,)),
                               ("cl31", CL31, (8,)), ("cl50", CL50, (8, 16, 28, 20, 96)), ("cl41", CL41, (8, 32))):
    for _c in _widths:
        CASES[f"egcl-{_tag}-{_c}"] = ("egcl", _metric, _c, False)
for _tag, _metric, _c in (("cl30", CL30, 8), ("cl30", CL30, 12), ("cl20", CL20, 40)):
    CASES[f"egcl-{_tag}-{_c}-det"] = ("egcl", _metric, _c, True)
CASES["cemlp-cl41-8x3"] = ("cemlp", CL41, (8, 8, 8, 8))             # three blocks: the parity-split kernels
CASES["cemlp-cl30-60-32"] = ("cemlp", CL30, (60, 32))
CASES["cemlp-cl30-90-32-32"] = ("cemlp", CL30, (90, 32, 32))
CASES["cemlp-cl30-40-16-16"] = ("cemlp", CL30, (40, 16, 16))
CASES["embed-hulls-edges"] = ("embed", CL50, 2, 1, 2, 1, 28)        # the convex-hulls model: 1-simplices, one block
CASES["embed-hulls-triangles"] = ("embed", CL50, 3, 1, 6, 2, 28)    # 2-simplices, two blocks

_D32 = [k for k, c in CASES.items() if len(c[1]) == 5 and k != "cemlp-cl41-8x3" and not k.endswith("-96")]
_W32 = ["egcl-cl30-32", "cemlp-cl30-60-32", "cemlp-cl30-90-32-32"]
# environment of the child -> cases it runs
VARIANTS = {
    "default": ({}, list(CASES)),
    "save_state_0": ({"CSMPN_SAVE_STATE": "0"}, ["egcl-cl50-28", "egcl-cl30-32", "egcl-cl41-32"]),
    "no_pq": ({"CSMPN_NO_PQ": "1"}, _W32),
    "no_cm_bwd": ({"CSMPN_NO_CM_BWD": "1"}, ["egcl-cl30-16"] + _W32),
    "no_cl": ({"CSMPN_NO_CL": "1"}, ["egcl-cl30-8", "egcl-cl30-8-det"]),
    "no_pl_plw_pg": ({"CSMPN_NO_PL": "1", "CSMPN_NO_PLW": "1", "CSMPN_NO_PG": "1"}, _D32),
    "force_h_2": ({"CSMPN_FORCE_H": "2"}, ["egcl-cl30-5", "egcl-cl30-8"]),
}
_CLEARED = sorted({k for env, _ in VARIANTS.values() for k in env} | {"CSMPN_DEBUG", "CSMPN_DETERMINISTIC", "CSMPN_QUIET"})


def _child(names):
    """Runs the cases on this thread (csmpn_last_kernel is per thread); a marker line on stderr in front of each."""
    import importlib
    sys.path.insert(0, ROOT)
    import torch
    pkg = importlib.import_module("clifford-group-equivariant-simplicial-message-passing-networks_amd")
    from csmpn_hip import native, ops
    from oracle import ref_path as O
    dev = torch.device("cuda:0")
    lib = native.lib()
    last = lambda: lib.csmpn_last_kernel().decode()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def egcl(metric, C, det, N, E, names_out):
        torch.manual_seed(3)
        layer = pkg.EGCL(pkg.CliffordAlgebra(tuple(metric)), C, C, C, edge_attr_features=6, node_attr_features=3).to(dev)
        h, ei, ea, na = (t.to(dev) for t in O.synthetic_complex(O.Algebra(list(metric)), N, E, C, seed=4))
        be, spec = ops.HipBackend, layer.spec()
        csr = ops.get_csr(ei, N)
        pe, pn = layer.edge_model.flat_params(), layer.node_model.flat_params()
        ops.set_deterministic(True if det else None)
        agg, st_e = be.edge_forward(spec, csr, h, ea, pe)
        names_out["edge_fwd"] = last()
        out, st_n = be.node_forward(spec, csr.deg, h, agg, na, pn)
        names_out["node_fwd"] = last()
        gh, g_agg, _, _ = be.node_backward(spec, csr.deg, h, agg, na, pn, torch.ones_like(out), False, st_n)
        names_out["node_bwd"] = last()
        be.edge_backward(spec, csr, h, ea, pe, g_agg, gh, False, st_e)
        names_out["edge_bwd"] = last()

    def module(metric, widths):
        torch.manual_seed(3)
        m = pkg.CEMLP(pkg.CliffordAlgebra(tuple(metric)), widths[0], widths[1], widths[-1], n_layers=len(widths) - 1).to(dev)
        b, params = m.binding(), m.flat_params()
        b.bind(params)
        return b, params

    def cemlp(metric, widths, N, E, names_out):
        # the calls of ops._CemlpFn, made here so that the backward runs on this thread too
        b, params = module(metric, widths)
        x = torch.randn(E, widths[0], b.D, generator=torch.Generator().manual_seed(5)).to(dev)
        y = torch.empty(E, widths[-1], b.D, device=dev)
        ws = b.workspace(dev)
        want_state = ops._SAVE_STATE and b.n == 3 and b.out_features == 32
        saved = b.new_saved(E, dev, want_state)
        flags = native.FLAG_SAVE_STATE if (want_state and saved is not None) else 0
        native.check(lib.csmpn_cemlp_forward(b.metric_arr, b.n, b.params, b.nblk, x.data_ptr(), E, y.data_ptr(), ops._ptr(saved),
                                             ws.data_ptr(), ws.numel(), flags, stream()))
        names_out["fwd"] = last()
        _flat, _views = b.new_grads(params, dev)
        gx = torch.empty_like(x)
        native.check(lib.csmpn_cemlp_backward(b.metric_arr, b.n, b.params, b.grads, b.nblk, x.data_ptr(), torch.ones_like(y).data_ptr(),
                                              E, gx.data_ptr(), ops._ptr(saved), ws.data_ptr(), ws.numel(),
                                              native.FLAG_WEIGHTS_PACKED | flags, stream()))
        names_out["bwd"] = last()

    def embed(metric, nv, kpv, orders, nblk, C, N, E, names_out):
        # the calls of ops._EmbedCemlpFn
        b, params = module(metric, (nv * kpv,) + (C,) * nblk)
        rows = E // orders * orders
        feat = torch.randn(N, kpv, b.D, generator=torch.Generator().manual_seed(5)).to(dev)
        verts = torch.randint(0, N, (rows, nv), generator=torch.Generator().manual_seed(6), dtype=torch.int32).to(dev)
        out = torch.empty(rows // orders, C, b.D, device=dev)
        ws = b.workspace(dev)
        state = ops._SAVE_STATE and nblk > 1
        saved = b.new_saved(rows, dev, state)
        flags = native.FLAG_SAVE_STATE if (state and saved is not None) else 0
        native.check(lib.csmpn_embed_cemlp_forward(b.metric_arr, b.n, b.params, b.nblk, feat.data_ptr(), N, kpv, verts.data_ptr(), nv,
                                                   orders, rows, out.data_ptr(), ops._ptr(saved), ws.data_ptr(), ws.numel(), flags,
                                                   stream()))
        names_out["fwd"] = last()
        _flat, _views = b.new_grads(params, dev)
        native.check(lib.csmpn_embed_cemlp_backward(b.metric_arr, b.n, b.params, b.grads, b.nblk, feat.data_ptr(), N, kpv,
                                                    verts.data_ptr(), nv, orders, rows, torch.ones_like(out).data_ptr(), ops._ptr(saved),
                                                    ws.data_ptr(), ws.numel(), flags | native.FLAG_NO_VALIDATE, stream()))
        names_out["bwd"] = last()

    result = {}
    for name in names:
        kind, metric, *rest = CASES[name]
        for size, (N, E) in SIZES.items():
            key = f"{name}@{size}"
            os.write(2, f"@@case {key}\n".encode())
            stages = {}
            try:
                {"egcl": egcl, "cemlp": cemlp, "embed": embed}[kind](metric, *rest, N, E, stages)
                torch.cuda.synchronize()
            except native.CsmpnError as err:     # a shape the library refuses: the refusal is the record
                stages["error"] = str(err)
            result[key] = stages
    print("@@kernels " + json.dumps(result))


def run_variant(variant):
    """{case@size: {"kernels": {stage: csmpn_last_kernel | "error": text}, "log": [launch lines]}} of one child process."""
    extra, names = VARIANTS[variant]
    env = {k: v for k, v in os.environ.items() if k not in _CLEARED}
    env.update(extra, CSMPN_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + names, env=env, capture_output=True, text=True,
                       cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    kernels = json.loads([l for l in r.stdout.splitlines() if l.startswith("@@kernels ")][-1][len("@@kernels "):])
    out, key = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("@@case "):
            key = line[len("@@case "):]
            out[key] = {"kernels": kernels[key], "log": []}
        elif line.startswith("[csmpn] ") and not line.startswith("[csmpn] note:"):
            out[key]["log"].append(line)
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        _child(sys.argv[2:])
    else:
        snap = {v: run_variant(v) for v in VARIANTS}
        with open(FIXTURE, "w") as f:
            json.dump(snap, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes")
