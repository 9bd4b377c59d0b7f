"""Snapshot of the buffer-sizing contract of the library (host-only queries, no GPU): csmpn_cemlp_saved_floats with and
without CSMPN_FLAG_SAVE_STATE, csmpn_cemlp_saved_floats_per_row and csmpn_cemlp_workspace_bytes over a sweep of shapes,
under the default environment and under each switch that enters the sizing. The switches are read once per process, so
every environment is measured in a child process of its own.

    python tests/golden/make_sizing_golden.py            # rewrites tests/golden/sizing_contract.npz

tests/test_sizing_contract.py compares the built library with the stored figures, entry by entry. The fixture in the
tree was recorded from the library of commit f7329ee (the parent of the change that split csrc/capi.hip), its "no_cm" table
from the library of commit 5645b40 (the parent of the change that gave every kernel family one statement of its regions).
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "sizing_contract.npz")

NS = (2, 3, 4, 5)
CHANNELS = (3, 5, 8, 12, 16, 24, 28, 32, 40, 64, 65, 96, 128, 256)
ROWS = (1, 15, 16, 17, 1001, 4095, 4096, 8191, 8192, 100000)
PLAIN_EXTRA_INPUTS = (40, 60, 90)      # standalone CEMLPs of the task models, at 16 and 32 channels
ENVS = {
    "default": {},
    "no_cm_bwd": {"CSMPN_NO_CM_BWD": "1"},
    "no_cm": {"CSMPN_NO_CM": "1"},
    "no_pq": {"CSMPN_NO_PQ": "1"},
    "phased_min_rows_1000": {"CSMPN_PHASED_MIN_ROWS": "1000"},
}
SWITCHES = sorted({k for e in ENVS.values() for k in e})


def configs():
    """(n, first-block input channels, channels, blocks) of every swept shape, in fixture order."""
    out = []
    for n in NS:
        for c in CHANNELS:
            inputs = [c + 6, 2 * c + 3, c]            # EGCL edge, EGCL node, plain
            if c in (16, 32):
                inputs += list(PLAIN_EXTRA_INPUTS)
            for i0 in inputs:
                for nblk in (1, 2, 3, 4):
                    out.append((n, i0, c, nblk))
    return out


def measure():
    """uint64 [configs, 2 + 2 * len(ROWS)]: per-row floats, workspace bytes, then saved floats (flags 0, SAVE_STATE) per row count."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import importlib
    importlib.import_module("clifford-group-equivariant-simplicial-message-passing-networks_amd")
    from csmpn_hip import native
    lib = native.lib()
    cfg = configs()
    table = np.zeros((len(cfg), 2 + 2 * len(ROWS)), dtype=np.uint64)
    for r, (n, i0, c, nblk) in enumerate(cfg):
        blocks = (native.BlockParams * nblk)()
        for k in range(nblk):
            blocks[k].in_features = i0 if k == 0 else c
            blocks[k].out_features = c
            blocks[k].lin_subspaces = 1
        table[r, 0] = lib.csmpn_cemlp_saved_floats_per_row(n, blocks, nblk)
        table[r, 1] = lib.csmpn_cemlp_workspace_bytes(n, blocks, nblk)
        for j, rows in enumerate(ROWS):
            table[r, 2 + 2 * j] = lib.csmpn_cemlp_saved_floats(n, blocks, nblk, rows, 0)
            table[r, 3 + 2 * j] = lib.csmpn_cemlp_saved_floats(n, blocks, nblk, rows, native.FLAG_SAVE_STATE)
    return table


def measure_in_child(env_name, out_path):
    """The sweep in a fresh interpreter under ENVS[env_name]; the table lands in out_path (.npy)."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[env_name])
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out_path], env=env, check=True, cwd=ROOT,
                   timeout=600)
    return np.load(out_path)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        np.save(sys.argv[2], measure())
    else:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            tables = {name: measure_in_child(name, os.path.join(tmp, name + ".npy")) for name in ENVS}
        np.savez_compressed(FIXTURE, configs=np.asarray(configs(), dtype=np.int32), rows=np.asarray(ROWS, dtype=np.int64),
                            **tables)
        print(f"{FIXTURE}: {os.path.getsize(FIXTURE)} bytes, {len(configs())} shapes x {len(ENVS)} environments")
