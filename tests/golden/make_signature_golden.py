"""EGCL fixtures of the IMPORTED reference on signatures the device serves through the run-time-signature kernels
(csrc/cemlp_sig.hpp): the cases of make_golden.make_egcl (N = 12, E = 40, 4 channels, float32 and float64 runs) on

    cl13   (1,-1,-1,-1)      cl03  (-1,-1,-1)      cl11  (1,-1)      cl23  (1,1,-1,-1,-1)      cl31x  (-1,1,1,1)

Writes tests/golden/egcl_sig_<name>.npz with the metric stored in the file (these signatures have no tables_<name>.npz). A file that would be above 1 MiB (cl23) keeps its float64 runs and leaves the
float32 runs to egcl_sig_<name>_f32.npz; tests/signature_helpers.py reads both as one fixture.
Runs only where the reference is present (make_golden.py says how); only the data is committed. Usage:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_signature_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np

import make_golden

SIGNATURES = {
    "cl13": (1.0, -1.0, -1.0, -1.0),
    "cl03": (-1.0, -1.0, -1.0),
    "cl11": (1.0, -1.0),
    "cl23": (1.0, 1.0, -1.0, -1.0, -1.0),
    "cl31x": (-1.0, 1.0, 1.0, 1.0),
}

LIMIT = 1 << 20   # bytes: no committed file is larger

if __name__ == "__main__":
    for name, metric in SIGNATURES.items():
        make_golden.make_egcl(name, metric, C=4, kind="egcl_sig")
        path = os.path.join(HERE, f"egcl_sig_{name}.npz")
        with np.load(path) as g:
            out = {k: g[k] for k in g.files}
        out["metric"] = np.asarray(metric, dtype=np.float32)
        np.savez_compressed(path, **out)
        if os.path.getsize(path) > LIMIT:
            # a file above the repository's size limit (n = 5) keeps the float64 runs; the float32 runs go to a second file
            f32 = {k: v for k, v in out.items() if k.startswith("f32/")}
            np.savez_compressed(path, **{k: v for k, v in out.items() if k not in f32})
            np.savez_compressed(os.path.join(HERE, f"egcl_sig_{name}_f32.npz"), **f32)
            assert os.path.getsize(path) <= LIMIT, os.path.getsize(path)
        print("signature EGCL vectors written for", name, os.path.getsize(path), "bytes")
