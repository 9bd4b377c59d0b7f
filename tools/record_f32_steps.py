#!/usr/bin/env python3
"""Record the float32 loss and gradients of the four task-model steps under CSMPN_DETERMINISTIC=1 (needs the GPU):
tests/golden/f32_steps_parent.npz, which tests/test_f64_gpu.py compares this build with, bit for bit. The recording in the
repository was made with --tree pointing at a built checkout of the commit in front of the float64 kernel family; the
helper that runs the steps is the test's own (tests/f64_helpers.py: f32_step_record).

    python tools/record_f32_steps.py [--tree CHECKOUT] [--out FILE]
"""
import argparse
import os
import sys

os.environ["CSMPN_DETERMINISTIC"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np  # noqa: E402

import f64_helpers as H  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--tree", default=H.ROOT, help="built checkout whose package runs the steps (default: this one)")
    ap.add_argument("--out", default=H.F32_RECORDING)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    mod = H.pkg()
    assert os.path.abspath(mod.__file__).startswith(os.path.abspath(a.tree)), mod.__file__
    rec = H.f32_step_record()
    np.savez_compressed(a.out, **rec)
    print("wrote", a.out, {k: (v.tolist() if v.size == 1 else v.shape) for k, v in rec.items() if k.endswith("loss")})


if __name__ == "__main__":
    main()
