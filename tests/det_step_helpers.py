"""Helpers of tests/test_deterministic_step_gpu.py: the task models and batches of tests/golden/model_<kind>.npz (the
build / load_batch of tests/test_model_harness.py, restated here so that file stays as it is) and the scoped switches
of the deterministic request."""
import contextlib
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KINDS = ["hulls", "md17", "motion", "nba"]


def load_batch(pkg, g, prefix="b/", device=None):
    from csmpn.data.complexes import SimplicialBatch
    t = {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}
    b = SimplicialBatch(**t)
    return b.to(device) if device is not None else b


def build(pkg, kind, g, device=None):
    from csmpn.models import simplicial_mpnn as M
    model = {"hulls": M.HullsSimplicialMPNN, "md17": M.MD17SimplicialMPNN, "motion": M.MotionSimplicialMPNN,
             "nba": M.NBASimplicialMPNN}[kind]()
    sd = model.state_dict()
    want = {k[2:] for k in g.files if k.startswith("p/")}
    have = {k for k in sd if "algebra." not in k}
    assert want == have, (sorted(want - have)[:5], sorted(have - want)[:5])
    for k in want:
        sd[k] = torch.from_numpy(g["p/" + k])
    model.load_state_dict(sd, strict=True)
    return model.to(device) if device is not None else model


def fixture(kind):
    return np.load(os.path.join(GOLD, f"model_{kind}.npz"))


@contextlib.contextmanager
def deterministic(torch_flag=True, request=True):
    """torch.use_deterministic_algorithms(torch_flag) and ops.set_deterministic(request) for the body; the state found
    on entry is put back whatever happens."""
    from csmpn_hip import ops
    was_torch = torch.are_deterministic_algorithms_enabled()
    was_warn = torch.is_deterministic_algorithms_warn_only_enabled()
    was_req = ops._DETERMINISTIC
    try:
        torch.use_deterministic_algorithms(torch_flag)
        ops.set_deterministic(request)
        yield ops
    finally:
        ops.set_deterministic(was_req)
        torch.use_deterministic_algorithms(was_torch, warn_only=was_warn)
