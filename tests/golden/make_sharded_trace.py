"""Records tests/golden/sharded_call_trace.json: per rank, the stage calls, collectives and waits of every class of
csmpn_hip.sharded on the cases of tests/sharded_trace_helpers.py.

    python tests/golden/make_sharded_trace.py cpu     # the eager classes: gloo, the oracle as compute backend
    python tests/golden/make_sharded_trace.py gpu     # the graphed classes: needs cuda:0; keeps the "cpu" section
    python tests/golden/make_sharded_trace.py gpu OUT # ... written to OUT instead of the fixture

The fixture pins how the module talks to its backend and to torch.distributed, so it is recorded from the commit BEFORE
a change to csmpn_hip/sharded.py and replayed after it (tests/test_sharded_trace_cpu.py, tests/test_sharded_trace_gpu.py).
The one in the tree was recorded from commit 6a73e47, the parent of the change that folded the repeated stages of
sharded.py into shared functions. Every section is recorded twice and must come out equal.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import sharded_trace_helpers as T   # noqa: E402


def main(section, out=T.FIXTURE):
    cases, worker = {"cpu": (T.CPU_CASES, T.cpu_worker), "gpu": (T.GPU_CASES, T.gpu_worker)}[section]
    first, second = T.record(cases, worker), T.record(cases, worker)
    assert first == second, "the trace is not reproducible: " + ", ".join(k for k in first if first[k] != second[k])
    # (the graphed classes issue no collective in a single process: their world-1 traces are empty, and pinned as such)
    assert section == "gpu" or all(ev for ranks in first.values() for ev in ranks), "an empty trace"
    fixture = T.load_fixture() if os.path.exists(T.FIXTURE) else {}
    fixture[section] = first
    with open(out, "w") as f:
        json.dump(fixture, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    for k, ranks in first.items():
        print(k, [len(ev) for ev in ranks])


if __name__ == "__main__":
    main(*(sys.argv[1:] or ["cpu"]))
