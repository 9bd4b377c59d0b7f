#!/usr/bin/env python3
"""Static instruction mix of the (row, channel)-per-lane kernels, per kernel symbol.

    hipcc $(CL_FLAGS) -S --cuda-device-only -o k_cl_n3.s k_cl_n3.hip
    python3 tools/cl_instruction_mix.py k_cl_n3.s [--raw]

Prints one column per cemlp_cl_{fwd,bwd}_kernel symbol with the instruction classes of DESIGN.md section 4.1. A class
is a mnemonic prefix, nothing else; `--raw` adds the full mnemonic histogram of every symbol (profiles/r09_S1_instruction_mix.txt).
A backward symbol holds two instantiations of the tile body (one tile per wave, and the tile loop).
This is a counter for the budget table, not a checker.
"""
import collections
import re
import subprocess
import sys

DPP_MIX = ("v_fmac_f32_dpp",)
FP32 = ("v_fma", "v_mul_f32", "v_add_f32", "v_sub_f32", "v_subrev_f32", "v_pk_add_f32", "v_pk_mul_f32", "v_pk_fma_f32")
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")
ROWS = ["all instructions", "v_fmac_f32_dpp", "other fp32 arithmetic", "transcendental", "MFMA", "other DPP (row sums)", "vector, not arithmetic",
        "  v_mov", "  v_cndmask", "  other", "SALU", "s_nop", "s_waitcnt", "LDS", "global / buffer", "VGPRs", "occupancy", "scratch B"]


def classify(m):
    if m.startswith(DPP_MIX): return "v_fmac_f32_dpp"
    if m.startswith("v_mfma"): return "MFMA"
    if m.endswith("_dpp"): return "other DPP (row sums)"
    if m.startswith(TRANS): return "transcendental"
    if m.startswith(FP32): return "other fp32 arithmetic"
    if m.startswith("v_mov"): return "  v_mov"
    if m.startswith("v_cndmask"): return "  v_cndmask"
    if m.startswith("v_"): return "  other"
    if m.startswith("s_nop"): return "s_nop"
    if m.startswith("s_waitcnt"): return "s_waitcnt"
    if m.startswith("s_"): return "SALU"
    if m.startswith("ds_"): return "LDS"
    if m.startswith(("global_", "buffer_", "flat_", "scratch_")): return "global / buffer"
    return "other"


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    m = re.search(r"cemlp_cl_(fwd|bwd)_kernel<[^,]*<[^>]*>, (.*)>\(", name)
    if not m: return name
    args = m.group(2).replace(" ", "")
    return ("fwd<" if m.group(1) == "fwd" else "bwd<") + args + ">"


def main():
    path = sys.argv[1]
    raw = "--raw" in sys.argv[2:]
    hist, meta, cur = collections.OrderedDict(), {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w*cemlp_cl_(?:fwd|bwd)_kernel\w*):", s)
        if m:
            cur = m.group(1)
            hist[cur] = collections.Counter()
            meta[cur] = {}
            continue
        if cur is None: continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"): continue
        hist[cur][s.split()[0]] += 1
    # resource usage: "; NumVgprs: N", "; Occupancy: N", "; ScratchSize: N" inside the block that follows each kernel
    cur = None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w*cemlp_cl_(?:fwd|bwd)_kernel\w*):", s)
        if m: cur = m.group(1)
        if cur is None: continue
        for key, row in (("NumVgprs", "VGPRs"), ("Occupancy", "occupancy"), ("ScratchSize", "scratch B")):
            mm = re.match(r"^; %s: (\d+)" % key, s)
            if mm and row not in meta[cur]: meta[cur][row] = int(mm.group(1))
    names = demangle(list(hist))
    cols = []
    for sym, h in hist.items():
        c = collections.Counter()
        for mn, n in h.items():
            c[classify(mn)] += n
            c["all instructions"] += n
        c["vector, not arithmetic"] = c["  v_mov"] + c["  v_cndmask"] + c["  other"]
        c.update(meta[sym])
        cols.append((short(names[sym]), c, h))
    width = max(len(r) for r in ROWS) + 2
    print(" " * width + "".join("%24s" % n for n, _, _ in cols))
    for r in ROWS:
        print(r.ljust(width) + "".join("%24d" % c[r] for _, c, _ in cols))
    if raw:
        for n, _, h in cols:
            print("\n== %s" % n)
            for mn, k in sorted(h.items(), key=lambda kv: (-kv[1], kv[0])):
                print("%6d  %s" % (k, mn))


if __name__ == "__main__":
    main()
