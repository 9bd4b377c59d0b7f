"""Host-side restatements shared by the tests of the wide row-tile kernel (cemlp_wide.hpp): the parameter rule of the
96-channel reference fixture, the size of one deterministic gradient copy and the number of copies (= workgroups of a
deterministic backward launch), the footprint of one row tile. No GPU, no library call: plain arithmetic, so that a test
can say what the library should have chosen without asking the library."""
import torch

LDS_BYTES = 160 * 1024      # launch.hpp: kMaxLdsBytes
GRID_CAP = 256              # plan.hip: kGlobalTileGrid (plan.grid_cap of every wide plan)
ROWS_PER_TILE = 16


def wide_fixture_param(name, shape):
    """tests/golden/make_wide_golden.py::param_value (restated; `psum/<name>` in the fixture pins it)."""
    g = torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(name)) % (2 ** 31))
    r = torch.randn(shape, generator=g, dtype=torch.float32)
    leaf = name.split(".")[-1]
    if leaf == "weight":
        v = r / (float(shape[1]) ** 0.5) if len(shape) == 3 else 0.5 * r
    elif leaf == "a" and "normalization" not in name:
        v = 1.0 + 0.3 * r
    else:
        v = 0.3 * r
    return v.half().float()


def slice_bytes(n, widths):
    """Bytes of one copy of the gradient tensors of a CEMLP with blocks `widths` = [(in, out), ...] over an algebra with
    n <= 3 generators (mirror_floats_of in csrc/plan.hip): W1 [O, I, G], WR and WL [O, O, G], b1, bL, ln_a [O], the MVSiLU
    a / b and the normalization a [O, G], the path weights [O, P]; every block rounded up to 4 floats."""
    G, P = n + 1, {2: 10, 3: 20}[n]
    tot = 0
    for I, O in widths:
        tot += (G * O * I + 2 * G * O * O + 3 * O + 3 * O * G + O * P + 3) // 4 * 4
    return 4 * tot


def wide_det_groups(n, widths):
    """Workgroups of a deterministic wide backward launch: as many gradient copies as fit in 128 MiB, 16 .. 512."""
    return max(16, min(512, (128 << 20) // slice_bytes(n, widths)))


def wide_tile_bytes(n, widths, bwd, stage_rowlen=0, use_saved=True):
    """Footprint of one row tile of the wide kernel (wide_layout in csrc/plan.hip): 16 rows, channel stride 16 D + 4 floats;
    the input tile (the forward's block outputs replace it, so it is as large as the widest of them; the backward without
    saved inputs adds up to two block-output tiles), the z tile, the gradient tile (forward: one buffer for both, at least the
    dense [16, stage_rowlen] staging of the edge stage), the LayerNorm scratch, the row indices and the parking region of
    1 (forward) / 4 (backward) slots x CT channel tiles x D x 256 floats."""
    D, R = 1 << n, ROWS_PER_TILE
    rup = lambda x, m: (x + m - 1) // m * m
    CS = R * D + 4
    maxCPo = max(rup(o, 4) for _, o in widths)
    CT = (maxCPo + 15) // 16
    nblk = len(widths)
    sz_in, sz_o = rup(widths[0][0], 4) * CS, maxCPo * CS
    single_in = (not bwd) or (use_saved and nblk > 1)
    if single_in:
        sz_in = max(sz_in, sz_o)
    sz_g = max(sz_o, rup(R * stage_rowlen, 4)) if stage_rowlen > 0 else sz_o
    total = sz_in
    if not single_in:
        total += sz_o * ((nblk >= 2) + (nblk >= 3))
    total += sz_g if not bwd else sz_o + sz_g
    total += rup(CT * 16, 4) + rup(3 * R, 4) + (4 if bwd else 1) * CT * D * 256
    return 4 * total


def egcl_widths(C, hidden, out, edge_attr=6, node_attr=3):
    """Block widths of the edge and the node model of an EGCL layer (two blocks each)."""
    return [(C + edge_attr, hidden), (hidden, out)], [(C + out + node_attr, hidden), (hidden, out)]
