"""CPU (no GPU needed): the C-ABI surface of the deterministic training step - csmpn_mvlinear_backward_det,
csmpn_type_attr_backward_det and their host-only scratch queries (include/csmpn_hip.h), and ops.det_launches()."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_NAME = "clifford-group-equivariant-simplicial-message-passing-networks_amd"

NEW = ["csmpn_mvlinear_backward_det_bytes", "csmpn_mvlinear_backward_det", "csmpn_type_attr_backward_det_bytes",
       "csmpn_type_attr_backward_det"]
# (n, in_features, out_features, subspaces): md17's feature embedding, a head, the hulls embedding, NBA's feature embedding
MVLINEAR_SHAPES = [(3, 35, 32, 0), (3, 32, 10, 1), (5, 1, 28, 0), (2, 43, 40, 0)]
MV_MAX_SLABS, MV_MIN_SLAB = 512, 8          # the documented cap: min(ceil(rows / 8), 512) slabs
TYPE_MAX_GROUPS, TYPE_ROW_BYTES = 256, 256   # min(ceil(rows / floor(256 / K)), 256) partial rows of 64 floats


def test_new_names_are_exported(pkg):
    from csmpn_hip import native
    lib = native.lib()
    for name in NEW:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.csmpn_abi_version() == 2


@pytest.mark.parametrize("n,I,O,sub", MVLINEAR_SHAPES)
def test_mvlinear_det_bytes(pkg, n, I, O, sub):
    from csmpn_hip import native
    q = native.lib().csmpn_mvlinear_backward_det_bytes
    nelem = O * I * ((n + 1) if sub else 1) + O
    cap_rows = (MV_MAX_SLABS - 1) * MV_MIN_SLAB + 1      # the first row count with 512 slabs
    rows = [1, 7, 8, 9, 940, cap_rows - 1, cap_rows, 20_000, 100_000, 10 ** 9]
    got = [int(q(n, r, I, O, sub)) for r in rows]
    assert all(b > 0 for b in got)
    assert all(a <= b for a, b in zip(got, got[1:])), got
    cap = MV_MAX_SLABS * nelem * 4
    assert got[rows.index(cap_rows) - 1] < cap and all(b == cap for b in got[rows.index(cap_rows):]), got
    assert got[0] == got[1] == nelem * 4                  # below the smallest slab: one partial row
    # a real launch never has more slabs than the query counts: slab >= 8 rows and >= rows / 512
    for r, b in zip(rows, got):
        assert b == min(-(-r // MV_MIN_SLAB), MV_MAX_SLABS) * nelem * 4
    for bad in ((n, 0, I, O, sub), (n, -5, I, O, sub), (n, 100, 0, O, sub), (n, 100, I, -1, sub), (0, 100, I, O, sub),
                (9, 100, I, O, sub)):
        assert int(q(*bad)) == 0, bad


@pytest.mark.parametrize("T,K,N,E", [(3, 3, 300, 2999), (3, 3, 1, 0), (2, 32, 17, 5)])
def test_type_attr_det_bytes(pkg, T, K, N, E):
    from csmpn_hip import native
    q = native.lib().csmpn_type_attr_backward_det_bytes
    assert int(q(T, K, N, E)) > 0
    rpp = 256 // K
    cap_rows = (TYPE_MAX_GROUPS - 1) * rpp + 1
    rows = sorted({1, rpp, rpp + 1, 3299, cap_rows - 1, cap_rows, 100_000, 10 ** 9})
    for split in (lambda r: (r, 0), lambda r: (0, r), lambda r: (r // 3, r - r // 3)):
        got = [int(q(T, K, *split(r))) for r in rows]
        assert got == [min(-(-r // rpp), TYPE_MAX_GROUPS) * TYPE_ROW_BYTES for r in rows], got
        assert all(a <= b for a, b in zip(got, got[1:]))
        assert got[rows.index(cap_rows) - 1] < got[rows.index(cap_rows)] == got[-1] == TYPE_MAX_GROUPS * TYPE_ROW_BYTES
    for bad in ((T, K, 0, 0), (T, K, -1, 5), (T, K, 5, -1), (T, 0, N, E), (0, K, N, E), (9, 8, N, E)):
        assert int(q(*bad)) == 0, bad


def test_det_launches_is_zero_in_a_fresh_process(pkg):
    from csmpn_hip import ops
    assert callable(ops.det_launches) and isinstance(ops.det_launches(), int)
    code = (f"import importlib, sys; sys.path.insert(0, {ROOT!r}); importlib.import_module({PKG_NAME!r}); "
            "from csmpn_hip import ops; print('det_launches', ops.det_launches())")
    flags = ["-s"] if sys.flags.no_user_site else []
    out = subprocess.run([sys.executable, *flags, "-c", code], capture_output=True, text=True, check=True).stdout
    assert out.split()[-2:] == ["det_launches", "0"], out
