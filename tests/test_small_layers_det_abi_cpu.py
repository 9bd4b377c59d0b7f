"""CPU (no GPU needed): the C-ABI surface of the deterministic forms of the four standalone small layers -
csmpn_mvsilu_backward_det, csmpn_mvnorm_backward_det, csmpn_mvlayernorm_forward_det / _backward_det,
csmpn_wgp_backward_det and the host-only scratch query csmpn_small_layer_det_bytes (include/csmpn_hip.h)."""
import pytest

NEW = ["csmpn_small_layer_det_bytes", "csmpn_mvsilu_backward_det", "csmpn_mvnorm_backward_det",
       "csmpn_mvlayernorm_forward_det", "csmpn_mvlayernorm_backward_det", "csmpn_wgp_backward_det"]
MAX_PARTS, TILE = 512, 256      # the documented cap: min(tiles, 512) partial rows; a tile = 256 lanes
OPS = ["mvsilu", "mvnorm", "mvlayernorm", "wgp"]


def op_id(native, op):
    return {"mvsilu": native.LAYER_MVSILU, "mvnorm": native.LAYER_MVNORM, "mvlayernorm": native.LAYER_MVLAYERNORM,
            "wgp": native.LAYER_WGP}[op]


def entries(pkg, op, n, C):
    """Floats of one partial row: 2(n+1)C, (n+1)C, C, P*C."""
    if op == "wgp":
        return int(pkg.CliffordAlgebra((1.0,) * n).geometric_product_paths.sum()) * C
    return {"mvsilu": 2 * (n + 1) * C, "mvnorm": (n + 1) * C, "mvlayernorm": C}[op]


def tiles(op, rows, C):
    """The documented tile count: 256 consecutive (row, channel) elements, for MVLayerNorm floor(256 / C) whole rows."""
    return -(-rows // (TILE // C)) if op == "mvlayernorm" else -(-(rows * C) // TILE)


def first_rows_with_tiles(op, C, want):
    """The smallest row count with `want` tiles."""
    per = TILE // C
    return (want - 1) * per + 1 if op == "mvlayernorm" else ((want - 1) * TILE) // C + 1


def test_new_names_are_exported(pkg):
    from csmpn_hip import native
    lib = native.lib()
    for name in NEW:
        assert name in native.EXPORTS and hasattr(lib, name), name
    assert lib.csmpn_abi_version() == 2
    assert (native.LAYER_MVSILU, native.LAYER_MVNORM, native.LAYER_MVLAYERNORM, native.LAYER_WGP) == (0, 1, 2, 3)


def test_path_count_depends_on_n_alone(pkg):
    """The query takes n, not the metric: the grade paths of Cl(3,1) / Cl(4,1) are those of Cl(4,0) / Cl(5,0)."""
    for metric in ((1.0, 1.0, 1.0, -1.0), (1.0, 1.0, 1.0, 1.0, -1.0)):
        a, b = pkg.CliffordAlgebra(metric), pkg.CliffordAlgebra((1.0,) * len(metric))
        assert int(a.geometric_product_paths.sum()) == int(b.geometric_product_paths.sum())


@pytest.mark.parametrize("C", [1, 3, 33, 256])
@pytest.mark.parametrize("n", [2, 3, 4, 5])
@pytest.mark.parametrize("op", OPS)
def test_small_layer_det_bytes(pkg, op, n, C):
    from csmpn_hip import native
    q = native.lib().csmpn_small_layer_det_bytes
    o, row_bytes = op_id(native, op), entries(pkg, op, n, C) * 4
    cap_rows = first_rows_with_tiles(op, C, MAX_PARTS)          # constant from here on
    assert tiles(op, cap_rows, C) == MAX_PARTS and (cap_rows == 1 or tiles(op, cap_rows - 1, C) == MAX_PARTS - 1)
    rows = sorted({1, 2, 5, 37, 257, 1031, max(cap_rows - 1, 1), cap_rows, cap_rows + 1, 3 * cap_rows, 100_000, 10 ** 9})
    got = [int(q(o, n, r, C)) for r in rows]
    assert all(b > 0 for b in got), got
    assert all(a <= b for a, b in zip(got, got[1:])), got
    assert all(b % row_bytes == 0 for b in got), (got, row_bytes)
    assert all(b <= MAX_PARTS * row_bytes for b in got), got
    assert got == [min(tiles(op, r, C), MAX_PARTS) * row_bytes for r in rows], got
    at = rows.index(cap_rows)
    assert all(b == MAX_PARTS * row_bytes for b in got[at:]), got
    if cap_rows > 1:
        assert got[at - 1] < MAX_PARTS * row_bytes
    for bad in ((o, n, 0, C), (o, n, -3, C), (o, n, 100, 0), (o, n, 100, 257), (o, 0, 100, C), (o, 1, 100, C), (o, 6, 100, C),
                (4, n, 100, C), (-1, n, 100, C)):
        assert int(q(*bad)) == 0, bad
