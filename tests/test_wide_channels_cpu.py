"""CPU (no GPU needed): host-side sizing of the wide CEMLP / EGCL path (65..256 output channels, cemlp_wide.hpp).

csmpn_cemlp_workspace_bytes and csmpn_cemlp_saved_floats cover the wide bindings and grow with the width; the deterministic
copies of the gradient tensors (n <= 3) are bounded instead of 512 copies of a slice that grows with O^2; widths above 256
still report no workspace-free plan (the launch returns CSMPN_ERR_UNSUPPORTED: tests/test_wide_channels_gpu.py::
test_wide_width_boundaries_and_refusal_above_256_channels)."""
import pytest

from wide_helpers import slice_bytes


def _node_binding(n, C, attr=3, nblk=2):
    from csmpn_hip import ops
    specs = [{"in_features": 2 * C + attr if k == 0 else C, "out_features": C} for k in range(nblk)]
    return ops.CemlpBinding((1.0,) * n, specs)


def _sizes(n, C, rows=1000):
    from csmpn_hip import native
    b = _node_binding(n, C)
    lib = native.lib()
    return (int(lib.csmpn_cemlp_workspace_bytes(b.n, b.params, b.nblk)),
            int(lib.csmpn_cemlp_saved_floats(b.n, b.params, b.nblk, rows, 0)),
            int(lib.csmpn_cemlp_saved_floats_per_row(b.n, b.params, b.nblk)))


def _slice_bytes(n, C, attr=3):
    """Bytes of one copy of the gradient tensors of a node model's two blocks (tests/wide_helpers.py::slice_bytes)."""
    return slice_bytes(n, [(2 * C + attr, C), (C, C)])


@pytest.mark.parametrize("n", [2, 3, 4, 5])
def test_wide_workspace_and_saved_grow_with_width(pkg, n):
    prev = None
    for C in (96, 128, 256):
        ws, saved, per_row = _sizes(n, C)
        assert ws > 0 and saved > 0 and per_row > 0, (n, C)
        # the block-1 input ([rows, C, D]) is saved
        assert saved >= 1000 * C * (1 << n) and per_row >= C * (1 << n)
        if prev is not None:
            assert ws > prev[0] and saved > prev[1], (n, C, prev, ws, saved)
        prev = (ws, saved)


@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("C", [128, 256])
def test_wide_deterministic_reservation_is_bounded(pkg, n, C):
    """The per-workgroup gradient copies of the deterministic mode are at most max(128 MiB, 16 copies): the whole workspace of
    a 128- or 256-channel node model stays below 1 GiB, far below 512 copies (0.5 GB at 128 channels, 3.8 GB at 256)."""
    ws, _, _ = _sizes(n, C)
    slice_bytes = _slice_bytes(n, C)
    assert ws < (1 << 30), (n, C, ws)
    assert ws < 512 * slice_bytes // 2, (n, C, ws, slice_bytes)
    assert ws > max(128 << 20, 16 * slice_bytes), (n, C, ws, slice_bytes)   # ... and the copies are reserved


def test_widths_up_to_64_keep_their_workspace(pkg):
    """Dispatch invariance, host side: the sizing of 8..64-channel bindings is not the wide kernel's (no parking region,
    512 deterministic copies for n <= 3)."""
    for C in (8, 16, 32, 64):
        ws, saved, _ = _sizes(3, C)
        assert ws >= 512 * _slice_bytes(3, C), (C, ws)
