"""The compact Cholesky workspace query without a GPU: it differs from the full workspace
(tests/test_abi_layout.py) only in the split-K partials area, min(2^23, 8 n^2) doubles instead of
2^23 for n > 128, whatever the Strassen setting adds behind it."""
import pytest

from vgposp_amd import _lib

q = _lib.query


@pytest.mark.parametrize("n", [1, 128, 129, 256, 512, 513, 640, 1000, 1023, 1024, 2048, 8192])
def test_compact_workspace_is_full_minus_unused_partials(n):
    full = q("vgposp_potrf_workspace_bytes", n)
    compact = q("vgposp_potrf_compact_workspace_bytes", n)
    part = (1 << 23) if n > 128 else 0
    assert compact == full - 8 * (part - min(part, 8 * n * n))
    if n <= 128 or n >= 1024:
        assert compact == full


def test_compact_workspace_small_orders():
    assert q("vgposp_potrf_compact_workspace_bytes", 0) == 0
    # n = 256: two leaf inverses, the 128 x 128 trtri panel, 8 n^2 partials, 64 spare doubles
    assert q("vgposp_potrf_compact_workspace_bytes", 256) == 8 * (3 * 128 * 128 + 8 * 256 * 256 + 64)
    assert q("vgposp_potrf_compact_workspace_bytes", 256) < 5 << 20
