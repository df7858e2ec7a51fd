"""The Cholesky and TRSM workspace queries against the layout of DESIGN.md §2, written out here
independently of the library's own layout code (host-only: no GPU needed)."""
import ctypes

import pytest

from vgposp_amd import _lib

q = _lib.query
SIZES = [1, 128, 129, 512, 513, 640, 1000, 1024, 2048, 4096]


def _potrf_elems(n, part):
    """Doubles of one matrix's workspace without Strassen scratch: leaf inverses, the trtri panel
    of the top split, the 512-wide block inverses and TRSM output, split-K partials, 64 spare."""
    leaves = -(-n // 128)
    n1 = 128 * (leaves // 2) if n > 128 else 0
    return (leaves * 128 * 128 + n1 * (n - n1) + (2 * 512 * n if n > 512 else 0)
            + (part if n > 128 else 0) + 64)


@pytest.fixture(scope="module")
def classical():
    """Strassen off (levels = 0) for the module, the setting restored afterwards."""
    md, lv = ctypes.c_int64(), ctypes.c_int()
    _lib.call("vgposp_potrf_strassen", ctypes.byref(md), ctypes.byref(lv))
    _lib.call("vgposp_potrf_set_strassen", 512, 0)
    yield
    _lib.call("vgposp_potrf_set_strassen", md.value, lv.value)


@pytest.mark.parametrize("n", SIZES)
def test_potrf_workspace_layout(classical, n):
    single = 8 * _potrf_elems(n, 1 << 23)       # 64 MiB of partials
    per = 8 * _potrf_elems(n, 1 << 21)          # a batch: 16 MiB per matrix
    assert q("vgposp_potrf_workspace_bytes", n) == single
    for b in (1, 3, 4):
        assert q("vgposp_potrf_batched_workspace_bytes", n, b) == max(b * per, single)


@pytest.mark.parametrize("n", SIZES)
def test_trsm_workspace_layout(n):
    # leaf inverses, the leaves' out-of-place 128 x m output, 16 MiB of partials, 64 spare
    for m in (1, 7, 300):
        assert q("vgposp_trsm_workspace_bytes", n, m) == \
            8 * (-(-n // 128) * 128 * 128 + 128 * m + (1 << 21) + 64)
