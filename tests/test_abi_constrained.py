"""C-ABI boundary of the constrained-placement entries without a GPU: the symbols are exported,
declared and typed, the scratch query answers, and bad arguments are reported by position before
any device work."""
import ctypes

import pytest

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = ["vgposp_greedy_mask", "vgposp_greedy_force", "vgposp_greedy_condition_workspace_bytes",
       "vgposp_greedy_condition"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2
    res, args = _lib.SIGNATURES["vgposp_greedy_condition"]
    assert res is ctypes.c_int and len(args) == 14
    res, args = _lib.SIGNATURES["vgposp_greedy_condition_workspace_bytes"]
    assert res is ctypes.c_size_t and len(args) == 2


def test_scratch_query():
    q = lambda n, b: _lib.query("vgposp_greedy_condition_workspace_bytes", n, b)
    assert q(1100, 1) > 0
    # T slices of the ceil(n / 512) x n partial sums, and the T extracted columns
    assert q(1100, 4) >= 4 * 3 * 1100 * 8 + 4 * 1100 * 8
    assert q(1100, 8) >= 2 * q(1100, 4) - 1024
    assert q(1100, 3) == 0 and q(1100, 0) == 0 and q(0, 4) == 0
    # the greedy workspace and its layout do not depend on the batch
    assert _lib.query("vgposp_greedy_workspace_bytes", 1100, 10) > 0


def _condition(n=10, lda=10, kmax=5, m=3, k=2, batch=4, placed=P8, selected=P8, ws=P8,
               ws_bytes=BIG, scratch=P8, scratch_bytes=BIG, sigma=P8):
    return _lib.call("vgposp_greedy_condition", sigma, n, lda, kmax, m, k, batch, placed, selected,
                     ws, ws_bytes, scratch, scratch_bytes, None)


def test_condition_argument_validation():
    with pytest.raises(_lib.VgpospError, match="bad argument 1"):
        _condition(sigma=None)
    with pytest.raises(_lib.VgpospError, match="bad argument 3"):
        _condition(lda=9)
    with pytest.raises(_lib.VgpospError, match="bad argument 4"):
        _condition(kmax=11)                       # kmax <= n
    with pytest.raises(_lib.VgpospError, match="bad argument 5"):
        _condition(m=0)
    with pytest.raises(_lib.VgpospError, match="bad argument 6"):
        _condition(m=3, k=3)                      # m + k <= kmax
    with pytest.raises(_lib.VgpospError, match="bad argument 7"):
        _condition(batch=0)
    with pytest.raises(_lib.VgpospError, match="bad argument 7"):
        _condition(batch=3)
    with pytest.raises(_lib.VgpospError, match="bad argument 8"):
        _condition(placed=None)
    with pytest.raises(_lib.VgpospError, match="bad argument 9"):
        _condition(selected=None)
    with pytest.raises(_lib.VgpospError, match="workspace is null"):
        _condition(ws=None)
    with pytest.raises(_lib.VgpospError, match="workspace 16 <"):
        _condition(ws_bytes=16)
    with pytest.raises(_lib.VgpospError, match="bad argument 12"):
        _condition(scratch=None)
    with pytest.raises(_lib.VgpospError, match="scratch 16 <"):
        _condition(scratch_bytes=16)


def test_mask_and_force_argument_validation():
    lib = _lib.load()
    assert lib.vgposp_greedy_mask(None, 10, 2, P8, None) == -1
    assert lib.vgposp_greedy_mask(P8, 0, 2, P8, None) == -2
    assert lib.vgposp_greedy_mask(P8, 10, 11, P8, None) == -3
    assert lib.vgposp_greedy_mask(P8, 10, 2, None, None) == -4
    assert lib.vgposp_greedy_force(10, 5, 5, P8, 0, P8, P8, BIG, None) == -3   # round < kmax
    assert lib.vgposp_greedy_force(10, 5, 1, None, 0, P8, P8, BIG, None) == -4
    assert lib.vgposp_greedy_force(10, 5, 1, P8, -1, P8, P8, BIG, None) == -5
    assert lib.vgposp_greedy_force(10, 5, 1, P8, 0, None, P8, BIG, None) == -6
    assert lib.vgposp_greedy_force(10, 5, 1, P8, 0, P8, None, BIG, None) == _lib.E_WS
    assert lib.vgposp_greedy_force(10, 5, 1, P8, 0, P8, P8, 16, None) == _lib.E_WS
