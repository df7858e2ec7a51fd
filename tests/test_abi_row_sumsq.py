"""C-ABI boundary of vgposp_row_sumsq without a GPU: the symbol is exported and typed, an empty
problem returns before any device work, and a bad argument is reported by its position."""
import ctypes

import pytest

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced


def test_row_sumsq_exported_and_typed():
    lib = _lib.load()
    assert hasattr(lib, "vgposp_row_sumsq")
    assert "vgposp_row_sumsq" in _lib.SIGNATURES
    assert "vgposp_row_sumsq" in _lib.header_symbols()
    res, args = _lib.SIGNATURES["vgposp_row_sumsq"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[4] is ctypes.c_double and args[5] is ctypes.c_double


def test_row_sumsq_zero_rows_returns_zero():
    assert _lib.call("vgposp_row_sumsq", None, 0, 5, 5, 1.0, 0.0, None, None) == 0
    assert _lib.call("vgposp_row_sumsq", P8, 0, 0, 0, -1.0, 1.0, P8, None) == 0


def test_row_sumsq_argument_validation():
    with pytest.raises(_lib.VgpospError, match="bad argument 2"):
        _lib.call("vgposp_row_sumsq", P8, -1, 4, 4, 1.0, 0.0, P8, None)
    with pytest.raises(_lib.VgpospError, match="bad argument 3"):
        _lib.call("vgposp_row_sumsq", P8, 2, -1, 4, 1.0, 0.0, P8, None)
    with pytest.raises(_lib.VgpospError, match="bad argument 4"):
        _lib.call("vgposp_row_sumsq", P8, 2, 5, 4, 1.0, 0.0, P8, None)
    with pytest.raises(_lib.VgpospError, match="bad argument 1"):
        _lib.call("vgposp_row_sumsq", None, 2, 4, 4, 1.0, 0.0, P8, None)
    with pytest.raises(_lib.VgpospError, match="bad argument 7"):
        _lib.call("vgposp_row_sumsq", P8, 2, 4, 4, 1.0, 0.0, None, None)
