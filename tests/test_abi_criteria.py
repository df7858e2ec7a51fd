"""C-ABI boundary of the variance-reduction / entropy placement entries without a GPU: the symbols
are exported, declared and typed, the workspace queries answer, and bad arguments are reported by
position before any device work."""
import ctypes

import pytest

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = ["vgposp_symv_upper_workspace_bytes", "vgposp_symv_upper", "vgposp_symv_upper_sq",
       "vgposp_crit_workspace_bytes", "vgposp_crit_init", "vgposp_crit_step",
       "vgposp_crit_buffers"]
VARIANCE, ENTROPY = 0, 1


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2
    assert len(_lib.SIGNATURES["vgposp_symv_upper"][1]) == 9
    assert len(_lib.SIGNATURES["vgposp_crit_init"][1]) == 12
    assert len(_lib.SIGNATURES["vgposp_crit_step"][1]) == 13
    assert "criteria.hip" in _lib.KERNEL_SOURCES["criteria_symv"]
    assert len(_lib.source_hash("criteria_symv")) == 16
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert "#define VGPOSP_CRIT_VARIANCE 0" in text and "#define VGPOSP_CRIT_ENTROPY 1" in text


def test_workspace_queries():
    sy = lambda n: _lib.query("vgposp_symv_upper_workspace_bytes", n)
    assert sy(0) == 0 and sy(-3) == 0
    # column- and row-direction partials: one slab of ceil(n / 512) x n doubles each
    assert sy(1) >= 16 and sy(513) >= 2 * 2 * 513 * 8
    assert sy(512) < sy(513) < sy(2000)
    cr = lambda n, k: _lib.query("vgposp_crit_workspace_bytes", n, k)
    assert cr(0, 4) == 0 and cr(100, 0) == 0
    assert cr(1000, 4) >= (4 + 6) * 1000 * 8 + sy(1000)
    assert cr(1000, 4) < cr(1000, 5) < cr(1100, 5) < cr(2000, 5)   # (areas round up to 256 bytes)


def _init(sigma=P8, n=10, lda=10, diag=None, kmax=5, criterion=VARIANCE, thr=1e-8, targets=None,
          allowed=None, ws=P8, ws_bytes=BIG):
    return _lib.call("vgposp_crit_init", sigma, n, lda, diag, kmax, criterion, thr, targets,
                     allowed, ws, ws_bytes, None)


def test_init_argument_validation():
    with pytest.raises(_lib.VgpospError, match="bad argument 1"):
        _init(sigma=None)
    with pytest.raises(_lib.VgpospError, match="bad argument 2"):
        _init(n=0)
    with pytest.raises(_lib.VgpospError, match="bad argument 3"):
        _init(lda=9)
    with pytest.raises(_lib.VgpospError, match="bad argument 5"):
        _init(kmax=11)                            # kmax <= n
    with pytest.raises(_lib.VgpospError, match="bad argument 5"):
        _init(kmax=0)
    with pytest.raises(_lib.VgpospError, match="bad argument 6"):
        _init(criterion=2)
    with pytest.raises(_lib.VgpospError, match="bad argument 6"):
        _init(criterion=-1)
    with pytest.raises(_lib.VgpospError, match="bad argument 7"):
        _init(thr=-1.0)
    with pytest.raises(_lib.VgpospError, match="bad argument 10"):
        _init(ws=None)
    with pytest.raises(_lib.VgpospError, match="workspace 16 <"):
        _init(ws_bytes=16)


def test_step_argument_validation():
    lib = _lib.load()
    step = lambda sigma=P8, n=10, lda=10, kmax=5, rnd=0, forced=None, j=0, sel=P8, ws=P8, \
        nbytes=BIG: lib.vgposp_crit_step(sigma, n, lda, None, kmax, rnd, forced, j, sel, None, ws,
                                         nbytes, None)
    assert step(sigma=None) == -1
    assert step(n=0) == -2
    assert step(lda=9) == -3
    assert step(kmax=11) == -5
    assert step(rnd=5) == -6 and step(rnd=-1) == -6
    assert step(forced=P8, j=-1) == -8
    assert step(sel=None) == -9
    assert step(ws=None) == -11
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_symv_and_buffers_argument_validation():
    lib = _lib.load()
    for fn in (lib.vgposp_symv_upper, lib.vgposp_symv_upper_sq):
        assert fn(None, 0, 0, None, None, None, None, 0, None) == 0       # n = 0: nothing to do
        assert fn(None, 4, 4, None, P8, P8, P8, BIG, None) == -1
        assert fn(P8, -1, 4, None, P8, P8, P8, BIG, None) == -2
        assert fn(P8, 4, 3, None, P8, P8, P8, BIG, None) == -3
        assert fn(P8, 4, 4, None, None, P8, P8, BIG, None) == -5
        assert fn(P8, 4, 4, None, P8, None, P8, BIG, None) == -6
        assert fn(P8, 4, 4, None, P8, P8, None, BIG, None) == _lib.E_WS
        assert fn(P8, 4, 4, None, P8, P8, P8, 8, None) == _lib.E_WS
    ptr = [ctypes.c_void_p() for _ in range(4)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_crit_buffers(None, 10, 2, *refs) == -1
    assert lib.vgposp_crit_buffers(P8, 0, 2, *refs) == -2
    assert lib.vgposp_crit_buffers(P8, 10, 0, *refs) == -3
    assert lib.vgposp_crit_buffers(ctypes.c_void_p(4096), 10, 2, *refs) == 0
    offs = [p.value - 4096 for p in ptr]
    assert offs == sorted(offs) and offs[0] > 0 and len(set(offs)) == 4
