"""C-ABI boundary of the rectangular mat-vec and the cross-covariance placement entries without a
GPU: the symbols are exported, declared and typed, the workspace queries answer, and bad arguments
are reported by position before any device work."""
import ctypes

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = ["vgposp_gemv_t_workspace_bytes", "vgposp_gemv_t", "vgposp_gemv_t_sq",
       "vgposp_critx_workspace_bytes", "vgposp_critx_init", "vgposp_critx_step",
       "vgposp_critx_buffers"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_gemv_t"][1]) == 9
    assert len(_lib.SIGNATURES["vgposp_gemv_t_sq"][1]) == 9
    assert len(_lib.SIGNATURES["vgposp_critx_init"][1]) == 14
    assert len(_lib.SIGNATURES["vgposp_critx_step"][1]) == 16
    assert len(_lib.SIGNATURES["vgposp_critx_buffers"][1]) == 9
    for fam in ("criteria_gemv_t", "criteria_gemv_t_sq"):
        assert "criteria.hip" in _lib.KERNEL_SOURCES[fam]
        assert _lib.source_hash(fam) == _lib.source_hash("criteria_symv")


def test_workspace_queries():
    gv = lambda P, n: _lib.query("vgposp_gemv_t_workspace_bytes", P, n)
    assert gv(0, 5) == 0 and gv(5, 0) == 0 and gv(-1, 5) == 0 and gv(0, 0) == 0
    # one partial per (512-row tile, column)
    assert gv(1, 1) >= 8 and gv(513, 100) >= 2 * 100 * 8 and gv(512, 100) < gv(513, 100)
    assert gv(2000, 100) < gv(2000, 200) and gv(2000, 200) < gv(4000, 200)
    cx = lambda n, P, k: _lib.query("vgposp_critx_workspace_bytes", n, P, k)
    assert cx(0, 100, 4) == 0 and cx(100, 0, 4) == 0 and cx(100, 100, 0) == 0
    cr = _lib.query("vgposp_crit_workspace_bytes", 1000, 4)
    assert cx(1000, 5000, 4) >= cr + (4 + 2) * 5000 * 8 + gv(5000, 1000)
    assert cx(1000, 5000, 4) < cx(1100, 5000, 4) < cx(2000, 5000, 4)      # n
    assert cx(1000, 5000, 4) < cx(1000, 5100, 4) < cx(1000, 9000, 4)      # P
    assert cx(1000, 5000, 4) < cx(1000, 5000, 5) < cx(1000, 5000, 9)      # kmax


def test_gemv_t_argument_validation():
    lib = _lib.load()
    for fn in (lib.vgposp_gemv_t, lib.vgposp_gemv_t_sq):
        assert fn(None, 0, 4, 4, None, None, None, 0, None) == 0      # P = 0: nothing to do
        assert fn(None, 4, 0, 0, None, None, None, 0, None) == 0      # n = 0: nothing to do
        assert fn(None, 6, 4, 4, P8, P8, P8, BIG, None) == -1
        assert fn(P8, -1, 4, 4, P8, P8, P8, BIG, None) == -2
        assert fn(P8, 6, -1, 4, P8, P8, P8, BIG, None) == -3
        assert fn(P8, 6, 4, 3, P8, P8, P8, BIG, None) == -4
        assert b"bad argument 4" in lib.vgposp_last_error()
        assert fn(P8, 6, 4, 4, None, P8, P8, BIG, None) == -5
        assert fn(P8, 6, 4, 4, P8, None, P8, BIG, None) == -6
        assert fn(P8, 6, 4, 4, P8, P8, None, BIG, None) == _lib.E_WS
        assert fn(P8, 6, 4, 4, P8, P8, P8, 8, None) == _lib.E_WS
        assert b"workspace 8 <" in lib.vgposp_last_error()


def test_init_argument_validation():
    lib = _lib.load()
    init = lambda sigma=P8, n=10, lda=10, R=P8, P=30, ldr=10, kmax=5, thr=1e-8, ws=P8, \
        nbytes=BIG: lib.vgposp_critx_init(sigma, n, lda, None, R, P, ldr, None, kmax, thr, None,
                                          ws, nbytes, None)
    assert init(sigma=None) == -1
    assert init(n=0) == -2
    assert init(lda=9) == -3
    assert init(R=None) == -5
    assert init(P=0) == -6 and init(P=-4) == -6
    assert init(ldr=9) == -7
    assert init(kmax=11) == -9 and init(kmax=0) == -9                # 1 <= kmax <= n
    assert init(thr=-1.0) == -10
    assert b"bad argument 10" in lib.vgposp_last_error()
    assert init(ws=None) == -12
    assert init(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_step_argument_validation():
    lib = _lib.load()
    step = lambda sigma=P8, n=10, lda=10, R=P8, P=30, ldr=10, kmax=5, rnd=0, forced=None, j=0, \
        sel=P8, ws=P8, nbytes=BIG: lib.vgposp_critx_step(sigma, n, lda, None, R, P, ldr, kmax, rnd,
                                                         forced, j, sel, None, ws, nbytes, None)
    assert step(sigma=None) == -1
    assert step(n=0) == -2
    assert step(lda=9) == -3
    assert step(R=None) == -5
    assert step(P=0) == -6
    assert step(ldr=9) == -7
    assert step(kmax=11) == -8
    assert step(rnd=5) == -9 and step(rnd=-1) == -9
    assert step(forced=P8, j=-1) == -11
    assert step(sel=None) == -12
    assert step(ws=None) == -14
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_buffers_argument_validation():
    lib = _lib.load()
    ptr = [ctypes.c_void_p() for _ in range(5)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_critx_buffers(None, 10, 30, 2, *refs) == -1
    assert lib.vgposp_critx_buffers(P8, 0, 30, 2, *refs) == -2
    assert lib.vgposp_critx_buffers(P8, 10, 0, 2, *refs) == -3
    assert lib.vgposp_critx_buffers(P8, 10, 30, 0, *refs) == -4
    assert lib.vgposp_critx_buffers(ctypes.c_void_p(4096), 10, 30, 2, *refs) == 0
    offs = [p.value - 4096 for p in ptr]
    assert offs == sorted(offs) and offs[0] > 0 and len(set(offs)) == 5
    # the location side lies where vgposp_crit_buffers puts it: the same kernels run on it
    old = [ctypes.c_void_p() for _ in range(4)]
    assert lib.vgposp_crit_buffers(ctypes.c_void_p(4096), 10, 2,
                                   *[ctypes.byref(p) for p in old]) == 0
    assert [p.value for p in old] == [p.value for p in ptr[:4]]
    assert offs[4] >= _lib.query("vgposp_crit_workspace_bytes", 10, 2)
