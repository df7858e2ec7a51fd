"""C-ABI boundary of the matrix-free pass and the rounds on a generated cross-covariance without a
GPU: the symbols are exported, declared and typed, the workspace queries answer, and bad arguments
are reported by position before any device work."""
import ctypes
import re

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = ["vgposp_kernel_gemv_t_workspace_bytes", "vgposp_kernel_gemv_t", "vgposp_kernel_gemv_t_sq",
       "vgposp_critk_workspace_bytes", "vgposp_critk_init", "vgposp_critk_step",
       "vgposp_critk_buffers"]


def _header_rows():
    with open(_lib.HEADER_PATH) as f:
        return int(re.search(r"#define\s+VGPOSP_KGEMV_ROWS\s+(\d+)", f.read()).group(1))


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_kernel_gemv_t"][1]) == 15
    assert len(_lib.SIGNATURES["vgposp_kernel_gemv_t_sq"][1]) == 15
    assert len(_lib.SIGNATURES["vgposp_critk_init"][1]) == 20
    assert len(_lib.SIGNATURES["vgposp_critk_step"][1]) == 22
    assert len(_lib.SIGNATURES["vgposp_critk_buffers"][1]) == 9
    assert _lib.KGEMV_ROWS == _header_rows() and _lib.KGEMV_ROWS >= 1
    for fam in ("criteria_kgemv_t", "criteria_kgemv_t_sq"):
        assert {"criteria.hip", "psd.h"} <= set(_lib.KERNEL_SOURCES[fam])
        assert len(_lib.source_hash(fam)) == 16
    # the stored pass's families are what they were
    assert _lib.source_hash("criteria_gemv_t") == _lib.source_hash("criteria_symv")


def test_workspace_queries():
    H = _lib.KGEMV_ROWS
    gv = lambda P, n: _lib.query("vgposp_kernel_gemv_t_workspace_bytes", P, n)
    assert gv(0, 5) == 0 and gv(5, 0) == 0 and gv(-1, 5) == 0 and gv(0, 0) == 0
    # one partial per (row chunk, column)
    for P, n in ((1, 1), (H, 100), (H + 1, 100), (3 * H + 1, 1025), (100000, 4096)):
        assert gv(P, n) >= -(-P // H) * n * 8
    assert gv(H, 100) < gv(H + 1, 100)
    assert gv(4 * H, 100) < gv(4 * H, 200) and gv(4 * H, 200) < gv(8 * H, 200)
    ck = lambda n, P, k: _lib.query("vgposp_critk_workspace_bytes", n, P, k)
    assert ck(0, 100, 4) == 0 and ck(100, 0, 4) == 0 and ck(100, 100, 0) == 0
    cr = _lib.query("vgposp_crit_workspace_bytes", 1000, 4)
    assert ck(1000, 5000, 4) >= cr + (4 + 2) * 5000 * 8 + gv(5000, 1000)
    assert ck(1000, 5000, 4) < ck(1100, 5000, 4) < ck(2000, 5000, 4)      # n
    assert ck(1000, 5000, 4) < ck(1000, 5100, 4) < ck(1000, 9000, 4)      # P
    assert ck(1000, 5000, 4) < ck(1000, 5000, 5) < ck(1000, 5000, 9)      # kmax
    # critx_layout with only the partials area sized by the new pass
    cx = _lib.query("vgposp_critx_workspace_bytes", 1000, 5000, 4)
    assert ck(1000, 5000, 4) - gv(5000, 1000) == \
        cx - _lib.query("vgposp_gemv_t_workspace_bytes", 5000, 1000)


def test_pass_argument_validation():
    lib = _lib.load()
    for fn in (lib.vgposp_kernel_gemv_t, lib.vgposp_kernel_gemv_t_sq):
        call = lambda kind=0, Xt=P8, P=6, X=P8, n=4, d=3, amp=P8, ls=P8, at=None, a_s=None, x=P8, \
            y=P8, ws=P8, nbytes=BIG: fn(kind, Xt, P, X, n, d, amp, ls, at, a_s, x, y, ws, nbytes,
                                        None)
        # an empty dimension: nothing to do, nothing looked at
        assert fn(9, None, 0, None, 4, 0, None, None, None, None, None, None, None, 0, None) == 0
        assert fn(9, None, 6, None, 0, 0, None, None, None, None, None, None, None, 0, None) == 0
        assert call(kind=4) == -1 and call(kind=-1) == -1
        assert call(Xt=None) == -2
        assert call(P=-1) == -3 and call(P=(1 << 24) + 1) == -3
        assert call(X=None) == -4
        assert call(n=-1) == -5 and call(n=(1 << 21) + 1) == -5
        assert call(d=0) == -6 and call(d=9) == -6
        assert b"bad argument 6" in lib.vgposp_last_error()
        assert call(amp=None) == -7
        assert call(ls=None) == -8
        assert call(x=None) == -11
        assert call(y=None) == -12
        assert call(ws=None) == _lib.E_WS
        assert call(nbytes=8) == _lib.E_WS
        assert b"workspace 8 <" in lib.vgposp_last_error()


def test_init_argument_validation():
    lib = _lib.load()
    init = lambda sigma=P8, n=10, lda=10, kind=0, Xt=P8, P=30, X=P8, d=3, amp=P8, ls=P8, kmax=5, \
        thr=1e-8, ws=P8, nbytes=BIG: lib.vgposp_critk_init(
            sigma, n, lda, None, kind, Xt, P, X, d, amp, ls, None, None, None, kmax, thr, None, ws,
            nbytes, None)
    assert init(sigma=None) == -1
    assert init(n=0) == -2
    assert init(lda=9) == -3
    assert init(kind=4) == -5
    assert init(Xt=None) == -6
    assert init(P=0) == -7 and init(P=-4) == -7
    assert init(X=None) == -8
    assert init(d=0) == -9 and init(d=9) == -9
    assert init(amp=None) == -10
    assert init(ls=None) == -11
    assert init(kmax=11) == -15 and init(kmax=0) == -15              # 1 <= kmax <= n
    assert init(thr=-1.0) == -16
    assert b"bad argument 16" in lib.vgposp_last_error()
    assert init(ws=None) == -18
    assert init(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_step_argument_validation():
    lib = _lib.load()
    step = lambda sigma=P8, n=10, lda=10, kind=0, Xt=P8, P=30, X=P8, d=3, amp=P8, ls=P8, kmax=5, \
        rnd=0, forced=None, j=0, sel=P8, ws=P8, nbytes=BIG: lib.vgposp_critk_step(
            sigma, n, lda, None, kind, Xt, P, X, d, amp, ls, None, None, kmax, rnd, forced, j, sel,
            None, ws, nbytes, None)
    assert step(sigma=None) == -1
    assert step(n=0) == -2
    assert step(lda=9) == -3
    assert step(kind=-1) == -5
    assert step(Xt=None) == -6
    assert step(P=0) == -7
    assert step(X=None) == -8
    assert step(d=9) == -9
    assert step(amp=None) == -10
    assert step(ls=None) == -11
    assert step(kmax=11) == -14
    assert step(rnd=5) == -15 and step(rnd=-1) == -15
    assert step(forced=P8, j=-1) == -17
    assert step(sel=None) == -18
    assert step(ws=None) == -20
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_buffers_argument_validation():
    lib = _lib.load()
    ptr = [ctypes.c_void_p() for _ in range(5)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_critk_buffers(None, 10, 30, 2, *refs) == -1
    assert lib.vgposp_critk_buffers(P8, 0, 30, 2, *refs) == -2
    assert lib.vgposp_critk_buffers(P8, 10, 0, 2, *refs) == -3
    assert lib.vgposp_critk_buffers(P8, 10, 30, 0, *refs) == -4
    assert lib.vgposp_critk_buffers(ctypes.c_void_p(4096), 10, 30, 2, *refs) == 0
    offs = [p.value - 4096 for p in ptr]
    assert offs == sorted(offs) and offs[0] > 0 and len(set(offs)) == 5
    # the location side lies where vgposp_crit_buffers puts it, and U where vgposp_critx_buffers
    # does: the same kernels run on both
    old = [ctypes.c_void_p() for _ in range(4)]
    assert lib.vgposp_crit_buffers(ctypes.c_void_p(4096), 10, 2,
                                   *[ctypes.byref(p) for p in old]) == 0
    assert [p.value for p in old] == [p.value for p in ptr[:4]]
    cx = [ctypes.c_void_p() for _ in range(5)]
    assert lib.vgposp_critx_buffers(ctypes.c_void_p(4096), 10, 30, 2,
                                    *[ctypes.byref(p) for p in cx]) == 0
    assert [p.value for p in cx] == [p.value for p in ptr]
    assert offs[4] >= _lib.query("vgposp_crit_workspace_bytes", 10, 2)
