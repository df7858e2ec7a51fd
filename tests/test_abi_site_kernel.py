"""C-ABI boundary of the pass over a generated Sigma and the rounds on it without a GPU: the symbols
are exported, declared and typed, the workspace queries answer, and bad arguments are reported by
position before any device work."""
import ctypes

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = ["vgposp_kernel_symv_workspace_bytes", "vgposp_kernel_symv", "vgposp_kernel_symv_sq",
       "vgposp_critg_workspace_bytes", "vgposp_critg_init", "vgposp_critg_step",
       "vgposp_critg_buffers", "vgposp_critgk_workspace_bytes", "vgposp_critgk_init",
       "vgposp_critgk_step", "vgposp_critgk_buffers"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    assert len(NEW) == 11
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_kernel_symv"][1]) == 13
    assert len(_lib.SIGNATURES["vgposp_kernel_symv_sq"][1]) == 13
    assert len(_lib.SIGNATURES["vgposp_critg_init"][1]) == 16
    assert len(_lib.SIGNATURES["vgposp_critg_step"][1]) == 17
    assert len(_lib.SIGNATURES["vgposp_critg_buffers"][1]) == 7
    assert len(_lib.SIGNATURES["vgposp_critgk_init"][1]) == 18
    assert len(_lib.SIGNATURES["vgposp_critgk_step"][1]) == 20
    assert len(_lib.SIGNATURES["vgposp_critgk_buffers"][1]) == 9
    for fam in ("criteria_ksymv", "criteria_ksymv_sq"):
        assert {"criteria.hip", "psd.h"} <= set(_lib.KERNEL_SOURCES[fam])
        assert _lib.source_hash(fam) == _lib.source_hash("criteria_kgemv_t")
    assert _lib.source_hash("criteria_gemv_t") == _lib.source_hash("criteria_symv")


def test_workspace_queries():
    ks = lambda n: _lib.query("vgposp_kernel_symv_workspace_bytes", n)
    assert ks(0) == 0 and ks(-1) == 0
    sizes = [1, 2, 511, 512, 513, 4096, 4097, 32768, 32769, 65536, 65537, 229376, 229377, 262144,
             262145, 1 << 20, 1 << 21]
    got = [ks(n) for n in sizes]
    # monotone in n (256-byte granules: strictly from 512 on)
    assert got[0] >= 16 and all(a <= b for a, b in zip(got, got[1:]))
    assert all(a < b for a, b in zip(got[3:], got[4:]))
    # the condition of the design: one partial per (group of 8 tiles, column) in each direction,
    # plus O(n): at most 1 KiB per site below the size at which the groups hold 8 x 8 tiles
    for n, b in zip(sizes, got):
        assert b <= 16 * n * -(-n // 4096) + 1024 * n + 512, n
    assert ks(1 << 21) <= 16 * (1 << 21) * 512 + 512
    assert ks(262144) <= 0.27e9
    cg = lambda n, k: _lib.query("vgposp_critg_workspace_bytes", n, k)
    cr = lambda n, k: _lib.query("vgposp_crit_workspace_bytes", n, k)
    assert cg(0, 4) == 0 and cg(-3, 4) == 0 and cg(100, 0) == 0 and cg(100, -1) == 0
    assert cg(1000, 4) < cg(1100, 4) < cg(2000, 4) < cg(70000, 4) < cg(300000, 4)     # n
    assert cg(1000, 4) < cg(1000, 5) < cg(1000, 9)                                     # kmax
    # crit_layout with only the partials area sized by the new pass
    up = lambda n: _lib.query("vgposp_symv_upper_workspace_bytes", n)
    for n, k in ((1000, 4), (5000, 7), (70000, 3)):
        assert cg(n, k) - ks(n) == cr(n, k) - up(n)
        assert cg(n, k) >= cr(n, k) - up(n)
    gk = lambda n, P, k: _lib.query("vgposp_critgk_workspace_bytes", n, P, k)
    ck = lambda n, P, k: _lib.query("vgposp_critk_workspace_bytes", n, P, k)
    assert gk(0, 100, 4) == 0 and gk(100, 0, 4) == 0 and gk(100, 100, 0) == 0
    assert gk(1000, 5000, 4) < gk(1100, 5000, 4) < gk(2000, 5000, 4)      # n
    assert gk(1000, 5000, 4) < gk(1000, 5100, 4) < gk(1000, 9000, 4)      # P
    assert gk(1000, 5000, 4) < gk(1000, 5000, 5) < gk(1000, 5000, 9)      # kmax
    # the rounds never pass over Sigma: critk's workspace less the partials of its pass
    assert gk(1000, 5000, 4) == ck(1000, 5000, 4) - up(1000)
    assert gk(70000, 5000, 4) == ck(70000, 5000, 4) - up(70000)


def test_pass_argument_validation():
    lib = _lib.load()
    for fn in (lib.vgposp_kernel_symv, lib.vgposp_kernel_symv_sq):
        call = lambda kind=0, X=P8, n=4, d=3, amp=P8, ls=P8, a=None, dg=None, x=P8, y=P8, ws=P8, \
            nbytes=BIG: fn(kind, X, n, d, amp, ls, a, dg, x, y, ws, nbytes, None)
        # n = 0: nothing to do, nothing looked at
        assert fn(9, None, 0, 0, None, None, None, None, None, None, None, 0, None) == 0
        assert call(kind=4) == -1 and call(kind=-1) == -1
        assert call(X=None) == -2
        assert call(n=-1) == -3 and call(n=(1 << 21) + 1) == -3
        assert call(d=0) == -4 and call(d=9) == -4
        assert b"bad argument 4" in lib.vgposp_last_error()
        assert call(amp=None) == -5
        assert call(ls=None) == -6
        assert call(x=None) == -9
        assert call(y=None) == -10
        assert call(ws=None) == _lib.E_WS
        assert call(nbytes=8) == _lib.E_WS
        assert b"workspace 8 <" in lib.vgposp_last_error()


def test_critg_init_argument_validation():
    lib = _lib.load()
    init = lambda kind=0, X=P8, n=10, d=3, amp=P8, ls=P8, kmax=5, crit=0, thr=1e-8, ws=P8, \
        nbytes=BIG: lib.vgposp_critg_init(kind, X, n, d, amp, ls, None, None, kmax, crit, thr,
                                          None, None, ws, nbytes, None)
    assert init(kind=4) == -1
    assert init(X=None) == -2
    assert init(n=0) == -3 and init(n=(1 << 21) + 1) == -3
    assert init(d=0) == -4 and init(d=9) == -4
    assert init(amp=None) == -5
    assert init(ls=None) == -6
    assert init(kmax=11) == -9 and init(kmax=0) == -9                # 1 <= kmax <= n
    assert init(crit=2) == -10
    assert init(thr=-1.0) == -11
    assert b"bad argument 11" in lib.vgposp_last_error()
    assert init(ws=None) == -14
    assert init(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_critg_step_argument_validation():
    lib = _lib.load()
    step = lambda kind=0, X=P8, n=10, d=3, amp=P8, ls=P8, kmax=5, rnd=0, forced=None, j=0, \
        sel=P8, ws=P8, nbytes=BIG: lib.vgposp_critg_step(kind, X, n, d, amp, ls, None, None, kmax,
                                                         rnd, forced, j, sel, None, ws, nbytes,
                                                         None)
    assert step(kind=-1) == -1
    assert step(X=None) == -2
    assert step(n=0) == -3
    assert step(d=9) == -4
    assert step(amp=None) == -5
    assert step(ls=None) == -6
    assert step(kmax=11) == -9
    assert step(rnd=5) == -10 and step(rnd=-1) == -10
    assert step(forced=P8, j=-1) == -12
    assert step(sel=None) == -13
    assert step(ws=None) == -15
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_critgk_init_argument_validation():
    lib = _lib.load()
    init = lambda n=10, kind=0, Xt=P8, P=30, X=P8, d=3, amp=P8, ls=P8, kmax=5, thr=1e-8, ws=P8, \
        nbytes=BIG: lib.vgposp_critgk_init(n, None, kind, Xt, P, X, d, amp, ls, None, None, None,
                                           kmax, thr, None, ws, nbytes, None)
    assert init(n=0) == -1
    assert init(kind=4) == -3
    assert init(Xt=None) == -4
    assert init(P=0) == -5 and init(P=-4) == -5
    assert init(X=None) == -6
    assert init(d=0) == -7 and init(d=9) == -7
    assert init(amp=None) == -8
    assert init(ls=None) == -9
    assert init(kmax=11) == -13 and init(kmax=0) == -13
    assert init(thr=-1.0) == -14
    assert b"bad argument 14" in lib.vgposp_last_error()
    assert init(ws=None) == -16
    assert init(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_critgk_step_argument_validation():
    lib = _lib.load()
    step = lambda n=10, kind=0, Xt=P8, P=30, X=P8, d=3, amp=P8, ls=P8, kmax=5, rnd=0, forced=None, \
        j=0, sel=P8, ws=P8, nbytes=BIG: lib.vgposp_critgk_step(
            n, None, kind, Xt, P, X, d, amp, ls, None, None, kmax, rnd, forced, j, sel, None, ws,
            nbytes, None)
    assert step(n=0) == -1
    assert step(kind=-1) == -3
    assert step(Xt=None) == -4
    assert step(P=0) == -5
    assert step(X=None) == -6
    assert step(d=9) == -7
    assert step(amp=None) == -8
    assert step(ls=None) == -9
    assert step(kmax=11) == -12
    assert step(rnd=5) == -13 and step(rnd=-1) == -13
    assert step(forced=P8, j=-1) == -15
    assert step(sel=None) == -16
    assert step(ws=None) == -18
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_buffers_argument_validation():
    lib = _lib.load()
    ptr = [ctypes.c_void_p() for _ in range(4)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_critg_buffers(None, 10, 2, *refs) == -1
    assert lib.vgposp_critg_buffers(P8, 0, 2, *refs) == -2
    assert lib.vgposp_critg_buffers(P8, 10, 0, *refs) == -3
    assert lib.vgposp_critg_buffers(ctypes.c_void_p(4096), 10, 2, *refs) == 0
    # nom, score, delta and W lie where vgposp_crit_buffers puts them: the same kernels run on them
    old = [ctypes.c_void_p() for _ in range(4)]
    assert lib.vgposp_crit_buffers(ctypes.c_void_p(4096), 10, 2,
                                   *[ctypes.byref(p) for p in old]) == 0
    assert [p.value for p in old] == [p.value for p in ptr]
    p5 = [ctypes.c_void_p() for _ in range(5)]
    r5 = [ctypes.byref(p) for p in p5]
    assert lib.vgposp_critgk_buffers(None, 10, 30, 2, *r5) == -1
    assert lib.vgposp_critgk_buffers(P8, 0, 30, 2, *r5) == -2
    assert lib.vgposp_critgk_buffers(P8, 10, 0, 2, *r5) == -3
    assert lib.vgposp_critgk_buffers(P8, 10, 30, 0, *r5) == -4
    assert lib.vgposp_critgk_buffers(ctypes.c_void_p(4096), 10, 30, 2, *r5) == 0
    offs = [p.value - 4096 for p in p5]
    assert offs == sorted(offs) and offs[0] > 0 and len(set(offs)) == 5
    assert [p.value for p in p5[:4]] == [p.value for p in old]
    assert offs[4] >= _lib.query("vgposp_critg_workspace_bytes", 10, 2) \
        - _lib.query("vgposp_kernel_symv_workspace_bytes", 10)
