"""C-ABI boundary of the passes over a factored Sigma = F F^T + diag(noise) and the rounds on it
without a GPU: the symbols are exported, declared and typed, the workspace queries answer, and bad
arguments are reported by position before any device work."""
import ctypes

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 44
NEW = ["vgposp_factor_symv_workspace_bytes", "vgposp_factor_symv", "vgposp_factor_symv_sq",
       "vgposp_critf_workspace_bytes", "vgposp_critf_init", "vgposp_critf_step",
       "vgposp_critf_buffers"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_factor_symv"][1]) == 10
    assert len(_lib.SIGNATURES["vgposp_factor_symv_sq"][1]) == 10
    # (F, n, s, ldf, noise) + (kmax, criterion, threshold, targets, allowed, ws, ws_bytes, stream):
    # the prototype of the header has 13 arguments
    assert len(_lib.SIGNATURES["vgposp_critf_init"][1]) == 13
    assert len(_lib.SIGNATURES["vgposp_critf_step"][1]) == 14
    assert len(_lib.SIGNATURES["vgposp_critf_buffers"][1]) == 8
    for fam in ("criteria_fsymv", "criteria_fsymv_sq"):
        assert _lib.KERNEL_SOURCES[fam] == _lib.KERNEL_SOURCES["criteria_symv"]
        assert _lib.source_hash(fam) == _lib.source_hash("criteria_symv")


def test_workspace_queries():
    fs = lambda n, s: _lib.query("vgposp_factor_symv_workspace_bytes", n, s)
    assert fs(0, 96) == 0 and fs(-1, 96) == 0 and fs(100, 0) == 0 and fs(100, -2) == 0
    ns = [1, 2, 63, 64, 65, 1000, 16383, 16384, 16385, 65536, 65537, 262144, 1 << 21, 1 << 22]
    ss = [1, 2, 7, 64, 75, 96, 256, 300, 1024, 1025, 2048, 4096]
    for s in ss:
        got = [fs(n, s) for n in ns]
        assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])), (s, got)     # in n
        big = [fs(n, s) for n in (1000, 16384, 65536, 262144, 1 << 21, 1 << 22)]
        assert all(a < b for a, b in zip(big, big[1:])), (s, big)   # (256-byte granules below)
    for n in ns:
        got = [fs(n, s) for s in ss]
        assert all(a < b for a, b in zip(got, got[1:])), (n, got)                      # in S
    # the condition of the design: the moment matrix, a chunk of at most 16,384 rows (the GEMM's
    # split partials included), and O(n) for the diagonal; nothing of size n S
    for n in ns:
        for s in ss:
            assert fs(n, s) <= 8 * (s * s + 16384 * s) + 8 * n + 8 * s + 4 * 256, (n, s)
    assert fs(262144, 300) < 45e6 and fs(1 << 21, 256) < 55e6
    cf = lambda n, s, k: _lib.query("vgposp_critf_workspace_bytes", n, s, k)
    cr = lambda n, k: _lib.query("vgposp_crit_workspace_bytes", n, k)
    up = lambda n: _lib.query("vgposp_symv_upper_workspace_bytes", n)
    assert cf(0, 9, 4) == 0 and cf(-3, 9, 4) == 0 and cf(100, 0, 4) == 0 and cf(100, 9, 0) == 0
    assert cf(100, -1, 4) == 0 and cf(100, 9, -1) == 0
    assert cf(1000, 96, 4) < cf(1100, 96, 4) < cf(2000, 96, 4) < cf(70000, 96, 4)          # n
    assert cf(70000, 96, 4) < cf(300000, 96, 4) < cf(1 << 21, 96, 4)
    assert cf(1000, 96, 4) < cf(1000, 97, 4) < cf(1000, 300, 4) < cf(1000, 4096, 4)        # S
    assert cf(1000, 96, 4) < cf(1000, 96, 5) < cf(1000, 96, 9)                             # kmax
    # crit_layout with only the pass area sized by the new source; the diagonal vector lives in
    # that area, so nothing but 256-byte alignment is left over
    for n, s, k in ((1000, 96, 4), (5000, 75, 7), (70000, 300, 3)):
        diff = (cf(n, s, k) - fs(n, s)) - (cr(n, k) - up(n))
        assert 0 <= diff <= 8 * n + 256, (n, s, k, diff)
    # what the device holds beside F: O(n kmax), not n^2
    assert cf(262144, 300, 50) < 8 * 262144 * (50 + 10) + 45e6


def test_pass_argument_validation():
    lib = _lib.load()
    for fn in (lib.vgposp_factor_symv, lib.vgposp_factor_symv_sq):
        call = lambda F=P8, n=4, s=3, ldf=3, noise=None, x=P8, y=P8, ws=P8, nbytes=BIG: \
            fn(F, n, s, ldf, noise, x, y, ws, nbytes, None)
        # n = 0: nothing to do, nothing looked at
        assert fn(None, 0, 0, 0, None, None, None, None, 0, None) == 0
        assert call(F=None) == -1
        assert call(n=-1) == -2 and call(n=(1 << 22) + 1) == -2
        assert call(s=0, ldf=0) == -3 and call(s=4097, ldf=4097) == -3 and call(s=-1) == -3
        assert b"bad argument 3" in lib.vgposp_last_error()
        assert call(ldf=2) == -4
        assert call(x=None) == -6
        assert call(y=None) == -7
        assert call(ws=None) == _lib.E_WS
        assert call(nbytes=8) == _lib.E_WS
        assert b"workspace 8 <" in lib.vgposp_last_error()
        assert call(nbytes=_lib.query("vgposp_factor_symv_workspace_bytes", 4, 3) - 1) == _lib.E_WS


def test_critf_init_argument_validation():
    lib = _lib.load()
    init = lambda F=P8, n=10, s=6, ldf=6, kmax=5, crit=0, thr=1e-8, ws=P8, nbytes=BIG: \
        lib.vgposp_critf_init(F, n, s, ldf, None, kmax, crit, thr, None, None, ws, nbytes, None)
    assert init(F=None) == -1
    # the rounds share their scoring and selection kernels with vgposp_crit_step: n <= 2^21,
    # one above it is refused although the passes alone go to 2^22
    assert init(n=0) == -2 and init(n=(1 << 21) + 1) == -2
    assert init(s=0, ldf=0) == -3 and init(s=4097, ldf=5000) == -3
    assert init(ldf=5) == -4
    assert init(kmax=11) == -6 and init(kmax=0) == -6                # 1 <= kmax <= n
    assert init(crit=2) == -7
    assert init(thr=-1.0) == -8
    assert b"bad argument 8" in lib.vgposp_last_error()
    assert init(ws=None) == -11
    assert init(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()
    assert init(nbytes=_lib.query("vgposp_critf_workspace_bytes", 10, 6, 5) - 1) == _lib.E_WS


def test_critf_step_argument_validation():
    lib = _lib.load()
    step = lambda F=P8, n=10, s=6, ldf=6, kmax=5, rnd=0, forced=None, j=0, sel=P8, ws=P8, \
        nbytes=BIG: lib.vgposp_critf_step(F, n, s, ldf, None, kmax, rnd, forced, j, sel, None, ws,
                                          nbytes, None)
    assert step(F=None) == -1
    assert step(n=0) == -2 and step(n=(1 << 21) + 1) == -2
    assert step(s=0, ldf=0) == -3 and step(s=4097, ldf=5000) == -3
    assert step(ldf=5) == -4
    assert step(kmax=11) == -6 and step(kmax=0) == -6
    assert step(rnd=5) == -7 and step(rnd=-1) == -7
    assert step(forced=P8, j=-1) == -9
    assert step(sel=None) == -10
    assert step(ws=None) == -12
    assert step(nbytes=16) == _lib.E_WS
    assert b"workspace 16 <" in lib.vgposp_last_error()


def test_buffers_argument_validation():
    lib = _lib.load()
    ptr = [ctypes.c_void_p() for _ in range(4)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_critf_buffers(None, 10, 6, 2, *refs) == -1
    assert lib.vgposp_critf_buffers(P8, 0, 6, 2, *refs) == -2
    assert lib.vgposp_critf_buffers(P8, 10, 0, 2, *refs) == -3
    assert lib.vgposp_critf_buffers(P8, 10, 6, 0, *refs) == -4
    assert lib.vgposp_critf_buffers(ctypes.c_void_p(4096), 10, 6, 2, *refs) == 0
    # nom, score, delta and W lie where vgposp_crit_buffers puts them: the same kernels run on them
    old = [ctypes.c_void_p() for _ in range(4)]
    assert lib.vgposp_crit_buffers(ctypes.c_void_p(4096), 10, 2,
                                   *[ctypes.byref(p) for p in old]) == 0
    assert [p.value for p in old] == [p.value for p in ptr]
    assert lib.vgposp_critf_buffers(ctypes.c_void_p(4096), 10, 6, 2, None, None, None, None) == 0
