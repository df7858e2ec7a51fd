"""C-ABI boundary of the mutual-information placement on a factored covariance (vgposp_fmi_*)
without a GPU: the symbols are exported, declared and typed, the workspace query answers, bad
arguments are reported by position under the entry's own name before any device work."""
import ctypes

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 44
NEW = ["vgposp_fmi_workspace_bytes", "vgposp_fmi_init", "vgposp_fmi_step", "vgposp_fmi_buffers"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
        # the prefixes tests/test_abi_criteria_names.py and test_abi_greedy_names.py enumerate
        assert not name.startswith("vgposp_crit") and not name.startswith("vgposp_greedy_")
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_fmi_workspace_bytes"][1]) == 3
    # (F, n, s, ldf, noise) + (kmax, threshold, allowed, info, ws, ws_bytes, stream)
    assert len(_lib.SIGNATURES["vgposp_fmi_init"][1]) == 12
    # (F, n, s, ldf, noise) + (kmax, round, forced, j, selected, sel_delta, ws, ws_bytes, stream)
    assert len(_lib.SIGNATURES["vgposp_fmi_step"][1]) == 14
    assert len(_lib.SIGNATURES["vgposp_fmi_buffers"][1]) == 9
    assert _lib.SIGNATURES["vgposp_fmi_step"] == _lib.SIGNATURES["vgposp_critf_step"]
    assert _lib.KERNEL_SOURCES["criteria_fmi_row"] == _lib.KERNEL_SOURCES["criteria_fsymv"]


def test_workspace_query():
    q = lambda n, s, k: _lib.query("vgposp_fmi_workspace_bytes", n, s, k)
    for bad in ((0, 9, 4), (-3, 9, 4), (100, 0, 4), (100, -1, 4), (100, 9, 0), (100, 9, -1)):
        assert q(*bad) == 0, bad
    shapes = [(1, 1, 1), (10, 6, 5), (257, 129, 16), (200, 4096, 8), (65536, 300, 50),
              (262144, 96, 50), (1 << 21, 256, 50)]
    for n, s, k in shapes:
        assert q(n, s, k) >= 8 * (2 * k * n + s * s), (n, s, k)
    assert q(1000, 96, 4) < q(1100, 96, 4) < q(2000, 96, 4) < q(70000, 96, 4)               # n
    assert q(1000, 96, 4) < q(1000, 97, 4) < q(1000, 300, 4) < q(1000, 4096, 4)             # S
    assert q(1000, 96, 4) < q(1000, 96, 5) < q(1000, 96, 9)                                 # kmax
    # what the device holds beside F: the two row sets, O(n) vectors, two S x S matrices, the
    # chunk area of the factored passes and the S x S factorization's workspace; never n^2, n S
    fs = lambda n, s: _lib.query("vgposp_factor_symv_workspace_bytes", n, s)
    po = lambda s: _lib.query("vgposp_potrf_compact_workspace_bytes", s)
    for n, s, k in shapes:
        assert q(n, s, k) <= 8 * n * (2 * k + 5) + 8 * s * s + fs(n, s) + po(s) + 64 * 1024, \
            (n, s, k)


def test_init_argument_validation():
    lib = _lib.load()
    init = lambda F=P8, n=10, s=6, ldf=6, noise=P8, kmax=5, thr=1e-8, info=P8, ws=P8, nbytes=BIG: \
        lib.vgposp_fmi_init(F, n, s, ldf, noise, kmax, thr, None, info, ws, nbytes, None)
    assert init(F=None) == -1
    assert b"vgposp_fmi_init: bad argument 1" in lib.vgposp_last_error()
    assert init(n=0) == -2 and init(n=(1 << 21) + 1) == -2
    assert init(s=0, ldf=0) == -3 and init(s=4097, ldf=5000) == -3
    assert init(ldf=5) == -4
    assert init(noise=None) == -5                                    # D must be invertible
    assert b"vgposp_fmi_init: bad argument 5" in lib.vgposp_last_error()
    assert init(kmax=11) == -6 and init(kmax=0) == -6                # 1 <= kmax <= n
    assert init(thr=-1.0) == -7
    assert b"vgposp_fmi_init: bad argument 7" in lib.vgposp_last_error()
    assert init(info=None) == -9
    assert init(ws=None) == -10
    assert init(nbytes=16) == _lib.E_WS
    assert b"vgposp_fmi_init: workspace 16 <" in lib.vgposp_last_error()
    assert init(nbytes=_lib.query("vgposp_fmi_workspace_bytes", 10, 6, 5) - 1) == _lib.E_WS


def test_step_argument_validation():
    lib = _lib.load()
    step = lambda F=P8, n=10, s=6, ldf=6, noise=P8, kmax=5, rnd=0, forced=None, j=0, sel=P8, \
        ws=P8, nbytes=BIG: lib.vgposp_fmi_step(F, n, s, ldf, noise, kmax, rnd, forced, j, sel,
                                               None, ws, nbytes, None)
    assert step(F=None) == -1
    assert step(n=0) == -2 and step(n=(1 << 21) + 1) == -2
    assert step(s=0, ldf=0) == -3 and step(s=4097, ldf=5000) == -3
    assert step(ldf=5) == -4
    assert step(noise=None) == -5
    assert step(kmax=11) == -6 and step(kmax=0) == -6
    assert step(rnd=5) == -7 and step(rnd=-1) == -7
    assert b"vgposp_fmi_step: bad argument 7" in lib.vgposp_last_error()
    assert step(forced=P8, j=-1) == -9
    assert step(sel=None) == -10
    assert step(ws=None) == -12
    assert step(nbytes=16) == _lib.E_WS
    assert b"vgposp_fmi_step: workspace 16 <" in lib.vgposp_last_error()


def test_buffers():
    lib = _lib.load()
    ptr = [ctypes.c_void_p() for _ in range(5)]
    refs = [ctypes.byref(p) for p in ptr]
    assert lib.vgposp_fmi_buffers(None, 10, 6, 2, *refs) == -1
    assert lib.vgposp_fmi_buffers(P8, 0, 6, 2, *refs) == -2
    assert lib.vgposp_fmi_buffers(P8, 10, 0, 2, *refs) == -3
    assert lib.vgposp_fmi_buffers(P8, 10, 4097, 2, *refs) == -3
    assert lib.vgposp_fmi_buffers(P8, 10, 6, 0, *refs) == -4
    assert b"vgposp_fmi_buffers: bad argument 4" in lib.vgposp_last_error()
    base = 4096
    assert lib.vgposp_fmi_buffers(ctypes.c_void_p(base), 10, 6, 2, *refs) == 0
    off = [p.value - base for p in ptr]
    # nom, prec, delta [n], then W and V [kmax][n]: ascending, disjoint, inside the workspace
    assert off[0] > 0 and all(b - a >= 8 * 10 for a, b in zip(off, off[1:4]))
    assert off[4] - off[3] >= 8 * 2 * 10
    assert off[4] + 8 * 2 * 10 <= _lib.query("vgposp_fmi_workspace_bytes", 10, 6, 2)
    # independent of where the workspace lies
    other = [ctypes.c_void_p() for _ in range(5)]
    assert lib.vgposp_fmi_buffers(ctypes.c_void_p(1 << 30), 10, 6, 2,
                                  *[ctypes.byref(p) for p in other]) == 0
    assert [p.value - (1 << 30) for p in other] == off
    # every output is optional
    assert lib.vgposp_fmi_buffers(ctypes.c_void_p(base), 10, 6, 2, None, None, None, None,
                                  None) == 0
    only = ctypes.c_void_p()
    assert lib.vgposp_fmi_buffers(ctypes.c_void_p(base), 10, 6, 2, None, None, None, None,
                                  ctypes.byref(only)) == 0
    assert only.value - base == off[4]
