"""C-ABI boundary of the field reconstruction on a factored covariance (vgposp_fpost_*) without a
GPU: the symbols are exported, declared and typed, the workspace query answers and is monotone, bad
arguments are reported by position under the entry's own name before any device work."""
import ctypes

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 44
NEW = ["vgposp_fpost_workspace_bytes", "vgposp_fpost_init", "vgposp_fpost_apply"]


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name)
        assert name in _lib.SIGNATURES
        assert name in _lib.header_symbols()
        assert not name.startswith("vgposp_crit") and not name.startswith("vgposp_greedy_")
    assert lib.vgposp_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert len(_lib.SIGNATURES["vgposp_fpost_workspace_bytes"][1]) == 4
    # (F, n, s, ldf, noise) + (sensors, k, obs_noise, info, ws, ws_bytes, stream)
    assert len(_lib.SIGNATURES["vgposp_fpost_init"][1]) == 12
    # (F, n, s, ldf, noise) + (k, var, Y, ldy, nrhs, mu, out, ldo, ws, ws_bytes, stream)
    assert len(_lib.SIGNATURES["vgposp_fpost_apply"][1]) == 16
    for scope in ("criteria_fpost_init", "criteria_fpost_rhs", "criteria_fpost_stream"):
        assert "criteria.hip" in _lib.KERNEL_SOURCES[scope]
    assert _lib.KERNEL_SOURCES["criteria_fpost_stream"] == _lib.KERNEL_SOURCES["criteria_fsymv"]


def test_workspace_query():
    q = lambda n, s, k, b: _lib.query("vgposp_fpost_workspace_bytes", n, s, k, b)
    for bad in ((0, 9, 4, 2), (-3, 9, 4, 2), (100, 0, 4, 2), (100, -1, 4, 2), (100, 9, 0, 2),
                (100, 9, -1, 2)):
        assert q(*bad) == 0, bad
    assert q(100, 9, 4, 0) > 0 and q(100, 9, 4, -5) == q(100, 9, 4, 0)
    shapes = [(1, 1, 1, 0), (10, 6, 5, 1), (257, 129, 16, 3), (200, 4096, 8, 70),
              (65536, 300, 50, 78), (262144, 96, 50, 14), (1 << 21, 256, 50, 64),
              (1 << 22, 4096, 1024, 1024)]
    po = lambda k: _lib.query("vgposp_potrf_compact_workspace_bytes", k)
    pad = lambda c: (c + 15) // 16 * 16
    for n, s, k, b in shapes:
        lo = 8 * (n + 2 * k * s + k * k + (3 * k + s) * b)
        hi = 8 * (n + 3 * k + k * s + pad(k) * s + k * k + (3 * k + s) * pad(b)) + po(k) \
            + 12 * 256
        assert lo <= q(n, s, k, b) <= hi, (n, s, k, b)      # never n k, never n s
    # monotone in every argument, strictly across what changes an area's size
    assert q(1000, 96, 4, 3) < q(1100, 96, 4, 3) < q(2000, 96, 4, 3) < q(70000, 96, 4, 3)     # n
    assert q(1000, 96, 4, 3) < q(1000, 97, 4, 3) < q(1000, 300, 4, 3) < q(1000, 4096, 4, 3)   # S
    assert q(1000, 96, 4, 3) < q(1000, 96, 5, 3) < q(1000, 96, 17, 3) < q(1000, 96, 1024, 3)  # k
    assert q(1000, 96, 4, 0) < q(1000, 96, 4, 1) <= q(1000, 96, 4, 16) < q(1000, 96, 4, 17) \
        < q(1000, 96, 4, 1024)                                                              # nrhs
    last = 0
    for k in range(1, 1025, 7):
        assert q(3000, 50, k, 5) >= last
        last = q(3000, 50, k, 5)
    # beyond the limits the query stays finite: the entries refuse those
    assert q(1000, 5000, 4, 3) == q(1000, 4096, 4, 3)
    assert q(3000, 96, 2000, 3) == q(3000, 96, 1024, 3)
    assert q(1000, 96, 4, 5000) == q(1000, 96, 4, 1024)


def test_init_argument_validation():
    lib = _lib.load()
    init = lambda F=P8, n=10, s=6, ldf=6, noise=P8, sensors=P8, k=5, s2=0.0, info=P8, ws=P8, \
        nbytes=BIG: lib.vgposp_fpost_init(F, n, s, ldf, noise, sensors, k, s2, info, ws, nbytes,
                                          None)
    assert init(F=None) == -1
    assert b"vgposp_fpost_init: bad argument 1" in lib.vgposp_last_error()
    assert init(n=0) == -2 and init(n=(1 << 22) + 1, k=5) == -2
    assert init(s=0, ldf=0) == -3 and init(s=4097, ldf=5000) == -3
    assert init(ldf=5) == -4
    assert init(sensors=None) == -6
    assert b"vgposp_fpost_init: bad argument 6" in lib.vgposp_last_error()
    assert init(k=0) == -7 and init(k=11) == -7                      # 1 <= k <= n
    assert init(n=5000, k=1025) == -7                                # k <= 1,024
    assert b"vgposp_fpost_init: bad argument 7" in lib.vgposp_last_error()
    assert init(s2=-1e-9) == -8 and init(s2=float("nan")) == -8 and init(s2=float("inf")) == -8
    assert init(info=None) == -9
    assert init(ws=None) == -10
    assert init(nbytes=16) == _lib.E_WS
    assert b"vgposp_fpost_init: workspace 16 <" in lib.vgposp_last_error()
    # init needs no room for readings; one byte short of that is refused
    assert init(nbytes=_lib.query("vgposp_fpost_workspace_bytes", 10, 6, 5, 0) - 1) == _lib.E_WS
    assert init(noise=None, F=None) == -1                            # noise may be NULL


def test_apply_argument_validation():
    lib = _lib.load()
    apply = lambda F=P8, n=10, s=6, ldf=6, noise=P8, k=5, var=P8, Y=P8, ldy=3, nrhs=3, mu=None, \
        out=P8, ldo=3, ws=P8, nbytes=BIG: lib.vgposp_fpost_apply(F, n, s, ldf, noise, k, var, Y,
                                                                 ldy, nrhs, mu, out, ldo, ws,
                                                                 nbytes, None)
    assert apply(F=None) == -1
    assert apply(n=0) == -2 and apply(n=(1 << 22) + 1) == -2
    assert apply(s=0, ldf=0) == -3 and apply(s=4097, ldf=5000) == -3
    assert apply(ldf=5) == -4
    assert apply(k=0) == -6 and apply(k=11) == -6 and apply(n=5000, k=1025) == -6
    assert b"vgposp_fpost_apply: bad argument 6" in lib.vgposp_last_error()
    assert apply(ldy=2) == -9
    assert apply(nrhs=-1) == -10 and apply(nrhs=1025, ldy=2000, ldo=2000) == -10
    assert b"vgposp_fpost_apply: bad argument 10" in lib.vgposp_last_error()
    assert apply(out=None) == -12
    assert apply(ldo=2) == -13
    assert apply(ws=None) == -14
    assert apply(nbytes=16) == _lib.E_WS
    assert b"vgposp_fpost_apply: workspace 16 <" in lib.vgposp_last_error()
    q = lambda b: _lib.query("vgposp_fpost_workspace_bytes", 10, 6, 5, b)
    assert apply(nbytes=q(3) - 1) == _lib.E_WS
    # a workspace sized for fewer readings than asked for is short
    assert apply(nrhs=17, ldy=17, ldo=17, nbytes=q(16)) == _lib.E_WS
