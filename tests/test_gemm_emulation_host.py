"""Host side of the int8 emulation of fp64 products (gemm_emul.hip), no GPU: the Garner
reconstruction against Python integers, and what the setting does to the workspace queries."""
import ctypes
import random

import pytest

MODULI = [256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217, 211, 199, 197, 193]
P = 1
for _p in MODULI:
    P *= _p


def _sym(x, p):
    """x mod p in [-(p-1)/2, (p-1)/2] (odd p) or [-128, 127] (256)."""
    r = x % p
    return r - p if r > (p - 1) // 2 else r


# p_j^-1 mod p_t, symmetric, j < t: the 120 constants of Garner's algorithm
INV = [[_sym(pow(MODULI[j], -1, MODULI[t]), MODULI[t]) for j in range(t)] for t in range(16)]


def garner(res):
    """Mixed-radix digits (symmetric) of the residue class, in plain Python integers."""
    v = []
    for t, p in enumerate(MODULI):
        x = res[t]
        for j in range(t):
            x = (x - v[j]) * INV[t][j] % p
        v.append(_sym(x, p))
    return v


def value(v):
    y = 0
    for t in reversed(range(16)):
        y = y * MODULI[t] + v[t]
    return y


def _cases():
    rnd = random.Random(7)
    half = (P - 1) // 2
    return [0, 1, -1, half, -half] + [rnd.randrange(-half, half + 1) for _ in range(10000)]


def test_moduli_are_coprime_and_large_enough():
    from math import gcd, log2
    assert all(gcd(a, b) == 1 for i, a in enumerate(MODULI) for b in MODULI[:i])
    assert abs(log2(P) - 125.37) < 0.01


def test_python_garner_round_trips():
    for x in _cases():
        v = garner([x % p for p in MODULI])
        assert value(v) == x
        assert -128 <= v[0] <= 127 and all(abs(v[t]) <= (MODULI[t] - 1) // 2 for t in range(1, 16))


def test_library_garner_equals_python():
    """The reconstruction the kernel runs (the same inline functions, compiled for the host):
    residues given as arbitrary representatives up to 2^30, as the int32 products deliver them."""
    from vgposp_amd import _lib
    lib = _lib.load()
    rnd = random.Random(11)
    R, D, V = (ctypes.c_int32 * 16)(), (ctypes.c_int32 * 16)(), ctypes.c_double()
    for x in _cases():
        for t, p in enumerate(MODULI):
            R[t] = x % p + p * rnd.randrange(-(2 ** 30) // p + 1, 2 ** 30 // p - 1)
        assert lib.vgposp_gemm_emulation_garner(R, D, ctypes.byref(V)) == 0
        assert list(D) == garner([x % p for p in MODULI])
        assert V.value == float(x)  # int -> float rounds once, to nearest even


class emulation_setting:
    """vgposp_potrf_set_emulation(min_dim, moduli) for a with-block; restores the previous one."""

    def __init__(self, min_dim, moduli):
        self.new = (min_dim, moduli)

    def __enter__(self):
        from vgposp_amd import _lib
        md, mo = ctypes.c_int64(), ctypes.c_int()
        _lib.call("vgposp_potrf_emulation", ctypes.byref(md), ctypes.byref(mo))
        self.old = (md.value, mo.value)
        _lib.call("vgposp_potrf_set_emulation", *self.new)
        return self

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_potrf_set_emulation", *self.old)
        return False


def _emul_need_32768():
    """The walk's need at n = 32,768, threshold 8,192: the plain products of the top split are
    8192 x 8192 x 16384 (SYRK), 16384 x 8192 x 8192 (TRSM, TRMM-B) and 8192 x 16384 x 8192
    (TRMM-A); the half-size nodes' have a dimension below the threshold."""
    from vgposp_amd import _lib
    return max(_lib.query("vgposp_gemm_emulated_workspace_bytes", *s)
               for s in ((8192, 8192, 16384), (16384, 8192, 8192), (8192, 16384, 8192)))


def test_workspace_queries():
    from vgposp_amd import _lib
    with emulation_setting(8192, 0):
        off = {n: _lib.query("vgposp_potrf_workspace_bytes", n) for n in (16384, 32768)}
        goff = _lib.query("vgposp_greedy_workspace_bytes", 2048, 10)
    # the default leaves everything below 32,768 as it is without emulation
    assert _lib.query("vgposp_potrf_workspace_bytes", 16384) == off[16384]
    assert _lib.query("vgposp_greedy_workspace_bytes", 2048, 10) == goff
    with emulation_setting(8192, 16):
        assert _lib.query("vgposp_potrf_workspace_bytes", 16384) == off[16384]
        assert _lib.query("vgposp_greedy_workspace_bytes", 2048, 10) == goff
        on = _lib.query("vgposp_potrf_workspace_bytes", 32768)
        if _lib.load().vgposp_gemm_emulation_available():
            need = (_emul_need_32768() + 7) // 8 * 8
            assert 0 <= on - off[32768] - need < 256  # (the area starts on a 256-byte boundary)
            _lib.call("vgposp_gemm_emulation_set_unavailable", 1)
            try:
                assert _lib.query("vgposp_potrf_workspace_bytes", 32768) == off[32768]
            finally:
                _lib.call("vgposp_gemm_emulation_set_unavailable", 0)
        else:
            assert on == off[32768]


@pytest.mark.parametrize("bad", [(0, 16), (300, 16), (-256, 16), (8192, 8), (8192, -1), (8192, 17)])
def test_bad_settings_are_rejected(bad):
    from vgposp_amd import _lib
    lib = _lib.load()
    md, mo = ctypes.c_int64(), ctypes.c_int()
    _lib.call("vgposp_potrf_emulation", ctypes.byref(md), ctypes.byref(mo))
    before = (md.value, mo.value)
    assert lib.vgposp_potrf_set_emulation(*bad) != 0
    _lib.call("vgposp_potrf_emulation", ctypes.byref(md), ctypes.byref(mo))
    assert (md.value, mo.value) == before
