"""The batched epilogue of the fast GEMM kernels (vgposp_gemm_set_epilogue(1)) against the
element-wise reference (0): every product is run with both on the same operands and the whole C
buffer, padding and unwritten parts included, must be bit-identical; one case of each family is
also checked against a NumPy fp64 product at the tolerance of tests/test_gpu_linalg.py's GEMM
tests.

The shapes are the smallest at which each branch of the epilogue can go wrong.  It decides per
128 x 128 tile: interior tiles (whole inside C and, for a lower C, below the diagonal) take the
path without tests, edge and diagonal tiles the masked one; beta = 0 destinations must not read
C (it is filled with NaN here); a split-K launch writes partials; the Strassen products write
two or four destinations with their own alpha and beta; the grouped kernel shares the body.
128 x 128 x 16 is one interior tile, 130 x 254 has edge tiles in both directions, 384 x 384
lower has three diagonal and three interior tiles.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-11, 1e-11  # test_gemm_all_flags / test_gemm_beta01 in tests/test_gpu_linalg.py
FULL, LOWER = 0, 1


@pytest.fixture(scope="module")
def L():
    from vgposp_amd import linalg
    torch.cuda.set_device(0)
    return linalg


class epilogue_setting:
    """vgposp_gemm_set_epilogue(v) for a with-block; restores the previous setting."""

    def __init__(self, v):
        self.new = v

    def __enter__(self):
        from vgposp_amd import _lib
        self.old = int(_lib.load().vgposp_gemm_epilogue())
        _lib.call("vgposp_gemm_set_epilogue", self.new)
        return self

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_gemm_set_epilogue", self.old)
        return False


def _bits(t):
    return t.contiguous().view(torch.int64)


def _both(run, buf0):
    """run(buf) under epilogue 0 and 1 on device copies of the host buffer buf0 (any shape: the
    whole allocation C lives in); returns the epilogue-1 buffer (host) after checking that the two
    are equal bit for bit, NaN payloads included."""
    out = []
    for v in (0, 1):
        buf = torch.as_tensor(buf0, dtype=torch.float64).cuda()
        with epilogue_setting(v):
            run(buf)
            torch.cuda.synchronize()
        out.append(buf.cpu())
    assert torch.equal(_bits(out[0]), _bits(out[1])), "epilogue 1 differs from epilogue 0"
    return out[1].numpy()


def _operands(m, n, k, ta, tb, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    C0 = rng.standard_normal((m, n))
    return A, B, C0


def _ref(A, B, C0, ta, tb, alpha, beta, tri_a=0, tri_b=0):
    opA = np.tril(A) if tri_a else A
    opB = np.tril(B) if tri_b else B
    opA = opA.T if ta else opA
    opB = opB.T if tb else opB
    return alpha * opA @ opB + (beta * C0 if beta != 0.0 else 0.0)


def _gemm_case(L, m, n, k, ta, tb, alpha, beta, tri_a=0, tri_b=0, uplo=FULL, numpy_check=True,
               pad=0, shift=0):
    """One vgposp_gemm with C inside a buffer of row pitch n + pad that starts `shift` doubles
    into its allocation.  beta = 0: C starts as NaN and must come out finite."""
    from vgposp_amd._lib import call
    A, B, C0 = _operands(m, n, k, ta, tb, seed=m + 7 * n + 13 * k + ta + 2 * tb + 4 * tri_a + 8 * tri_b)
    if beta == 0.0:
        C0 = np.full((m, n), np.nan)
    Ad, Bd = L.as_device(A), L.as_device(B)
    ldc = n + pad
    rng = np.random.default_rng(5)
    buf0 = rng.standard_normal(shift + m * ldc)
    view0 = buf0[shift:].reshape(m, ldc)
    view0[:, :n] = C0

    def run(buf):
        C = buf[shift:].view(m, ldc)
        call("vgposp_gemm", ta, tb, m, n, k, float(alpha), L._p(Ad), Ad.stride(0), L._p(Bd),
             Bd.stride(0), float(beta), C.data_ptr(), ldc, uplo, tri_a, tri_b, L._stream())

    got_buf = _both(run, buf0)
    got = got_buf[shift:].reshape(m, ldc)
    # nothing outside C is written: the doubles ahead of it and the padding of every row
    assert np.array_equal(got_buf[:shift], buf0[:shift])
    assert np.array_equal(got[:, n:], view0[:, n:])
    ref = _ref(A, B, C0, ta, tb, alpha, beta, tri_a, tri_b)
    if uplo == LOWER:
        il, iu = np.tril_indices(m), np.triu_indices(m, 1)
        assert np.array_equal(got[:, :n][iu], C0[iu], equal_nan=True)  # the strict upper triangle is not written
        assert np.isfinite(got[:, :n][il]).all()
        if numpy_check:
            np.testing.assert_allclose(got[:, :n][il], ref[il], rtol=RTOL, atol=ATOL)
    else:
        assert np.isfinite(got[:, :n]).all()
        if numpy_check:
            np.testing.assert_allclose(got[:, :n], ref, rtol=RTOL, atol=ATOL)


ALPHA_BETA = [(a, b) for a in (1.0, -1.0, 0.5) for b in (0.0, 1.0, 0.5)]


@pytest.mark.parametrize("alpha,beta", ALPHA_BETA)
@pytest.mark.parametrize("tb", [1, 0])
def test_one_tile(L, tb, alpha, beta):
    _gemm_case(L, 128, 128, 16, 0, tb, alpha, beta)


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_edge_tiles(L, ta, tb, alpha, beta):
    _gemm_case(L, 130, 254, 48, ta, tb, alpha, beta)


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0), (0.5, 0.5)])
@pytest.mark.parametrize("tb", [1, 0])
def test_lower_c(L, tb, alpha, beta):
    _gemm_case(L, 384, 384, 64, 0, tb, alpha, beta, uplo=LOWER)


@pytest.mark.parametrize("tb,tri_a,tri_b", [(0, 1, 0), (0, 0, 1), (1, 0, 1)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, 1.0)])
def test_triangular(L, tb, tri_a, tri_b, alpha, beta):
    _gemm_case(L, 256, 256, 256, 0, tb, alpha, beta, tri_a=tri_a, tri_b=tri_b)


@pytest.mark.parametrize("beta", [0.0, 0.5])
@pytest.mark.parametrize("pad,shift", [(0, 1), (1, 0), (3, 1)])
def test_unaligned_c(L, pad, shift, beta):
    """C off 16-byte alignment (base one double in, odd leading dimension): the fast kernel takes
    it as before, with 8-byte accesses."""
    _gemm_case(L, 130, 254, 48, 0, 1, -1.0, beta, pad=pad, shift=shift)
    _gemm_case(L, 256, 128, 32, 0, 0, -1.0, beta, pad=pad, shift=shift, numpy_check=False)


@pytest.mark.parametrize("tb", [1, 0])
@pytest.mark.parametrize("beta", [0.0, -2.0])
def test_splitk(L, tb, beta):
    from vgposp_amd._lib import call, query
    m, n, k, splits = 256, 256, 512, 4
    A, B, C0 = _operands(m, n, k, 0, tb, seed=21 + tb)
    if beta == 0.0:
        C0 = np.full((m, n), np.nan)
    Ad, Bd = L.as_device(A), L.as_device(B)
    nbytes = query("vgposp_gemm_splitk_workspace_bytes", m, n, k, FULL, splits)
    assert nbytes >= splits * m * n * 8  # the products really go through the partials
    ws = L.workspace(nbytes)

    def run(C):
        ws.fill_(0xFF)  # NaN partials: every partial element must be written
        call("vgposp_gemm_splitk", 0, tb, m, n, k, 0.5, L._p(Ad), Ad.stride(0), L._p(Bd),
             Bd.stride(0), float(beta), L._p(C), C.stride(0), FULL, 0, 0, splits, L._p(ws),
             ws.numel(), L._stream())

    got = _both(run, C0)
    np.testing.assert_allclose(got, _ref(A, B, C0, 0, tb, 0.5, beta), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("tb", [1, 0])
def test_splitk_lower_edge(L, tb):
    """Partials of a lower C with edge tiles (the masked partial path)."""
    from vgposp_amd._lib import call, query
    m, k, splits = 200, 256, 4
    A, B, C0 = _operands(m, m, k, 0, tb, seed=23 + tb)
    Ad, Bd = L.as_device(A), L.as_device(B)
    ws = L.workspace(query("vgposp_gemm_splitk_workspace_bytes", m, m, k, LOWER, splits))

    def run(C):
        call("vgposp_gemm_splitk", 0, tb, m, m, k, -1.0, L._p(Ad), Ad.stride(0), L._p(Bd),
             Bd.stride(0), 1.0, L._p(C), C.stride(0), LOWER, 0, 0, splits, L._p(ws),
             ws.numel(), L._stream())

    got = _both(run, C0)
    il, iu = np.tril_indices(m), np.triu_indices(m, 1)
    np.testing.assert_allclose(got[il], _ref(A, B, C0, 0, tb, -1.0, 1.0)[il], rtol=RTOL, atol=ATOL)
    assert np.array_equal(got[iu], C0[iu])


@pytest.mark.parametrize("tb", [1, 0])
def test_batched(L, tb):
    from vgposp_amd._lib import call
    nb, m, n, k, ldc = 3, 256, 128, 32, 136
    rng = np.random.default_rng(31 + tb)
    A = rng.standard_normal((nb, m, k))
    B = rng.standard_normal((nb, n, k) if tb else (nb, k, n))
    buf0 = rng.standard_normal((nb, m, ldc))
    Ad, Bd = L.as_device(A), L.as_device(B)
    ref = -A @ (B.transpose(0, 2, 1) if tb else B) + buf0[:, :, :n]

    def run(buf):  # no workspace: one launch, no split-K
        call("vgposp_gemm_batched", 0, tb, m, n, k, -1.0, L._p(Ad), Ad.stride(1), Ad.stride(0),
             L._p(Bd), Bd.stride(1), Bd.stride(0), 1.0, L._p(buf), ldc, m * ldc, FULL, 0, 0, nb,
             None, 0, L._stream())

    got = _both(run, buf0)
    np.testing.assert_allclose(got[:, :, :n], ref, rtol=RTOL, atol=ATOL)
    assert np.array_equal(got[:, :, n:], buf0[:, :, n:])


def test_grouped(L):
    """One vgposp_gemm_group launch of two problems: 256 x 256 x 64 (four tiles, K split into
    partials) and 384 x 384 x 16 lower (one K-tile, written directly; diagonal and interior
    tiles)."""
    rng = np.random.default_rng(51)
    A1, B1, C1 = (rng.standard_normal(s) for s in ((256, 64), (256, 64), (256, 256)))
    A2, B2, C2 = (rng.standard_normal(s) for s in ((384, 16), (16, 384), (384, 384)))
    ops = [L.as_device(x) for x in (A1, B1, A2, B2)]
    buf0 = np.concatenate([C1.ravel(), C2.ravel()])

    def run(buf):
        c1, c2 = buf[:256 * 256].view(256, 256), buf[256 * 256:].view(384, 384)
        L.gemm_group([dict(A=ops[0], B=ops[1], C=c1, alpha=-1.0, beta=1.0, transb=True),
                      dict(A=ops[2], B=ops[3], C=c2, alpha=0.5, beta=0.5, lower_c=True)])

    got = _both(run, buf0)
    g1, g2 = got[:256 * 256].reshape(256, 256), got[256 * 256:].reshape(384, 384)
    np.testing.assert_allclose(g1, -A1 @ B1.T + C1, rtol=RTOL, atol=ATOL)
    il, iu = np.tril_indices(384), np.triu_indices(384, 1)
    np.testing.assert_allclose(g2[il], (0.5 * A2 @ B2 + 0.5 * C2)[il], rtol=RTOL, atol=ATOL)
    assert np.array_equal(g2[iu], C2[iu])


@pytest.mark.parametrize("beta", [0.0, -2.0])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("ta,tb", [(0, 1), (0, 0), (1, 0), (1, 1)])
def test_strassen_multi_destination(L, ta, tb, levels, beta):
    """Two (one level) and four (two levels) destinations per product; a quadrant's first product
    has the caller's beta (0: C is NaN there and must not be read), the later ones beta = 1."""
    from vgposp_amd import _lib
    n = 512
    A, B, C0 = _operands(n, n, n, ta, tb, seed=41 + ta + 2 * tb + 4 * levels)
    if beta == 0.0:
        C0 = np.full((n, n), np.nan)
    Ad, Bd = L.as_device(A), L.as_device(B)
    md, lv = ctypes.c_int64(), ctypes.c_int()
    _lib.call("vgposp_potrf_strassen", ctypes.byref(md), ctypes.byref(lv))
    _lib.call("vgposp_potrf_set_strassen", 256, lv.value)
    try:
        ws = L.workspace(_lib.query("vgposp_gemm_strassen_workspace_bytes", n, n, n, levels))
        assert ws.numel() > 0  # the products really take the Strassen path

        def run(C):
            _lib.call("vgposp_gemm_strassen", ta, tb, n, n, n, 0.5, L._p(Ad), Ad.stride(0),
                      L._p(Bd), Bd.stride(0), float(beta), L._p(C), C.stride(0), levels,
                      L._p(ws), ws.numel(), L._stream())

        got = _both(run, C0)
    finally:
        _lib.call("vgposp_potrf_set_strassen", md.value, lv.value)
    # Strassen's own error is bounded in tests/test_gpu_strassen.py; here: the same tolerance
    # as the classical products holds at this size with a wide margin
    np.testing.assert_allclose(got, _ref(A, B, C0, ta, tb, 0.5, beta), rtol=RTOL, atol=ATOL)


def test_in_place_trsm_form(L):
    """C aliasing A (256 x 128 x 128 NT, beta = 0): a tile reads the rows of A that it overwrites,
    and only in its K loop."""
    from vgposp_amd._lib import call
    m, n, k = 256, 128, 128
    rng = np.random.default_rng(61)
    A, B = rng.standard_normal((m, k)), rng.standard_normal((n, k))
    Bd = L.as_device(B)

    def run(buf):
        call("vgposp_gemm", 0, 1, m, n, k, -1.0, L._p(buf), k, L._p(Bd), Bd.stride(0), 0.0,
             L._p(buf), n, FULL, 0, 0, L._stream())

    got = _both(run, A)
    np.testing.assert_allclose(got, -A @ B.T, rtol=RTOL, atol=ATOL)


def test_setter_rejects_other_values():
    from vgposp_amd import _lib
    lib = _lib.load()
    old = int(lib.vgposp_gemm_epilogue())
    assert old in (0, 1)
    assert lib.vgposp_gemm_set_epilogue(2) != 0 and lib.vgposp_gemm_set_epilogue(-1) != 0
    assert int(lib.vgposp_gemm_epilogue()) == old
