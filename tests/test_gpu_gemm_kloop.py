"""The hand-scheduled K loop of the fast GEMM kernels (vgposp_gemm_set_kloop) against the
compiler-scheduled one: every product is run with kloop 0 and kloop 1 on the same operands and
must be bit-identical, and the kloop-1 result must match a NumPy fp64 product at the tolerance of
tests/test_gpu_linalg.py's GEMM tests.

The shapes are the smallest at which the hand-scheduled path can go wrong.  It takes pairs of
K-tiles (16 deep) that need no mask and have a successor, so m = n = 128 with k = 16 .. 96 gives
runs of 0, 0, 2, 2, 4 and 4 tiles, k = 200 a run that stops ahead of the partial last tile;
200 x 136 has clamped rows in both operands; 384^3 with a triangular operand has interior tiles
before or after the eight that straddle the diagonal; split-K starts every split at a non-zero k;
the Strassen products go through the multi-destination kernels.  TN and TT are not ported and
must not change.
"""
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


class kloop_setting:
    """vgposp_gemm_set_kloop(v) for a with-block; restores the previous setting."""

    def __init__(self, v):
        self.new = v

    def __enter__(self):
        from vgposp_amd import _lib
        self.old = int(_lib.load().vgposp_gemm_kloop())
        _lib.call("vgposp_gemm_set_kloop", self.new)
        return self

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_gemm_set_kloop", self.old)
        return False


def _operands(m, n, k, ta, tb, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((k, m) if ta else (m, k))
    B = rng.standard_normal((n, k) if tb else (k, n))
    C0 = rng.standard_normal((m, n))
    return A, B, C0


def _both(run, C0):
    """run(C) under kloop 0 and kloop 1 on copies of C0; returns the two results (host)."""
    out = []
    for v in (0, 1):
        C = torch.as_tensor(C0, dtype=torch.float64).cuda()
        with kloop_setting(v):
            run(C)
            torch.cuda.synchronize()
        out.append(C.cpu())
    return out


def _check(run, C0, ref, lower=False):
    c0, c1 = _both(run, C0)
    assert torch.equal(c0, c1), "kloop 1 differs from kloop 0"
    got = c1.numpy()
    if lower:
        il = np.tril_indices(ref.shape[0])
        np.testing.assert_allclose(got[il], ref[il], rtol=RTOL, atol=ATOL)
        iu = np.triu_indices(ref.shape[0], 1)
        assert np.array_equal(got[iu], C0[iu])  # the strict upper triangle is not written
    else:
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL)


def _gemm_case(L, m, n, k, ta, tb, alpha, beta, tri_a=0, tri_b=0, uplo=FULL):
    from vgposp_amd._lib import call
    A, B, C0 = _operands(m, n, k, ta, tb, seed=m + 7 * n + 13 * k + ta + 2 * tb + 4 * tri_a + 8 * tri_b)
    Ad, Bd = L.as_device(A), L.as_device(B)
    opA = (np.tril(A) if tri_a else A)
    opB = (np.tril(B) if tri_b else B)
    opA = opA.T if ta else opA
    opB = opB.T if tb else opB
    ref = alpha * opA @ opB + beta * C0

    def run(C):
        call("vgposp_gemm", ta, tb, m, n, k, float(alpha), L._p(Ad), Ad.stride(0), L._p(Bd),
             Bd.stride(0), float(beta), L._p(C), C.stride(0), uplo, tri_a, tri_b, L._stream())

    _check(run, C0, ref, lower=uplo == LOWER)


AB = [(1.0, 0.0), (-1.0, 1.0), (0.5, -2.0)]


@pytest.mark.parametrize("tb", [1, 0])
@pytest.mark.parametrize("k", [16, 32, 48, 64, 80, 96, 200])
def test_tile_counts(L, k, tb):
    alpha, beta = AB[(k // 16) % 3]
    _gemm_case(L, 128, 128, k, 0, tb, alpha, beta)


@pytest.mark.parametrize("alpha,beta", AB)
@pytest.mark.parametrize("tb", [1, 0])
def test_clamped_rows(L, tb, alpha, beta):
    _gemm_case(L, 200, 136, 96, 0, tb, alpha, beta)


@pytest.mark.parametrize("ta,tb", [(1, 0), (1, 1)])
def test_unported_layouts(L, ta, tb):
    _gemm_case(L, 256, 256, 96, ta, tb, -1.0, 1.0)


@pytest.mark.parametrize("tb,tri_a,tri_b", [(0, 1, 0), (0, 0, 1), (1, 0, 1)])
@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (0.5, -2.0)])
def test_triangular(L, tb, tri_a, tri_b, alpha, beta):
    _gemm_case(L, 384, 384, 384, 0, tb, alpha, beta, tri_a=tri_a, tri_b=tri_b)


@pytest.mark.parametrize("tb", [1, 0])
def test_lower_c(L, tb):
    _gemm_case(L, 384, 384, 96, 0, tb, -1.0, 1.0, uplo=LOWER)


@pytest.mark.parametrize("tb", [1, 0])
def test_splitk(L, tb):
    from vgposp_amd._lib import call, query
    m, n, k, splits = 256, 256, 512, 4
    A, B, C0 = _operands(m, n, k, 0, tb, seed=21 + tb)
    Ad, Bd = L.as_device(A), L.as_device(B)
    ws = L.workspace(query("vgposp_gemm_splitk_workspace_bytes", m, n, k, FULL, splits))

    def run(C):
        call("vgposp_gemm_splitk", 0, tb, m, n, k, 0.5, L._p(Ad), Ad.stride(0), L._p(Bd),
             Bd.stride(0), -2.0, L._p(C), C.stride(0), FULL, 0, 0, splits, L._p(ws), ws.numel(),
             L._stream())

    _check(run, C0, 0.5 * A @ (B.T if tb else B) - 2.0 * C0)


@pytest.mark.parametrize("tb", [1, 0])
def test_batched(L, tb):
    from vgposp_amd._lib import call
    nb, m, n, k = 3, 256, 128, 80
    rng = np.random.default_rng(31 + tb)
    A = rng.standard_normal((nb, m, k))
    B = rng.standard_normal((nb, n, k) if tb else (nb, k, n))
    C0 = rng.standard_normal((nb, m, n))
    Ad, Bd = L.as_device(A), L.as_device(B)
    ref = -A @ (B.transpose(0, 2, 1) if tb else B) + C0

    def run(C):  # no workspace: one launch, no split-K
        call("vgposp_gemm_batched", 0, tb, m, n, k, -1.0, L._p(Ad), Ad.stride(1), Ad.stride(0),
             L._p(Bd), Bd.stride(1), Bd.stride(0), 1.0, L._p(C), C.stride(1), C.stride(0), FULL,
             0, 0, nb, None, 0, L._stream())

    _check(run, C0, ref)


@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("tb", [0, 1])
def test_strassen_multi_destination(L, tb, levels):
    import ctypes
    from vgposp_amd import _lib
    n = 512
    A, B, C0 = _operands(n, n, n, 0, tb, seed=41 + tb + 2 * levels)
    Ad, Bd = L.as_device(A), L.as_device(B)
    md, lv = ctypes.c_int64(), ctypes.c_int()
    _lib.call("vgposp_potrf_strassen", ctypes.byref(md), ctypes.byref(lv))
    _lib.call("vgposp_potrf_set_strassen", 256, lv.value)
    try:
        ws = L.workspace(_lib.query("vgposp_gemm_strassen_workspace_bytes", n, n, n, levels))
        assert ws.numel() > 0  # the products really take the Strassen path

        def run(C):
            _lib.call("vgposp_gemm_strassen", 0, tb, n, n, n, 0.5, L._p(Ad), Ad.stride(0),
                      L._p(Bd), Bd.stride(0), -2.0, L._p(C), C.stride(0), levels, L._p(ws),
                      ws.numel(), L._stream())

        c0, c1 = _both(run, C0)
    finally:
        _lib.call("vgposp_potrf_set_strassen", md.value, lv.value)
    assert torch.equal(c0, c1), "kloop 1 differs from kloop 0"
    # Strassen's own error is bounded in tests/test_gpu_strassen.py; here: the same tolerance
    # as the classical products holds at this size with a wide margin
    np.testing.assert_allclose(c1.numpy(), 0.5 * A @ (B.T if tb else B) - 2.0 * C0, rtol=RTOL,
                               atol=ATOL)
