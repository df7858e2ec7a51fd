"""Strassen for the large plain products of the fused Cholesky + inverse (vgposp_gemm_strassen,
vgposp_potrf_set_strassen), at sizes small enough to run in seconds: min_dim 256 / 512 sends
512..2048 problems down every branch the N = 65,536 step takes at min_dim 8192.

* integer-valued operands: one and two levels are EXACT for every layout, alpha / beta, padded
  leading dimensions, and touch nothing outside C;
* ineligible shapes and levels = 0 are the classical launch, bit for bit;
* real operands stay within Higham's bound for Strassen over classical blocks;
* the fused factor + inverse with the split SYRK / TRMMs meets the tolerance of the classical
  routine's own test, deterministically, and the greedy picks equal the oracle's;
* a failed pivot still stops the recursion (the add kernel and the multi-destination launches read
  the abort flag) and reports its column.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from vgposp_amd import linalg
    torch.cuda.set_device(0)
    return linalg


class strassen_setting:
    """vgposp_potrf_set_strassen(min_dim, levels) for a with-block; restores the previous one."""

    def __init__(self, min_dim, levels):
        self.new = (min_dim, levels)

    def __enter__(self):
        from vgposp_amd import _lib
        md, lv = ctypes.c_int64(), ctypes.c_int()
        _lib.call("vgposp_potrf_strassen", ctypes.byref(md), ctypes.byref(lv))
        self.old = (md.value, lv.value)
        _lib.call("vgposp_potrf_set_strassen", *self.new)
        return self

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_potrf_set_strassen", *self.old)
        return False


def _gemm_strassen(L, ta, tb, m, n, k, alpha, A, B, beta, C, levels):
    from vgposp_amd._lib import call, query
    ws = L.workspace(query("vgposp_gemm_strassen_workspace_bytes", m, n, k, levels))
    call("vgposp_gemm_strassen", ta, tb, m, n, k, float(alpha), L._p(A), A.stride(0), L._p(B),
         B.stride(0), float(beta), L._p(C), C.stride(0), levels, L._p(ws), ws.numel(), L._stream())


def _gemm(L, ta, tb, m, n, k, alpha, A, B, beta, C):
    from vgposp_amd._lib import call
    call("vgposp_gemm", ta, tb, m, n, k, float(alpha), L._p(A), A.stride(0), L._p(B), B.stride(0),
         float(beta), L._p(C), C.stride(0), 0, 0, 0, L._stream())


PAD = 256


def _padded(host):
    """A device view of `host` inside a buffer 256 columns wider (the rest filled with 77)."""
    r, c = host.shape
    buf = torch.full((r, c + PAD), 77.0, dtype=torch.float64, device="cuda")
    buf[:, :c] = torch.as_tensor(host, dtype=torch.float64)
    return buf, buf[:, :c]


@pytest.fixture(scope="module")
def int_operands():
    """Integer operands and their int64 products, computed once per shape and layout."""
    cache = {}

    def get(m, n, k, ta, tb):
        key = (m, n, k, ta, tb)
        if key not in cache:
            rng = np.random.default_rng(m + 3 * n + 7 * k + 11 * ta + 13 * tb)
            A = rng.integers(-4, 5, (k, m) if ta else (m, k))
            B = rng.integers(-4, 5, (n, k) if tb else (k, n))
            C0 = rng.integers(-4, 5, (m, n))
            # |entries| <= 16 k < 2^53: the float64 BLAS product is the exact integer product
            P = ((A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64))
            P = P.astype(np.int64)
            cache[key] = (A, B, C0, P)
        return cache[key]

    return get


@pytest.mark.parametrize("alpha,beta", [(1, 0), (-1, 1), (2, -1)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("levels", [1, 2])
@pytest.mark.parametrize("m,n,k", [(512, 512, 512), (768, 512, 1024), (1024, 1024, 512)])
def test_exact_products(L, int_operands, m, n, k, levels, ta, tb, alpha, beta):
    A, B, C0, P = int_operands(m, n, k, ta, tb)
    ref = alpha * P + beta * C0.astype(np.int64)
    Abuf, Ad = _padded(A.astype(np.float64))
    Bbuf, Bd = _padded(B.astype(np.float64))
    Cinit = np.full((m, n), np.nan) if beta == 0 else C0.astype(np.float64)
    Cbuf, Cd = _padded(Cinit)
    with strassen_setting(256, levels):
        _gemm_strassen(L, ta, tb, m, n, k, alpha, Ad, Bd, beta, Cd, levels)
    assert torch.equal(Cd.cpu(), torch.as_tensor(ref, dtype=torch.float64))
    for buf, host in ((Abuf, A), (Bbuf, B)):
        assert torch.equal(buf[:, :host.shape[1]].cpu(), torch.as_tensor(host, dtype=torch.float64))
    for buf in (Abuf, Bbuf, Cbuf):
        assert bool((buf[:, -PAD:] == 77.0).all())  # the neighbouring columns are untouched


@pytest.mark.parametrize("m,n,k,min_dim,levels", [(640, 512, 512, 256, 2), (512, 512, 384, 512, 2),
                                                  (512, 512, 512, 256, 0)])
def test_ineligible_is_the_classical_kernel(L, m, n, k, min_dim, levels):
    rng = np.random.default_rng(m + k + levels)
    A = L.as_device(rng.standard_normal((m, k)))
    B = L.as_device(rng.standard_normal((n, k)))
    C0 = rng.standard_normal((m, n))
    C1, C2 = L.as_device(C0.copy()), L.as_device(C0.copy())
    with strassen_setting(min_dim, max(levels, 1)):
        _gemm_strassen(L, 0, 1, m, n, k, -1.5, A, B, 0.5, C1, levels)
    _gemm(L, 0, 1, m, n, k, -1.5, A, B, 0.5, C2)
    assert torch.equal(C1, C2)


def test_real_error_within_higham_bound(L):
    """Standard-normal 1024^3, two levels over classical 256-blocks: the max-norm error against a
    long-double product is within 12^L (n0^2 + 5 n0) u max|A| max|B| (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., Theorem 23.2), L = 2, n0 = 256, u = 2^-53."""
    n, lv = 1024, 2
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    ref = (A.astype(np.longdouble) @ B.astype(np.longdouble))
    Ad, Bd = L.as_device(A), L.as_device(B)
    Cs = torch.empty((n, n), dtype=torch.float64, device="cuda")
    Cc = torch.empty_like(Cs)
    with strassen_setting(256, lv):
        _gemm_strassen(L, 0, 0, n, n, n, 1.0, Ad, Bd, 0.0, Cs, lv)
    _gemm(L, 0, 0, n, n, n, 1.0, Ad, Bd, 0.0, Cc)
    err_s = float(np.abs(Cs.cpu().numpy().astype(np.longdouble) - ref).max())
    err_c = float(np.abs(Cc.cpu().numpy().astype(np.longdouble) - ref).max())
    n0 = n // 2 ** lv
    bound = 12.0 ** lv * (n0 * n0 + 5 * n0) * 2.0 ** -53 * np.abs(A).max() * np.abs(B).max()
    print(f"strassen max error {err_s:.3e}, classical {err_c:.3e}, ratio {err_s / err_c:.2f}, "
          f"bound {bound:.3e}")
    assert err_s <= bound
    assert err_s > 0.0 and not torch.equal(Cs, Cc)  # the Strassen path did run


@pytest.fixture(scope="module")
def problem2048():
    """The bench's covariance on placement_split((16, 16, 8), 0), its Cholesky factor and inverse."""
    from oracle import gp as ogp
    from vgposp_amd.workloads import placement_split
    X, ls = placement_split((16, 16, 8), 0)
    S = ogp.kernel_matrix("eq", X, X, 1.0, ls)[0] + (1e-2 + 1e-6) * np.eye(len(X))
    Lref = np.linalg.cholesky(S)
    return dict(S=S, L=Lref, Linv=np.linalg.inv(Lref))


def _potrf(L, S, invert):
    from vgposp_amd._lib import call, query
    n = S.shape[0]
    A = L.as_device(S.copy())
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = L.workspace(query("vgposp_potrf_workspace_bytes", n))
    call("vgposp_potrf_lower", L._p(A), n, A.stride(0), 0, 1, int(invert), None, L._p(info),
         L._p(ws), ws.numel(), L._stream())
    assert int(info.item()) == 0
    return A


@pytest.mark.parametrize("min_dim", [512, 256])
def test_factor_and_inverse(L, problem2048, min_dim):
    S, il = problem2048["S"], np.tril_indices(2048)
    with strassen_setting(min_dim, 2):
        for invert, ref in ((1, problem2048["Linv"]), (0, problem2048["L"])):
            A = _potrf(L, S, invert)
            Ah = A.cpu().numpy()
            np.testing.assert_allclose(Ah[il], ref[il], rtol=1e-9, atol=1e-10 * np.abs(ref).max())
            np.testing.assert_array_equal(np.triu(Ah, 1), np.triu(S, 1))
            assert torch.equal(A, _potrf(L, S, invert))  # deterministic
        Astr = _potrf(L, S, 1)
    with strassen_setting(min_dim, 0):
        assert not torch.equal(Astr, _potrf(L, S, 1))  # the Strassen path did run


def test_selections_equal_oracle(L, problem2048):
    from oracle import placement as op
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    S, k = problem2048["S"], 10
    Q = problem2048["Linv"].T @ problem2048["Linv"]
    deltas, margins = [], []
    ref = op.placement_lazy_columns(np.diag(S).copy(), lambda y: S[y], np.diag(Q).copy(),
                                    lambda y: Q[y], k, deltas_out=deltas, margins_out=margins)
    assert ref == op.placement_lazy_incremental(S, k)
    assert ref == [1084, 540, 596, 1251, 1708, 1172, 1755, 314, 362, 1473]
    rel = min(m / abs(d) for m, d in zip(margins, deltas))
    print(f"smallest top-two margin {rel:.3e} relative")
    assert rel > 1e-8  # only a real error flips a pick
    with strassen_setting(256, 2):
        g = GreedyPlacement(S, k, copy=True).run()
        sel, dlt, _ = g.result()
    assert [int(a) for a in sel] == ref
    np.testing.assert_allclose(dlt, deltas, rtol=1e-9)


def test_early_abort(L, problem2048):
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    S = problem2048["S"].copy()
    col = 1500  # in the trailing half: the leading half's products have run by then
    S[col, col] = -1.0
    with strassen_setting(256, 2):
        g = GreedyPlacement(S, 4, copy=True).init()
        torch.cuda.synchronize()
        assert int(g.info.item()) == col + 1


def test_workspace_too_small(L):
    from vgposp_amd import _lib
    with strassen_setting(512, 0):
        base = _lib.query("vgposp_potrf_workspace_bytes", 2048)
    with strassen_setting(512, 1):
        A = torch.zeros((1024, 1024), dtype=torch.float64, device="cuda")
        C = torch.zeros_like(A)
        ws = L.workspace(base)  # enough for the classical layout, not for the operand temporaries
        assert _lib.query("vgposp_gemm_strassen_workspace_bytes", 1024, 1024, 1024, 1) > 1024
        rc = _lib.load().vgposp_gemm_strassen(0, 0, 1024, 1024, 1024, 1.0, L._p(A), 1024, L._p(A),
                                              1024, 0.0, L._p(C), 1024, 1, L._p(ws), 1024,
                                              L._stream())
        assert rc == _lib.E_WS
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert _lib.query("vgposp_potrf_workspace_bytes", 2048) > base
        S = torch.zeros((2048, 2048), dtype=torch.float64, device="cuda")
        rc = _lib.load().vgposp_potrf_lower(L._p(S), 2048, 2048, 0, 1, 1, None, L._p(info),
                                            L._p(ws), ws.numel(), L._stream())
        assert rc == _lib.E_WS
