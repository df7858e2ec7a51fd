"""fp64 products emulated on the int8 matrix cores (vgposp_gemm_emulated, vgposp_potrf_set_emulation)
at sizes that run in seconds; the factorization reaches the path through a lowered min_dim.

* integer-valued operands give the exact product, bit for bit, in every layout and with beta, and
  the int32 accumulation holds at k = 65,536 with residue-extreme entries;
* operands that stress the scaling stay within the derived truncation bound;
* quadrants of larger matrices, and an output processed in chunks, give the same bits;
* a non-finite row is NaN and nothing else is, and the abort flag stops every write;
* the fused factor + inverse meets the classical routine's tolerance, picks like the oracle, is
  deterministic, and without the int8 library is today's Strassen result.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_gemm_emulation_host import emulation_setting
from test_gpu_strassen import _gemm, _gemm_strassen, _potrf, strassen_setting

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from vgposp_amd import _lib, linalg
    torch.cuda.set_device(0)
    assert _lib.load().vgposp_gemm_emulation_available() == 1, "libhipblaslt.so.1 did not resolve"
    return linalg


def _emul(L, ta, tb, m, n, k, alpha, A, B, beta, C):
    from vgposp_amd._lib import call, query
    ws = L.workspace(query("vgposp_gemm_emulated_workspace_bytes", m, n, k))
    call("vgposp_gemm_emulated", ta, tb, m, n, k, float(alpha), L._p(A), A.stride(0), L._p(B),
         B.stride(0), float(beta), L._p(C), C.stride(0), L._p(ws), ws.numel(), L._stream())
    torch.cuda.synchronize()


def _scale_bits(k):
    import math
    l2p = sum(math.log2(p) for p in (256, 255, 253, 251, 247, 241, 239, 233, 229, 227, 223, 217,
                                     211, 199, 197, 193))
    return min(57, math.floor((l2p - 1 - math.ceil(math.log2(k))) / 2))


@pytest.fixture(scope="module")
def int_problem():
    rng = np.random.default_rng(3)
    m, n, k = 256, 384, 512
    A = rng.integers(-2 ** 20 + 1, 2 ** 20, (m, k)).astype(np.int64)
    B = rng.integers(-2 ** 20 + 1, 2 ** 20, (k, n)).astype(np.int64)
    C0 = rng.integers(-2 ** 40, 2 ** 40, (m, n)).astype(np.int64)
    return A, B, C0, A @ B  # |sum| < 512 * 2^40 = 2^49: int64 and fp64 hold every partial sum


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0)])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_exact_products(L, int_problem, ta, tb, alpha, beta):
    A, B, C0, AB = int_problem
    m, k = A.shape
    n = B.shape[1]
    Ad = L.as_device((A.T if ta else A).astype(np.float64).copy())
    Bd = L.as_device((B.T if tb else B).astype(np.float64).copy())
    exact = (int(alpha) * AB + int(beta) * C0).astype(np.float64)
    for fn in (_emul, _gemm):  # the classical kernel is exact here too
        C = L.as_device(C0.astype(np.float64))
        fn(L, ta, tb, m, n, k, alpha, Ad, Bd, beta, C)
        np.testing.assert_array_equal(C.cpu().numpy(), exact)


def test_exact_at_k_65536_with_extreme_residues(L):
    """Entries +-127: residue +-127 for every modulus >= 255, so the int32 sums of the first two
    planes reach 127^2 * 65536 = 1.06e9 in the rows and columns that are all of one sign."""
    m = n = 128
    k = 65536
    rng = np.random.default_rng(4)
    A = 127 * rng.choice([-1, 1], (m, k)).astype(np.int64)
    B = 127 * rng.choice([-1, 1], (n, k)).astype(np.int64)
    A[:4] = 127
    B[:2] = 127
    B[2:4] = -127
    C = torch.empty((m, n), dtype=torch.float64, device="cuda")
    _emul(L, 0, 1, m, n, k, 1.0, L.as_device(A.astype(np.float64)), L.as_device(B.astype(np.float64)),
          0.0, C)
    np.testing.assert_array_equal(C.cpu().numpy(), (A @ B.T).astype(np.float64))


def test_truncation_bound_on_scaled_operands(L):
    """|C - C_ref|_ij <= 2 k 2^-s max_k|a_ik| max_k|b_kj| + 4 u |C_ref|_ij against a long-double
    product, rows of A and columns of B scaled by 2^[-40, 40], one zero row, one row of denormals.
    Below the normal range fp64 has no relative rounding term: there the final rounding is up to
    half a denormal spacing, 2^-1075, which the bound takes in addition."""
    m, n, k = 512, 512, 1024
    rng = np.random.default_rng(6)
    A = rng.standard_normal((m, k)) * 2.0 ** rng.integers(-40, 41, (m, 1))
    B = rng.standard_normal((k, n)) * 2.0 ** rng.integers(-40, 41, (1, n))
    A[7] = 0.0
    A[11] = rng.integers(-2 ** 20, 2 ** 20, k) * 2.0 ** -1074
    ref = A.astype(np.longdouble) @ B.astype(np.longdouble)
    Ad, Bd = L.as_device(A), L.as_device(B)
    out = {}
    for name, fn in (("emulated", _emul), ("classical", _gemm)):
        C = torch.full((m, n), 7.0, dtype=torch.float64, device="cuda")
        fn(L, 0, 0, m, n, k, 1.0, Ad, Bd, 0.0, C)
        out[name] = C.cpu().numpy()
    C = torch.full((m, n), 7.0, dtype=torch.float64, device="cuda")
    with strassen_setting(256, 2):
        _gemm_strassen(L, 0, 0, m, n, k, 1.0, Ad, Bd, 0.0, C, 2)
    out["strassen"] = C.cpu().numpy()
    scale = np.abs(A).max(1)[:, None].astype(np.longdouble) * np.abs(B).max(0)[None, :]
    s = _scale_bits(k)
    assert s == 57
    bound = 2 * k * np.longdouble(2.0) ** -s * scale + 4 * np.longdouble(2.0) ** -53 * np.abs(ref) \
        + np.longdouble(2.0) ** -1075
    live = scale > 2.0 ** -900  # (the figures: rows and columns in the normal range)
    for name, C in out.items():
        rel = np.abs(C.astype(np.longdouble) - ref)[live] / scale[live]
        print(f"{name}: largest |C - C_ref|_ij / (max|a_i| max|b_j|) = {float(rel.max()):.3e}")
    err = np.abs(out["emulated"].astype(np.longdouble) - ref)
    assert np.all(err <= bound), float((err / bound).max())
    assert np.all(out["emulated"][7] == 0.0)


def test_quadrants_and_chunks(L):
    from vgposp_amd import _lib
    m, n, k = 768, 512, 512
    rng = np.random.default_rng(8)
    Abig = L.as_device(rng.standard_normal((2 * m, 2 * k)))
    Bbig = L.as_device(rng.standard_normal((2 * k, 2 * n)))
    A, B = Abig[m:, k:], Bbig[:k, n:]
    Cbig0 = rng.standard_normal((2 * m, 2 * n))
    full = _lib.query("vgposp_gemm_emulated_workspace_bytes", m, n, k)
    results = []
    for cap in (0, 16 * (m + n) * k + 64 * (m * n // 4)):
        _lib.call("vgposp_gemm_emulation_set_block_cap", cap)
        try:
            if cap:
                capped = _lib.query("vgposp_gemm_emulated_workspace_bytes", m, n, k)
                assert full - capped >= 64 * (m * n - m * n // 4)  # blocks of at most a quarter
            Cbig = L.as_device(Cbig0.copy())
            _emul(L, 0, 0, m, n, k, -0.5, A, B, 2.0, Cbig[:m, n:])
        finally:
            _lib.call("vgposp_gemm_emulation_set_block_cap", 0)
        results.append(Cbig.cpu().numpy())
    np.testing.assert_array_equal(results[0], results[1])
    got = results[0]
    np.testing.assert_array_equal(got[m:], Cbig0[m:])  # nothing outside the quadrant
    np.testing.assert_array_equal(got[:m, :n], Cbig0[:m, :n])
    ref = -0.5 * (A.cpu().numpy() @ B.cpu().numpy()) + 2.0 * Cbig0[:m, n:]
    np.testing.assert_allclose(got[:m, n:], ref, rtol=0, atol=1e-12 * np.abs(ref).max())
    # the contiguous operands give the same bits as the quadrants
    C2 = L.as_device(Cbig0[:m, n:].copy())
    _emul(L, 0, 0, m, n, k, -0.5, A.contiguous(), B.contiguous(), 2.0, C2)
    np.testing.assert_array_equal(C2.cpu().numpy(), got[:m, n:])


def test_non_finite_row_and_abort_flag(L):
    from vgposp_amd import _lib
    m, n, k = 256, 256, 256
    rng = np.random.default_rng(9)
    A, B = rng.standard_normal((m, k)), rng.standard_normal((k, n))
    A[17, 100] = np.nan
    Ad, Bd = L.as_device(A), L.as_device(B)
    C = torch.zeros((m, n), dtype=torch.float64, device="cuda")
    _emul(L, 0, 0, m, n, k, 1.0, Ad, Bd, 0.0, C)
    nan = np.isnan(C.cpu().numpy())
    assert nan[17].all() and not np.delete(nan, 17, axis=0).any()
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    C.fill_(3.0)
    _lib.call("vgposp_gemm_set_abort_flag", L._p(flag))
    try:
        _emul(L, 0, 0, m, n, k, 1.0, Ad, Bd, 0.0, C)
    finally:
        _lib.call("vgposp_gemm_set_abort_flag", None)
    assert bool((C == 3.0).all())


@pytest.fixture(scope="module")
def problem2048():
    from oracle import gp as ogp
    from vgposp_amd.workloads import placement_split
    X, ls = placement_split((16, 16, 8), 0)
    S = ogp.kernel_matrix("eq", X, X, 1.0, ls)[0] + (1e-2 + 1e-6) * np.eye(len(X))
    Lref = np.linalg.cholesky(S)
    return dict(S=S, L=Lref, Linv=np.linalg.inv(Lref))


def test_factor_and_inverse(L, problem2048):
    from vgposp_amd import _lib
    S, il = problem2048["S"], np.tril_indices(2048)
    with emulation_setting(256, 16):
        for invert, ref in ((1, problem2048["Linv"]), (0, problem2048["L"])):
            A = _potrf(L, S, invert)
            Ah = A.cpu().numpy()
            np.testing.assert_allclose(Ah[il], ref[il], rtol=1e-9, atol=1e-10 * np.abs(ref).max())
            np.testing.assert_array_equal(np.triu(Ah, 1), np.triu(S, 1))
            assert torch.equal(A, _potrf(L, S, invert))  # deterministic
        Aem = _potrf(L, S, 1)
    with emulation_setting(256, 0):
        assert not torch.equal(Aem, _potrf(L, S, 1))  # the emulation did run
    # without the library the same call is today's Strassen path
    with strassen_setting(256, 2):
        with emulation_setting(256, 0):
            Astr = _potrf(L, S, 1)
        with emulation_setting(256, 16):
            _lib.call("vgposp_gemm_emulation_set_unavailable", 1)
            try:
                Aun = _potrf(L, S, 1)
            finally:
                _lib.call("vgposp_gemm_emulation_set_unavailable", 0)
    assert torch.equal(Astr, Aun)


def test_selections_equal_oracle(L, problem2048):
    from oracle import placement as op
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    S, k = problem2048["S"], 10
    Q = problem2048["Linv"].T @ problem2048["Linv"]
    deltas = []
    ref = op.placement_lazy_columns(np.diag(S).copy(), lambda y: S[y], np.diag(Q).copy(),
                                    lambda y: Q[y], k, deltas_out=deltas)
    with emulation_setting(256, 16):
        g = GreedyPlacement(S, k, copy=True).run()
        sel, dlt, _ = g.result()
    assert [int(a) for a in sel] == ref
    np.testing.assert_allclose(dlt, deltas, rtol=1e-9)
