"""GPU: a factorization in the compact Cholesky workspace equals the one in the full workspace bit
for bit (the smaller partials area still holds every split the recursion takes), for orders on
both sides of the 128 / 512 block sizes, odd orders, and with and without the inverse."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("n", [129, 151, 256, 513, 640, 1000])
def test_compact_workspace_factor_is_bit_identical(n, invert):
    import torch
    torch.cuda.set_device(0)
    from vgposp_amd import linalg
    rng = np.random.default_rng(n)
    X = rng.uniform(-2, 2, (n, 3))
    K = linalg.kernel_matrix("eq", X, None, 1.0, 0.4, diag_shift=0.05)[0]
    A, B = K.clone(), K.clone()
    _, da, ia = linalg.cholesky_(A, invert=invert)
    _, db, ib = linalg.cholesky_(B, invert=invert, compact_ws=True)
    assert int(ia[0]) == 0 and int(ib[0]) == 0
    assert torch.equal(A, B)
    assert torch.equal(da, db)
    L = np.tril(A.cpu().numpy())
    ref = np.linalg.cholesky(K.cpu().numpy())
    ref = np.linalg.inv(ref) if invert else ref
    np.testing.assert_allclose(L, ref, rtol=1e-8, atol=1e-10 * np.abs(ref).max())
