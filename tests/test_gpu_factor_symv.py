"""GPU: y = Sigma x and y_j = sum_i x_i Sigma_ij^2 for Sigma = F F^T + diag(noise)
(vgposp_factor_symv / _sq) against the longdouble products of tests/numpy_factor_cov.py, which never
form Sigma, within the dot-product bound derived there.

n crosses the 64-row share of a wave, the 256 rows of a workgroup and several row blocks; S covers
one column, odd lengths (8-byte loads), a full and a ragged 128-column group and, with 257, more
than a lane's four column pairs.  ldf = S + 3 is a pitched view whose padding holds NaN: an odd
pitch on an even S takes the 8-byte path, an even pitch on an odd S the 16-byte path with a lone
last column."""
import ctypes

import numpy as np
import pytest

from tests import numpy_factor_cov as FC
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu

# two S per n: every S meets a single ragged block and sizes with full blocks
SHAPES = [(1, 1), (1, 257), (2, 2), (2, 75), (63, 7), (63, 64), (511, 1), (511, 64), (512, 2),
          (512, 257), (513, 7), (513, 75), (1025, 64), (1025, 257), (1537, 75), (1537, 2)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _launch(F, noise, x, squared):
    """One launch on a NaN-filled output and workspace -> y on the host."""
    import torch
    from vgposp_amd import _lib
    from vgposp_amd.linalg import _p, _stream
    n, S = F.shape
    nbytes = _lib.query("vgposp_factor_symv_workspace_bytes", n, S)
    assert nbytes % 8 == 0
    ws = torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    _lib.call("vgposp_factor_symv_sq" if squared else "vgposp_factor_symv", _p(F), n, S,
              F.stride(0), _p(noise), _p(x), _p(y), _p(ws), ctypes.c_size_t(nbytes), _stream())
    return y.cpu().numpy()


def _case(n, S, seed):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, S)) / np.sqrt(S)
    x = rng.standard_normal(n)
    x[rng.permutation(n) < n // 3] = 0.0                 # a third of x is zero (a target mask)
    noise = rng.uniform(0.0, 0.1, n)
    return F, x, noise


def _check(n, S, squared, with_noise, pitched, seed):
    import torch
    F, x, noise = _case(n, S, seed)
    base = torch.full((n, S + 3 if pitched else S), float("nan"), dtype=torch.float64,
                      device="cuda")
    Fd = base[:, :S]
    Fd.copy_(torch.as_tensor(F))
    assert Fd.stride(0) == (S + 3 if pitched else S) and Fd.stride(1) == 1
    xd = torch.as_tensor(x, device="cuda")
    nd = torch.as_tensor(noise, device="cuda") if with_noise else None
    before = base.cpu().numpy().tobytes()
    got = _launch(Fd, nd, xd, squared)
    again = _launch(Fd, nd, xd, squared)
    want, weight = FC.fsymv_ld(F, noise if with_noise else None, x, squared)
    assert np.isfinite(got).all()
    err = float(np.max(np.abs(got.astype(FC.LD) - want) / weight))
    bound = FC.fsymv_bound(n, S, squared)
    print(f"factor_symv{'_sq' if squared else ''} n={n} S={S} noise={with_noise} "
          f"pitched={pitched}: {err:.2e} of the weight (bound {bound:.2e})")
    assert err <= bound
    assert got.tobytes() == again.tobytes()                      # two launches are bit-identical
    assert base.cpu().numpy().tobytes() == before                # F is only read
    return got


@pytest.mark.parametrize("squared", [False, True], ids=["plain", "squared"])
@pytest.mark.parametrize("n,S", SHAPES, ids=[f"n{n}-S{S}" for n, S in SHAPES])
def test_against_longdouble(n, S, squared):
    require_longdouble()
    for with_noise in (False, True):
        for pitched in (False, True):
            _check(n, S, squared, with_noise, pitched, seed=1000 * n + S)


@pytest.mark.parametrize("squared,S", [(False, 96), (True, 33)], ids=["plain-S96", "squared-S33"])
def test_large(squared, S):
    """n = 65,537: 513 row blocks of 128 rows with a last block of one row, five chunks of the
    squared pass with an odd last one; every row is checked."""
    require_longdouble()
    _check(65537, S, squared, True, False, seed=7)


def test_host_wrapper():
    """covariance.factor_symv: a host F, a pitched device view, noise given or not."""
    import torch
    from vgposp_amd.covariance import factor_symv
    F, x, noise = _case(300, 40, 5)
    for squared in (False, True):
        want, weight = FC.fsymv_ld(F, noise, x, squared)
        got = factor_symv(F, x, noise=noise, squared=squared).cpu().numpy()
        assert np.max(np.abs(got - want) / weight) <= FC.fsymv_bound(300, 40, squared)
        base = torch.zeros((300, 44), dtype=torch.float64, device="cuda")
        base[:, :40] = torch.as_tensor(F)
        out = torch.empty(300, dtype=torch.float64, device="cuda")
        assert factor_symv(base[:, :40], x, squared=squared, out=out) is out
        want0, weight0 = FC.fsymv_ld(F, None, x, squared)
        assert np.max(np.abs(out.cpu().numpy() - want0) / weight0) \
            <= FC.fsymv_bound(300, 40, squared)
    with pytest.raises(ValueError, match="shapes do not match"):
        factor_symv(F, x[:-1])
    with pytest.raises(ValueError, match="shapes do not match"):
        factor_symv(F, x, noise=noise[:-1])
