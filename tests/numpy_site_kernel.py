"""TEST INFRASTRUCTURE: the longdouble reference of a covariance generated from the points, the
Sigma of placement_criteria.SiteKernel and of vgposp_kernel_symv / vgposp_critg_* / vgposp_critgk_*
(csrc/criteria.hip).  numpy only; never imported by vgposp_amd/.

    Sigma_ij = a_i a_j k(X_i, X_j)            i != j     (k: tests/numpy_kernel_cross.kernel_ld)
    Sigma_ii = diag_i, or a_i^2 amp^2 when diag is None
"""
import numpy as np

from tests import numpy_criteria_greedy as C
from tests.numpy_criteria_greedy import LD
from tests.numpy_kernel_cross import EPS, TAU, kernel_ld


def site_cov_ld(kind, X, amp, ls, scale=None, diag=None):
    """Sigma [n, n] in longdouble from float64 points, scale (None: ones) and diag."""
    S = kernel_ld(kind, X, X, amp, ls)
    n = S.shape[0]
    a = np.ones(n, dtype=LD) if scale is None else np.asarray(scale, dtype=LD)
    S = S * (a[:, None] * a[None, :])       # (bit-symmetric: a_i a_j commutes)
    d = a * a * LD(amp) * LD(amp) if diag is None else np.asarray(diag, dtype=LD)
    S[np.arange(n), np.arange(n)] = d
    return S


def symv_ld(S, x, squared=False):
    """(want, weight): Sigma x (``squared``: of the squared entries) and |Sigma| |x|, the weight of
    the error bound, in longdouble."""
    M = S * S if squared else S
    x = np.asarray(x, dtype=LD)
    return M @ x, np.abs(M) @ np.abs(x)


def symv_bound(n, weight, squared=False):
    """numpy_kernel_cross.gemv_t_bound with P = n: (4 n eps + tau) (|Sigma| |x|)_i, tau doubled for
    the squared form."""
    return (4 * n * EPS + (2 * TAU if squared else TAU)) * weight


def fixture_site(name):
    """What numpy_criteria_greedy.grid_cov builds fixture F1 / F2 from, D (K + 1e-2 I) D, as a
    generated covariance: (kind, X, amp, ls, scale, diag) with scale the amplitude field and
    diag = 1.01 a^2."""
    from vgposp_amd.data_generation import grid_points, grid_spacing
    kind, shape, seed = C.FIXTURES[name]
    X = grid_points(shape, jitter=0.3, seed=seed)
    a = np.random.default_rng(seed + 100).uniform(1.0, 1.3, len(X))
    return kind, X, 1.0, 2 * grid_spacing(shape), a, 1.01 * a * a


_cov = {}


def fixture_cov(name):
    """The generated fixture in float64 (from longdouble), computed once and left unchanged."""
    if name not in _cov:
        _cov[name] = np.ascontiguousarray(site_cov_ld(*fixture_site(name)), dtype=np.float64)
        _cov[name].setflags(write=False)
    return _cov[name]
