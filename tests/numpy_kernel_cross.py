"""TEST INFRASTRUCTURE: a longdouble evaluation of the four stationary kernels, the references of the
matrix-free pass (vgposp_kernel_gemv_t / _sq of csrc/criteria.hip) and the inputs of the matrix-free
rounds (the vgposp_critk_* entries, CriterionPlacement(cross_kernel=...)).  numpy only; never
imported by vgposp_amd/.

The kernels are written from the formulas of csrc/psd.h's header comment, k = amp^2 p(s) exp(-s):

    eq        exp(-r^2 / (2 ls^2))
    matern12  exp(-r / ls)
    matern32  (1 + s) exp(-s),              s = sqrt(3) r / ls
    matern52  (1 + s + s^2 / 3) exp(-s),    s = sqrt(5) r / ls

with r the Euclidean distance.  The generated matrix is R = diag(a_t) K(Xt, X) diag(a_s).
"""
import numpy as np

from tests import numpy_cross_criteria as X
from tests.numpy_criteria_greedy import LD

KINDS = ("eq", "matern12", "matern32", "matern52")
EPS = np.finfo(np.float64).eps
TAU = 1e-13            # the project's per-entry assembly tolerance (relative)


def kernel_ld(kind, Xt, Xs, amp, ls):
    """K(Xt, Xs) [P, n] in longdouble from float64 points."""
    A, B = np.asarray(Xt, dtype=LD), np.asarray(Xs, dtype=LD)
    A = A[:, None] if A.ndim == 1 else A
    B = B[:, None] if B.ndim == 1 else B
    d2 = np.zeros((A.shape[0], B.shape[0]), dtype=LD)
    for k in range(A.shape[1]):
        e = A[:, k, None] - B[None, :, k]
        d2 += e * e
    amp, ls = LD(amp), LD(ls)
    if kind == "eq":
        return amp * amp * np.exp(-d2 / (2 * ls * ls))
    r = np.sqrt(d2) / ls
    if kind == "matern12":
        return amp * amp * np.exp(-r)
    if kind == "matern32":
        s = np.sqrt(LD(3)) * r
        return amp * amp * (1 + s) * np.exp(-s)
    if kind == "matern52":
        s = np.sqrt(LD(5)) * r
        return amp * amp * (1 + s + s * s / 3) * np.exp(-s)
    raise ValueError(kind)


def cross_ld(kind, Xt, Xs, amp, ls, target_scale=None, site_scale=None):
    """R = diag(a_t) K(Xt, Xs) diag(a_s) in longdouble (None: ones)."""
    R = kernel_ld(kind, Xt, Xs, amp, ls)
    if target_scale is not None:
        R = np.asarray(target_scale, dtype=LD)[:, None] * R
    if site_scale is not None:
        R = R * np.asarray(site_scale, dtype=LD)[None, :]
    return R


def gemv_t_ld(R, x, squared=False):
    """(want, weight): R^T x (``squared``: of the squared entries) and |R|^T |x|, the weight of the
    error bound, both in longdouble."""
    M = R * R if squared else R
    x = np.asarray(x, dtype=LD)
    return M.T @ x, np.abs(M).T @ np.abs(x)


def gemv_t_bound(P, weight, squared=False):
    """|err_j| <= (4 P eps + tau) (|R|^T |x|)_j: the summation bound of a P-term sum in any order
    with one rounding per product (tests/test_gpu_gemv_t.py), plus the per-entry tolerance of a
    generated entry, doubled for its square."""
    return (4 * P * EPS + (2 * TAU if squared else TAU)) * weight


# ---- the fixtures of tests/numpy_cross_criteria.py as points ----
def fixture_points(name):
    """What ``numpy_cross_criteria.joint_cov`` builds fixture ``name`` from: (kind, Xs, Xt, amp, ls,
    a_s, a_t), so that R = a_t K(Xt, Xs) a_s."""
    from vgposp_amd.data_generation import grid_points, grid_spacing
    kind, sshape, sseed, tshape, tseed = X.FIXTURES[name]
    Xs = grid_points(sshape, jitter=0.3, seed=sseed)
    Xt = grid_points(tshape, jitter=0.3, seed=tseed)
    n = len(Xs)
    a = np.random.default_rng(sseed + 100).uniform(1.0, 1.3, n + len(Xt))
    return kind, Xs, Xt, 1.0, 2 * grid_spacing(sshape), a[:n].copy(), a[n:].copy()


# ---- a 5-D case: 3^5 sites, 4^5 jittered targets ----
D5_SEED, D5_K = 5, 6
D5_KIND, D5_AMP, D5_NOISE = "matern32", 1.2, 1e-2


def d5_case(seed=D5_SEED):
    """(Xs [243, 5], Xt [1024, 5], ls, Sigma, R): sites and targets jittered by +-0.3 of their
    spacing, Sigma = K_ss + noise I and R = K(Xt, Xs) in float64 from the longdouble kernels."""
    from vgposp_amd.data_generation import grid_points, grid_spacing
    Xs = grid_points((3,) * 5, jitter=0.3, seed=seed)
    Xt = grid_points((4,) * 5, jitter=0.3, seed=seed + 50)
    ls = 1.5 * grid_spacing((3,) * 5)
    S = kernel_ld(D5_KIND, Xs, Xs, D5_AMP, ls) + LD(D5_NOISE) * np.eye(len(Xs), dtype=LD)
    R = kernel_ld(D5_KIND, Xt, Xs, D5_AMP, ls)
    return Xs, Xt, ls, np.ascontiguousarray(S, dtype=np.float64), \
        np.ascontiguousarray(R, dtype=np.float64)


_d5 = {}


def d5_reference():
    """(case, rounds): the case and its longdouble rounds, computed once per process."""
    if not _d5:
        case = d5_case()
        _d5["v"] = (case, X.reference_run(case[3], case[4], D5_K))
    return _d5["v"]
