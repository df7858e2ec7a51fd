"""TEST INFRASTRUCTURE: references for a covariance given by a factor, Sigma = F F^T + diag(noise)
(csrc/criteria.hip's SFactor, placement_criteria.FactoredCovariance).  numpy only; never imported
by vgposp_amd/.

``factor_cov_ld`` is the longdouble Sigma the rounds' reference (tests/numpy_criteria_greedy.py)
runs on.  ``fsymv_ld`` is y = Sigma x, or y_j = sum_i x_i Sigma_ij^2, in O(n S) / O(n S^2)
longdouble operations without forming Sigma, with the weight its error bound scales with.

The bounds come from the dot-product error gamma_k = k eps / (1 - k eps) of the chained sums,
doubled for the products' own roundings and the final additions:
  plain:    z = F^T x (n terms), then f_i . z (S terms)                     -> 2 (n + S) eps
  squared:  M = F^T diag(x) F (n terms, one scaling), F M (S terms), the row dot (S terms), the
            row's own square and the two diagonal terms (8 operations)      -> 2 (n + 2 S + 8) eps
each times the same expression evaluated on |F|, |x| and noise.
"""
import numpy as np

from tests import numpy_criteria_greedy as C

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

# (covariance fixture of numpy_criteria_greedy, S, noise relative to the fixture's own nugget):
# S = 75 gives odd row lengths (8-byte loads), noise 0 a singular Sigma (rank S - 1 < n)
FIXTURES = (("F1", 96, 1e-2), ("F1", 75, 0.0), ("F2", 75, 1e-2), ("F2", 96, 0.0))
CONFIGS = ("plain", "random", "oddeven")
CRITERIA = ("variance", "entropy")


def factor_of(samples, tr_stdev=1.0, dtype=np.float64):
    """F = (samples - their mean per location) / (tr_stdev sqrt(S)): F F^T is the biased empirical
    covariance, centred on the sample mean."""
    T = np.asarray(samples, dtype=dtype)
    S = T.shape[1]
    return (T - T.mean(axis=1, keepdims=True)) / (dtype(tr_stdev) * np.sqrt(dtype(S)))


def factor_cov_ld(F, noise=None):
    """Sigma = F F^T off the diagonal, f_i . f_i + noise_i on it (longdouble)."""
    F = np.asarray(F, dtype=LD)
    Sigma = F @ F.T
    if noise is not None:
        Sigma[np.diag_indices_from(Sigma)] += np.asarray(noise, dtype=LD)
    return Sigma


def fsymv_ld(F, noise, x, squared=False):
    """(want, weight), both longdouble [n]."""
    F, x = np.asarray(F, dtype=LD), np.asarray(x, dtype=LD)
    nz = np.zeros(len(x), dtype=LD) if noise is None else np.asarray(noise, dtype=LD)
    Fa, xa = np.abs(F), np.abs(x)
    if not squared:
        return F @ (F.T @ x) + nz * x, Fa @ (Fa.T @ xa) + nz * xa
    ff = np.sum(F * F, axis=1)
    dg = ff + nz
    M = F.T @ (F * x[:, None])
    Ma = Fa.T @ (Fa * xa[:, None])
    want = np.sum((F @ M) * F, axis=1) - x * ff * ff + x * dg * dg
    return want, np.sum((Fa @ Ma) * Fa, axis=1) + xa * dg * dg


def fsymv_bound(n, S, squared=False):
    """The relative factor of the bound: |got - want| <= fsymv_bound * weight."""
    return 2.0 * ((n + 2 * S + 8) if squared else (n + S)) * EPS


_samples, _ref = {}, {}


def sample_fixture(name, S, seed=21, noise_rel=0.0):
    """(samples [n, S], noise [n]): samples = chol(fixture_cov(name)) z + 3.0 with z [n, S]
    standard normal, so that the centring has a mean to remove; noise = noise_rel diag / 1.01 (the
    fixtures' diagonal is 1.01 a_i^2)."""
    key = (name, S, seed, noise_rel)
    if key not in _samples:
        Sigma = C.fixture_cov(name)
        z = np.random.default_rng(seed).standard_normal((Sigma.shape[0], S))
        T = np.linalg.cholesky(Sigma) @ z + 3.0
        noise = noise_rel * np.diag(Sigma) / 1.01
        T.setflags(write=False)
        noise.setflags(write=False)
        _samples[key] = T, noise
    return _samples[key]


def fixture_id(fx):
    return f"{fx[0]}-S{fx[1]}-{'noise' if fx[2] else 'singular'}"


def reference(F, noise, key, config, criterion, k=C.K_ROUNDS):
    """The longdouble rounds on the Sigma of (F, noise) under a configuration of
    numpy_criteria_greedy, computed once per process for ``key`` and left unchanged."""
    key = (key, config, criterion, k)
    if key not in _ref:
        name = key[0][0]
        T, cand = C.config_masks(name, config)
        _ref[key] = C.reference_run(factor_cov_ld(F, noise), criterion, k,
                                    None if criterion == "entropy" else T, cand)
    return _ref[key]
