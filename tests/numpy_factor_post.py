"""TEST INFRASTRUCTURE: the field reconstruction from placed sensors on a factored covariance
Sigma = F F^T + D, restated in float64 numpy exactly as csrc/criteria.hip's vgposp_fpost_* run it
(Sigma is never formed, Cholesky-based, the same operation order), and beside it the longdouble
reference on ``numpy_factor_cov.factor_cov_ld(F, noise)`` (n <= 1,320).  numpy only; never
imported by vgposp_amd/.

    A = sensors, sigma2 = obs_noise:  G = F_A F_A^T + diag(d_A + sigma2) = L L^T,  M = L^-1
    W = M F_A,   var_i = dg_i - |W f_i|^2,   the sensor rows with t_a = W f_a + d_a M[:, pos(a)]
    alpha = M^T (M (Y - mu_A)),  Z = F_A^T alpha,  mean_i,b = mu_i + f_i . Z[:, b],
    the sensor rows + d_a alpha[pos(a), b]
"""
import numpy as np

from tests import numpy_factor_cov as FC
from tests import numpy_factor_mi as FM
from tests.greedy_state_reference import LD, chol_lower, require_longdouble, tri_inverse

EPS = float(np.finfo(np.float64).eps)
K_SENSORS = 16
N_READINGS = 3
# (fixture of numpy_criteria_greedy, S, noise relative to the fixture's nugget)
FIXTURES = tuple((name, S, rel) for name in ("F1", "F2") for S in (75, 96, 300)
                 for rel in (1e-2, 1e-3))
OBS_NOISE_REL = (0.0, 1e-2)      # sigma2 relative to the mean diagonal of Sigma


def fixture_id(fx):
    return f"{fx[0]}-S{fx[1]}-noise{fx[2]:g}"


class FactorPost:
    """The float64 restatement.  Raises numpy.linalg.LinAlgError where the device reports
    info > 0."""

    def __init__(self, F, noise, sensors, obs_noise=0.0):
        self.F = np.ascontiguousarray(F, dtype=np.float64)
        n, S = self.F.shape
        self.d = np.zeros(n) if noise is None else np.ascontiguousarray(noise, dtype=np.float64)
        self.A = np.asarray(sensors, dtype=np.int64)
        self.k = len(self.A)
        assert len(set(self.A.tolist())) == self.k and self.d.shape == (n,)
        self.dg = np.sum(self.F * self.F, axis=1) + self.d
        self.FA = self.F[self.A]
        G = self.FA @ self.FA.T
        G[np.diag_indices(self.k)] += self.d[self.A] + obs_noise
        self.M = np.tril(np.linalg.inv(np.linalg.cholesky(G)))
        self.Wt = self.FA.T @ self.M.T                       # [S, k]

    def variance(self):
        T = self.F @ self.Wt
        var = self.dg - np.sum(T * T, axis=1)
        for p, a in enumerate(self.A):
            t = self.Wt.T @ self.F[a] + self.d[a] * self.M[:, p]
            var[a] = self.dg[a] - t @ t
        return var

    def mean(self, Y, mu=None):
        Y = np.asarray(Y, dtype=np.float64).reshape(self.k, -1)
        mu = np.zeros(len(self.F)) if mu is None else np.asarray(mu, dtype=np.float64)
        self.alpha = self.M.T @ (self.M @ (Y - mu[self.A, None]))
        Z = self.FA.T @ self.alpha
        out = mu[:, None] + self.F @ Z
        for p, a in enumerate(self.A):
            out[a] = (mu[a] + self.F[a] @ Z) + self.d[a] * self.alpha[p]
        return out


class Reference:
    """Longdouble: var [n], mean [n, B] and the mean's error scale |mu_i| + sum_j |c_ij alpha_jb|
    on the assembled Sigma (longdouble [n, n])."""

    def __init__(self, Sigma, sensors, obs_noise, Y=None, mu=None):
        A = [int(a) for a in sensors]
        k, n = len(A), Sigma.shape[0]
        G = Sigma[np.ix_(A, A)].copy()
        G[np.diag_indices(k)] += LD(obs_noise)
        M = tri_inverse(chol_lower(G))
        C = Sigma[:, A]
        T = C @ M.T
        self.dg = np.diag(Sigma).copy()
        self.var = self.dg - np.sum(T * T, axis=1)
        self.mean = self.scale = None
        if Y is not None:
            Y = np.asarray(Y, dtype=LD).reshape(k, -1)
            mu = np.zeros(n, dtype=LD) if mu is None else np.asarray(mu, dtype=LD)
            alpha = M.T @ (M @ (Y - mu[A, None]))
            self.mean = mu[:, None] + C @ alpha
            self.scale = np.abs(mu)[:, None] + np.abs(C) @ np.abs(alpha)


def errors(ref, var=None, mean=None):
    """{"var": max |dvar_i| / dg_i, "mean": max |dmean_ib| / (|mu_i| + sum_j |c_ij alpha_jb|)}, the
    denominators from the reference; only what is given."""
    out = {}
    if var is not None:
        out["var"] = float(np.max(np.abs(np.asarray(var, dtype=np.float64).astype(LD) - ref.var)
                                  / ref.dg))
    if mean is not None:
        got = np.asarray(mean, dtype=np.float64).astype(LD).reshape(ref.mean.shape)
        out["mean"] = float(np.max(np.abs(got - ref.mean) / ref.scale))
    return out


def error_floor(S, k):
    """The least error a float64 evaluation can be held to, in units of the comparison, as the
    device sums it:
        (ceil(S / 4) + ceil(k / 16) + 4 + 8) eps
    ceil(S / 4) chained accumulations on the matrix core for each of a row's numbers (one per
    K-step of four columns), ceil(k / 16) additions of squares in the lane and four more across a
    16-lane group, and eight more roundings (dg's own sum and the noise, the square, the final
    subtraction; for the mean the gathered difference, the two triangular products' last
    additions and mu).  The tolerance is 16 times the larger of this and the restatement's e_cpu,
    which on a tiny input can be exact by accident."""
    return (-(-S // 4) + -(-k // 16) + 4 + 8) * EPS


def readings(F, noise, sensors, B=N_READINGS, seed=3, mu=None):
    """B seeded sets of readings at the sensors: draws of the field itself, F z + sqrt(noise) e
    (+ mu), so that the posterior mean has something to explain."""
    rng = np.random.default_rng(seed)
    n, S = F.shape
    d = np.zeros(n) if noise is None else np.asarray(noise)
    field = F @ rng.standard_normal((S, B)) + np.sqrt(d)[:, None] * rng.standard_normal((n, B))
    if mu is not None:
        field = field + np.asarray(mu)[:, None]
    return np.ascontiguousarray(field[np.asarray(sensors)])


def prior_mean(n, seed=4):
    return np.random.default_rng(seed).uniform(1.0, 4.0, n)


def obs_noise_of(F, noise, rel):
    d = 0.0 if noise is None else np.asarray(noise)
    return rel * float(np.mean(np.sum(F * F, axis=1) + d))


def fixture_factor(fx):
    """(F, noise) of a fixture with the numpy-centred factor."""
    name, S, rel = fx
    T, noise = FC.sample_fixture(name, S, noise_rel=rel)
    return FC.factor_of(T), noise


_sigma, _picks = {}, {}


def sigma_ld(F, noise, key):
    """factor_cov_ld(F, noise), built once per process for ``key`` and left unchanged."""
    if key not in _sigma:
        require_longdouble()
        _sigma[key] = FC.factor_cov_ld(F, noise)
        _sigma[key].setflags(write=False)
    return _sigma[key]


def fixture_sensors(fx, F, noise, k=K_SENSORS):
    """The first k picks of numpy_factor_mi.reference_picks on the fixture's longdouble Sigma
    (the numpy-centred factor), once per process."""
    if (fx, k) not in _picks:
        _picks[fx, k] = FM.reference_picks(FM.reference(F, noise, fx + ("numpy",)), k)
    return list(_picks[fx, k])


# ---- edge shapes of the device kernels (numpy_factor_mi.random_factor) ----
# Each list runs against the base shape, not as the full product.  n around a 16-row block, a
# wave's 32 rows and a workgroup's 128; S around the pair, the K-tile of 32 and its multiples, and
# the largest; k around the 16-column fragment, the 64-column panel and more than two panels; B
# around a fragment and a panel, with (k, B) = (50, 14) and (50, 15) the two sides of the panel
# boundary 64 + 16.
BASE = dict(n=200, S=75, k=16, B=3)
EDGE_N = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
EDGE_S = (1, 2, 3, 4, 5, 63, 64, 65, 127, 129, 257)
EDGE_K = (1, 15, 16, 17, 63, 64, 65, 130)
EDGE_B = (0, 1, 14, 15, 64, 70)


def edge_shapes():
    """(n, S, k, B) tuples."""
    b = BASE
    out = [(n, b["S"], min(b["k"], n), b["B"]) for n in EDGE_N]
    out += [(b["n"], S, b["k"], b["B"]) for S in EDGE_S] + [(33, 4096, 16, b["B"])]
    out += [(max(b["n"], k), b["S"], k, b["B"]) for k in EDGE_K]
    out += [(b["n"], b["S"], b["k"], B) for B in EDGE_B]
    out += [(b["n"], b["S"], 50, 14), (b["n"], b["S"], 50, 15)]
    return out


def edge_case(n, S, k, B, noise=True):
    """(F, noise, sensors, Y, mu) of an edge shape: a seeded random factor, k seeded distinct
    sensors, readings drawn from the field, a prior mean."""
    F, d = FM.random_factor(n, S, 7000 + 31 * n + 7 * S + 3 * k + B)
    rng = np.random.default_rng(n + S + k + B)
    sensors = np.sort(rng.choice(n, size=k, replace=False)).astype(np.int64)
    rng.shuffle(sensors)
    d = d if noise else None
    mu = prior_mean(n)
    Y = readings(F, d, sensors, B, mu=mu) if B else None
    return F, d, sensors, Y, mu
