"""TEST INFRASTRUCTURE: the mutual-information rounds on a factored covariance Sigma = F F^T + D,
D = diag(noise) > 0, restated in float64 numpy exactly as csrc/criteria.hip's vgposp_fmi_* run
them (Woodbury; Sigma is never formed), and the comparison of a round's state with the longdouble
reference ``greedy_state_reference.LongdoubleGreedy`` on ``numpy_factor_cov.factor_cov_ld``.
numpy only; never imported by vgposp_amd/.

    C = I + F^T D^-1 F = L L^T,  M = L^-1,  C^-1 = M^T M
    prec_y = Q_yy = 1 / d_y - |M f_y|^2 / d_y^2,   nom_y = dg_y = f_y . f_y + d_y
    a round, for its pick a:   s_i = f_i . f_a (dg_a at i = a),
                               q_i = [i = a] / d_a - (f_i . u_a) / d_i,  u_a = C^-1 f_a / d_a,
    both downdated by the earlier rows of W and V through the pick's pivots,
    w = s / sqrt(nom_a), v = q / sqrt(prec_a), nom -= w^2, prec -= v^2,
    delta = nom / (1 / prec), 0 where |nom| or |1 / prec| < thr.
Selection is the full greedy: the arg-max of the fresh deltas over the free candidates, ties to the
lower index.  A round scores and selects first and then updates for its pick, so after round r
``delta`` is conditioned on picks[:r] and nom, prec, W, V on picks[:r + 1].
"""
import numpy as np

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_cov as FC
from tests.greedy_state_reference import LD, LongdoubleGreedy, require_longdouble

THRESHOLD = 1e-8
ROUNDS = 16
# (fixture of numpy_criteria_greedy, S, noise relative to the fixture's nugget): D > 0 everywhere
FIXTURES = (("F1", 96, 1e-2), ("F2", 75, 1e-2), ("F2", 300, 1e-3))
CONFIGS = ("plain", "random", "oddeven")
MIN_DISTANCE = 1e-6          # of |nom| and |den| from the zeroing threshold
ERROR_KEYS = ("delta", "nom", "prec", "W", "V")


def fixture_id(fx):
    return f"{fx[0]}-S{fx[1]}-noise{fx[2]:g}"


class FactorMI:
    """The float64 rounds.  ``state`` after ``round(a)``: delta as scored before the pick."""

    def __init__(self, F, noise, thr=THRESHOLD, candidates=None):
        self.F = np.ascontiguousarray(F, dtype=np.float64)
        self.d = np.ascontiguousarray(noise, dtype=np.float64)
        n, S = self.F.shape
        assert self.d.shape == (n,) and (self.d > 0).all()
        self.n, self.thr = n, thr
        self.dg = np.sum(self.F * self.F, axis=1) + self.d
        Cm = np.eye(S) + self.F.T @ (self.F / self.d[:, None])
        M = np.linalg.inv(np.linalg.cholesky(Cm))
        self.M = np.tril(M)
        self.Cinv = self.M.T @ self.M
        T = self.F @ self.M.T
        self.nom = self.dg.copy()
        self.prec = 1.0 / self.d - np.sum(T * T, axis=1) / (self.d * self.d)
        self.qdiag = self.prec.copy()
        self.blocked = ~C.as_mask(n, candidates)
        self.W, self.V, self.picks = [], [], []
        self.delta = np.zeros(n)

    def sigma_col(self, a):
        s = self.F @ self.F[a]
        s[a] = self.dg[a]
        return s

    def q_col(self, a):
        u = self.Cinv @ self.F[a] / self.d[a]
        q = -(self.F @ u) / self.d
        q[a] += 1.0 / self.d[a]
        return q

    def score(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            den = 1.0 / self.prec
            return np.where((np.abs(den) < self.thr) | (np.abs(self.nom) < self.thr), 0.0,
                            self.nom / den)

    def round(self, forced=None):
        """One round: score, select (``forced``: that location) and update.  Returns the pick, or
        -1 when no candidate is left (nothing changes then)."""
        self.delta = self.score()
        if forced is None:
            free = ~self.blocked
            if not free.any():
                self.picks.append(-1)
                return -1
            a = C.argmax_low(self.delta, free)
        else:
            a = int(forced)
        self.blocked[a] = True
        noma, preca = self.nom[a], self.prec[a]
        s, q = self.sigma_col(a), self.q_col(a)
        for w, v in zip(self.W, self.V):
            s -= w[a] * w
            q -= v[a] * v
        w = s / np.sqrt(noma) if noma >= self.thr and noma > 0.0 else np.zeros(self.n)
        v = q / np.sqrt(preca) if preca > 0.0 else np.zeros(self.n)
        self.W.append(w)
        self.V.append(v)
        self.nom = self.nom - w * w
        self.prec = self.prec - v * v
        self.picks.append(a)
        return a

    def state(self):
        return {"delta": self.delta, "nom": self.nom, "prec": self.prec,
                "W": np.array(self.W).reshape(len(self.W), self.n),
                "V": np.array(self.V).reshape(len(self.V), self.n)}


def state_errors(ref, picks, r, st, candidates=None):
    """Errors of the state ``st`` after round r of a run whose picks were picks[:r + 1], against
    the LongdoubleGreedy ``ref``: delta relative over every location outside picks[:r] (blocked
    ones included); nom and prec relative over every location outside picks[:r + 1]; the rows of W
    and V normwise (|error| / max |row|).  Also the relative gap between the best and the
    second-best delta over the free candidates, the reference's arg-max (ties to the lower index)
    and the smallest |nom| and |den| of the compared deltas."""
    n = ref.N
    A = [int(a) for a in picks[:r + 1]]
    before, after = ref.state(A[:r], n), ref.state(A, n)
    use = ~before.sel
    free = use & C.as_mask(n, candidates)
    f64 = lambda x: np.asarray(x, dtype=np.float64).astype(LD)
    out = {"delta": float(np.max(np.abs(f64(st["delta"])[use] - before.delta[use])
                                 / np.abs(before.delta[use]))),
           "min_nom": float(np.min(np.abs(before.nom[use]))),
           "min_den": float(np.min(np.abs(before.den[use])))}
    d = np.where(free, before.delta, -np.inf).astype(np.float64)
    out["argmax"] = int(np.argmax(d))
    top = np.sort(np.unique(d[free]))[::-1]
    out["gap"] = float((top[0] - top[1]) / abs(top[0])) if len(top) > 1 else np.inf
    keep = ~after.sel
    for key, want in (("nom", after.nom), ("prec", after.prec)):
        out[key] = float(np.max(np.abs(f64(st[key])[keep] - want[keep]) / np.abs(want[keep]))) \
            if keep.any() else 0.0
    for key, want in (("W", after.W), ("V", after.V)):
        got = f64(st[key])
        assert got.shape == want.shape, (key, got.shape, want.shape)
        out[key] = float(np.max(np.max(np.abs(got - want), axis=1) / np.max(np.abs(want), axis=1)))
    return out


def worst(errs):
    return max(e[k] for e in errs for k in ERROR_KEYS)


def forced_run_errors(ref, F, noise, picks, candidates=None, first=0):
    """state_errors of the float64 restatement driven through ``picks`` (forced), for the rounds
    first .. len(picks) - 1: the e_cpu the device's tolerance is taken from."""
    g = FactorMI(F, noise, candidates=candidates)
    errs = []
    for r, a in enumerate(picks):
        g.round(forced=a)
        if r >= first:
            errs.append(state_errors(ref, picks, r, g.state(), candidates))
    return errs


def reference_picks(ref, k, candidates=None, placed=()):
    """k picks of the full greedy on the longdouble deltas after ``placed`` (ties to the lower
    index)."""
    n = ref.N
    A = [int(a) for a in placed]
    free = C.as_mask(n, candidates).copy()
    free[A] = False
    for _ in range(k):
        d = ref.state(A, n, THRESHOLD).delta.astype(np.float64)
        y = C.argmax_low(d, free)
        A.append(y)
        free[y] = False
    return A[len(placed):]


_ref = {}


def reference(F, noise, key):
    """LongdoubleGreedy of Sigma = F F^T + diag(noise), built once per process for ``key``."""
    if key not in _ref:
        require_longdouble()
        _ref[key] = LongdoubleGreedy(FC.factor_cov_ld(F, noise))
    return _ref[key]


def fixture_factor(fx):
    """(F, noise) of a fixture with the numpy-centred factor."""
    name, S, rel = fx
    T, noise = FC.sample_fixture(name, S, noise_rel=rel)
    return FC.factor_of(T), noise


# Edge shapes of the device kernels: S around the 128-column step of a wave and the 64 of the u_a
# rows, odd S (8-byte loads, the lone last column), n around a wave's 64 rows and a workgroup's
# 256, S > n; and S = 4,096, where f_a and u_a together no longer fit the LDS a workgroup is given
# by default.  Seeds for which every round's gap holds (tests/test_factor_mi_reference.py).
EDGE_S = (1, 2, 75, 127, 128, 129, 300)
EDGE_N = (1, 63, 64, 65, 255, 257)
EDGE_SHAPES = tuple((n, S) for S in EDGE_S for n in EDGE_N) + ((200, 4096),)
EDGE_SEEDS = {(64, 1): 1155, (65, 1): 1086, (255, 1): 1542, (257, 1): 1474, (255, 2): 2262,
              (257, 128): 128264, (257, 300): 300271}   # the others: 1000 S + n
EPS = float(np.finfo(np.float64).eps)


def edge_seed(n, S):
    return EDGE_SEEDS.get((n, S), 1000 * S + n)


def edge_rounds(n):
    return min(ROUNDS, n)


def edge_error_floor(S, rounds):
    """The least error a float64 evaluation of a round's quantities can be held to, in units of
    the comparison: a dot product of length S as the device sums it (S / 64 chained terms per lane,
    then six butterfly additions), two downdate terms per earlier round, and eight more roundings
    (the division by d, the square root, the quotient, the square, the subtraction, 1 / prec,
    nom / den, the diagonal's own sum).  The edge shapes take their tolerance from the larger of
    this and the restatement's e_cpu, which on a tiny input can be exact by accident."""
    return (-(-S // 64) + 6 + 2 * rounds + 8) * EPS


def random_factor(n, S, seed, noise_rel=0.3):
    """A seeded random F [n, S] (rows scaled by a field in [0.5, 1.5]) with noise between
    noise_rel and 2 noise_rel of diag(F F^T), not proportional to it: with S = 1 a proportional
    noise leaves every delta after the first pick equal.  The Woodbury form loses about
    (Sigma_yy / d_y)^2 eps where S >= n (cond C times the cancellation of 1 / d - |t|^2 / d^2), so
    the edge shapes keep the noise well above the 1e-2 diag at which that reaches 1e-12."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, S)) * rng.uniform(0.5, 1.5, (n, 1)) / np.sqrt(S)
    noise = noise_rel * np.sum(F * F, axis=1) * rng.uniform(1.0, 2.0, n)
    return F, noise
