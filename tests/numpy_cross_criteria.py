"""TEST INFRASTRUCTURE: references of the variance-reduction placement for targets outside V
(the vgposp_critx_* entries of csrc/criteria.hip, CriterionPlacement(cross_cov=...)).  numpy only;
never imported by vgposp_amd/.

Sigma [n, n] is the covariance of the locations, R [P, n] the covariance between the P targets and
the locations, omega [P] >= 0 the targets' weights.  ``reference_run`` (np.longdouble) keeps the
whole conditional covariance C and the whole conditional cross-covariance D, recomputes every delta
directly from them each round and downdates both by the rank-1 term of the pick:

    delta_y = sum_v omega_v D_vy^2 / C_yy;   C_yy < thr -> 0
    pick = arg-max over candidates \\ A, ties to the lower index
    w = C_{a,:} / sqrt(C_aa),  u = D_{:,a} / sqrt(C_aa);   C <- C - w w^T,  D <- D - u w^T

``incremental_run`` (float64) is the kernels' algorithm: nom, s, the rows W and U, one product with
the unfactored R per round.

Both return one ``Round`` per round (forced rounds on ``placed`` first): ``delta`` as scored before
the pick, ``pick``, ``pick_delta``, and ``nom``, ``s``, ``w``, ``u`` (the new rows of W and U)
after it.
"""
import numpy as np

from tests.numpy_criteria_greedy import LD, THRESHOLD, argmax_low, as_mask

K_ROUNDS = 12
MIN_GAP = 1e-6        # relative, between the best and the second-best delta of a round
STATE_TOL = 1e-9      # the project's tolerance for deltas


class Round:
    def __init__(self, delta, pick, pick_delta, nom, s, w, u):
        self.delta, self.pick, self.pick_delta = delta, pick, pick_delta
        self.nom, self.s, self.w, self.u = nom, s, w, u


def _deltas(C_diag, s, thr):
    with np.errstate(divide="ignore", invalid="ignore"):
        d = s / C_diag
    d[C_diag < thr] = 0
    return d


def _weights(P, weights, dtype):
    return np.ones(P, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)


def reference_run(Sigma, R, k, weights=None, candidates=None, placed=(), thr=THRESHOLD, dtype=LD):
    n, P = Sigma.shape[0], R.shape[0]
    C, D = np.array(Sigma, dtype=dtype), np.array(R, dtype=dtype)
    om = _weights(P, weights, dtype)
    free = as_mask(n, candidates)
    free[list(placed)] = False
    rounds = []
    for r in range(len(placed) + k):
        delta = _deltas(np.diag(C).copy(), om @ (D * D), dtype(thr))
        a = int(placed[r]) if r < len(placed) else argmax_low(delta, free)
        free[a] = False
        if C[a, a] >= thr:
            w, u = C[a] / np.sqrt(C[a, a]), D[:, a] / np.sqrt(C[a, a])
        else:
            w, u = np.zeros(n, dtype=dtype), np.zeros(P, dtype=dtype)
        C -= np.outer(w, w)
        D -= np.outer(u, w)
        rounds.append(Round(delta, a, delta[a], np.diag(C).copy(), om @ (D * D), w, u))
    return rounds


def incremental_run(Sigma, R, k, weights=None, candidates=None, placed=(), thr=THRESHOLD):
    """float64: the incremental form of the kernels, with numpy's own summation order."""
    S, R = np.asarray(Sigma, dtype=np.float64), np.asarray(R, dtype=np.float64)
    n, P = S.shape[0], R.shape[0]
    om = _weights(P, weights, np.float64)
    free = as_mask(n, candidates)
    free[list(placed)] = False
    nom = np.diag(S).copy()
    s = (R * R).T @ om
    W, U = np.zeros((0, n)), np.zeros((0, P))
    rounds = []
    for r in range(len(placed) + k):
        delta = _deltas(nom, s, thr)
        a = int(placed[r]) if r < len(placed) else argmax_low(delta, free)
        free[a] = False
        if nom[a] >= thr:
            w = (S[a] - W[:, a] @ W) / np.sqrt(nom[a])
            u = (R[:, a] - W[:, a] @ U) / np.sqrt(nom[a])
        else:
            w, u = np.zeros(n), np.zeros(P)
        wu = om * u
        g = R.T @ wu - W.T @ (U @ wu)
        s = s - 2 * w * g + w * w * (u @ wu)
        nom = nom - w * w
        W, U = np.vstack([W, w]), np.vstack([U, u])
        rounds.append(Round(delta, a, delta[a], nom.copy(), s.copy(), w, u))
    return rounds


# ---- fixtures ----
# name: (kernel, sensor grid, its seed, target grid, its seed)
FIXTURES = {"X1": ("eq", (9, 8, 7), 21, (14, 12, 10), 71),
            "X2": ("matern52", (10, 7, 6), 22, (13, 11, 9), 72)}
CONFIGS = [(f, c) for f in ("X1", "X2") for c in ("plain", "weighted")]


def joint_cov(kind, sshape, sseed, tshape, tseed):
    """(Sigma, R): sensors and targets on two grids jittered by +-0.3 of their spacing, length
    scale 2 x the sensor spacing, one amplitude field a in [1, 1.3] over both sets;
    Sigma = a_s (K_ss + 1e-2 I) a_s (the noise 1e-2 a^2 sits on Sigma's diagonal alone),
    R = a_t K_ts a_s (the latent field at the targets)."""
    from oracle import gp as ogp
    from vgposp_amd.data_generation import grid_points, grid_spacing
    Xs = grid_points(sshape, jitter=0.3, seed=sseed)
    Xt = grid_points(tshape, jitter=0.3, seed=tseed)
    ls = 2 * grid_spacing(sshape)
    n, P = len(Xs), len(Xt)
    a = np.random.default_rng(sseed + 100).uniform(1.0, 1.3, n + P)
    Kss = ogp.kernel_matrix(kind, Xs, Xs, 1.0, ls)[0] + 1e-2 * np.eye(n)
    Kts = ogp.kernel_matrix(kind, Xt, Xs, 1.0, ls)[0]
    return (np.ascontiguousarray(a[:n, None] * Kss * a[None, :n]),
            np.ascontiguousarray(a[n:, None] * Kts * a[None, :n]))


def low_rank_joint(seed=6):
    """X3: [Sigma; R] = Z Z^T / 40 with Z (200 + 300) x 40 standard normal: rank 40, singular."""
    Z = np.random.default_rng(seed).standard_normal((500, 40))
    G = Z @ Z[:200].T / 40
    return np.ascontiguousarray(G[:200]), np.ascontiguousarray(G[200:])


def weighted_config(n, P, seed=9):
    """weights: about 10 % zeros, the rest in [0.5, 2]; candidates: 60 %."""
    rng = np.random.default_rng(seed)
    om = rng.uniform(0.5, 2.0, P)
    om[rng.random(P) < 0.1] = 0.0
    return om, rng.permutation(n) < (6 * n) // 10


_cov, _ref = {}, {}


def fixture(name):
    """(Sigma, R) of a fixture, computed once per process and read-only."""
    if name not in _cov:
        _cov[name] = low_rank_joint() if name == "X3" else joint_cov(*FIXTURES[name])
        for M in _cov[name]:
            M.setflags(write=False)
    return _cov[name]


def config(name, cfg):
    """(weights, candidates) of a configuration."""
    S, R = fixture(name)
    return (None, None) if cfg == "plain" else weighted_config(S.shape[0], R.shape[0])


def reference(name, cfg):
    """The longdouble rounds of a configuration, computed once per process and left unchanged."""
    if (name, cfg) not in _ref:
        S, R = fixture(name)
        om, cand = config(name, cfg)
        _ref[name, cfg] = reference_run(S, R, K_ROUNDS, om, cand)
    return _ref[name, cfg]
