"""TEST INFRASTRUCTURE: references of the variance-reduction and entropy placements
(csrc/criteria.hip, vgposp_amd/placement_criteria.py).  numpy only; never imported by vgposp_amd/.

``reference_run`` (np.longdouble) keeps the whole conditional covariance C, recomputes every delta
directly from it each round and downdates it by the rank-1 term of the pick:

    variance: delta_y = sum_{v in T} C_vy^2 / C_yy        entropy: delta_y = C_yy
    C_yy < thr -> 0;   pick = arg-max over candidates \\ A, ties to the lower index
    C <- C - C_{:,a} C_{a,:} / C_aa

``incremental_run`` (float64) is the kernels' algorithm: nom, s and the rows W, one product with
the unfactored Sigma per round.

Both return one ``Round`` per round (forced rounds on ``placed`` first): ``delta`` as scored
before the pick, ``pick``, ``pick_delta``, and ``nom``, ``s``, ``w`` (the new row of W) after it.
"""
import numpy as np

LD = np.longdouble
THRESHOLD = 1e-8
K_ROUNDS = 16
MIN_GAP = 1e-6        # relative, between the best and the second-best delta of a round
STATE_TOL = 1e-9      # the project's tolerance for deltas


class Round:
    def __init__(self, delta, pick, pick_delta, nom, s, w):
        self.delta, self.pick, self.pick_delta, self.nom, self.s, self.w = (delta, pick,
                                                                            pick_delta, nom, s, w)


def as_mask(n, arg):
    """None / index list / bool mask -> bool mask [n] (None: all True)."""
    if arg is None:
        return np.ones(n, dtype=bool)
    a = np.asarray(arg)
    if a.dtype == np.bool_:
        assert a.shape == (n,)
        return a.copy()
    m = np.zeros(n, dtype=bool)
    m[a] = True
    return m


def argmax_low(delta, free):
    """Arg-max of delta over ``free``; ties go to the lower index (np.argmax takes the first)."""
    return int(np.argmax(np.where(free, delta, -np.inf)))


def _deltas(C_diag, s, criterion, thr):
    with np.errstate(divide="ignore", invalid="ignore"):
        d = C_diag.copy() if criterion == "entropy" else s / C_diag
    d[C_diag < thr] = 0
    return d


def reference_run(Sigma, criterion, k, targets=None, candidates=None, placed=(), thr=THRESHOLD,
                  dtype=LD):
    n = Sigma.shape[0]
    C = np.array(Sigma, dtype=dtype)
    T, free = as_mask(n, targets), as_mask(n, candidates)
    free[list(placed)] = False
    rounds = []
    for r in range(len(placed) + k):
        diag = np.diag(C).copy()
        s = np.sum(C[T] * C[T], axis=0)
        delta = _deltas(diag, s, criterion, dtype(thr))
        a = int(placed[r]) if r < len(placed) else argmax_low(delta, free)
        free[a] = False
        w = C[a] / np.sqrt(C[a, a]) if C[a, a] >= thr else np.zeros(n, dtype=dtype)
        C -= np.outer(w, w)
        rounds.append(Round(delta, a, delta[a], np.diag(C).copy(),
                            np.sum(C[T] * C[T], axis=0), w))
    return rounds


def incremental_run(Sigma, criterion, k, targets=None, candidates=None, placed=(),
                    thr=THRESHOLD):
    """float64: the incremental form of the kernels, with numpy's own summation order."""
    S = np.asarray(Sigma, dtype=np.float64)
    n = S.shape[0]
    T, free = as_mask(n, targets), as_mask(n, candidates)
    free[list(placed)] = False
    t = T.astype(np.float64)
    nom = np.diag(S).copy()
    s = (S * S).T @ t
    W = np.zeros((0, n))
    rounds = []
    for r in range(len(placed) + k):
        delta = _deltas(nom, s, criterion, thr)
        a = int(placed[r]) if r < len(placed) else argmax_low(delta, free)
        free[a] = False
        w = (S[a] - W[:, a] @ W) / np.sqrt(nom[a]) if nom[a] >= thr else np.zeros(n)
        wt = w * t
        g = S @ wt - W.T @ (W @ wt)
        s = s - 2 * w * g + w * w * (wt @ wt)
        nom = nom - w * w
        W = np.vstack([W, w])
        rounds.append(Round(delta, a, delta[a], nom.copy(), s.copy(), w))
    return rounds


def round_gaps(rounds, candidates, placed=()):
    """Per free round: the relative gap between the best and the second-best distinct delta over
    the candidates free in that round, and whether the pick is the lowest index of the best."""
    n = len(rounds[0].delta)
    free = as_mask(n, candidates)
    free[list(placed)] = False
    out = []
    for r, rd in enumerate(rounds):
        if r >= len(placed):
            d = np.where(free, rd.delta, -np.inf)
            best = d[rd.pick]
            assert best == d.max()
            lowest = rd.pick == int(np.flatnonzero(d == best)[0])
            rest = d[d < best]
            gap = float((best - rest.max()) / best) if rest.size and best > 0 else np.inf
            out.append((gap, lowest))
        free[rd.pick] = False
    return out


# ---- fixtures ----
FIXTURES = {"F1": ("eq", (12, 11, 10), 11), "F2": ("matern52", (13, 9, 7), 12)}


def grid_cov(kind, shape, seed):
    """D (K + 1e-2 I) D on a grid jittered by +-0.3 of a spacing, D = diag of a fixed random
    amplitude field in [1, 1.3]: the prior variances differ."""
    from oracle import gp as ogp
    from vgposp_amd.data_generation import grid_points, grid_spacing
    X = grid_points(shape, jitter=0.3, seed=seed)
    K = ogp.kernel_matrix(kind, X, X, 1.0, 2 * grid_spacing(shape))[0] + 1e-2 * np.eye(len(X))
    a = np.random.default_rng(seed + 100).uniform(1.0, 1.3, len(X))
    return np.ascontiguousarray(a[:, None] * K * a[None, :])


def low_rank_cov(seed=5):
    """F3: Z Z^T / 40 with Z 200 x 40 standard normal (rank 40, singular)."""
    Z = np.random.default_rng(seed).standard_normal((200, 40))
    return Z @ Z.T / 40


def random_masks(n, seed=7):
    """targets: half of V; candidates: 60 %."""
    rng = np.random.default_rng(seed)
    return rng.permutation(n) < n // 2, rng.permutation(n) < (6 * n) // 10


def odd_even(n):
    """T = the odd indices, S = the even ones (disjoint)."""
    return np.arange(n) % 2 == 1, np.arange(n) % 2 == 0


_cov, _ref = {}, {}


def fixture_cov(name):
    if name not in _cov:
        _cov[name] = low_rank_cov() if name == "F3" else grid_cov(*FIXTURES[name])
        _cov[name].setflags(write=False)
    return _cov[name]


def config_masks(name, config):
    n = fixture_cov(name).shape[0]
    return {"plain": (None, None), "random": random_masks(n), "oddeven": odd_even(n)}[config]


# every (fixture, configuration, rule) the GPU test runs; entropy has no target set
CONFIGS = ([(f, c, "variance") for f in ("F1", "F2") for c in ("plain", "random", "oddeven")]
           + [(f, c, "entropy") for f in ("F1", "F2") for c in ("plain", "random", "oddeven")]
           + [("F3", "plain", "variance"), ("F3", "plain", "entropy")])


def rounds_of(name):
    return 10 if name == "F3" else K_ROUNDS


def reference(name, config, criterion):
    """The longdouble rounds of a configuration, computed once per process and left unchanged."""
    key = (name, config, criterion)
    if key not in _ref:
        T, S = config_masks(name, config)
        _ref[key] = reference_run(fixture_cov(name), criterion, rounds_of(name),
                                  None if criterion == "entropy" else T, S)
    return _ref[key]
