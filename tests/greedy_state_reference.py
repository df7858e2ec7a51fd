"""TEST INFRASTRUCTURE: an extended-precision reference of the whole state of the greedy placement
kernels (csrc/greedy.hip), and an exact emulator of the lazy-cache policy.  numpy only; never
imported by vgposp_amd/.

``LongdoubleGreedy`` restates ``oracle.placement.all_deltas`` in ``np.longdouble`` without the
n x n inverse: Sigma + eps I = L L^T and M = L^-1 are formed once, with plain column loops (LAPACK
has no longdouble), and every per-candidate quantity of a selected list A then costs
O(n |A|) + one O(n^2) column of Q = M^T M per new member of A:

    nom_y  = sigma_yy - Sigma_yA (Sigma_AA + eps I)^-1 Sigma_Ay = sigma_yy - |W[:, y]|^2
    prec_y = Q_yy - Q_yA Q_AA^-1 Q_Ay                           = Q_yy     - |V[:, y]|^2
    den_y  = 1 / prec_y - eps,   delta_y = nom_y / den_y
    W[t]   = (L_{Sigma_AA + eps I}^-1 Sigma_{A,:})_t,   V[t] = (L_{Q_AA}^-1 Q_{A,:})_t

(prec is the diagonal of (Sigma_SS + eps I)^-1, S = V \\ A: the Schur complement of the A block of
Q.)  A leading principal block of Sigma has the leading blocks of L and of M as its factor and
inverse, so one factorization at the largest order serves every smaller order n; only the column
norms Q_yy and the columns Q e_a are taken from M[:n, :n].

``lazy_round`` follows placement_algorithm2.py:173-208 (``oracle.placement._lazy_select_np``): keys
order by value, ties go to the lower index.
"""
import numpy as np
import pytest

LD = np.longdouble


def require_longdouble():
    """The reference needs a 64-bit significand (x87 extended or better)."""
    if np.finfo(LD).nmant < 63:
        pytest.skip(f"np.longdouble has a {np.finfo(LD).nmant}-bit significand: no extended "
                    "precision to take the reference in")


def chol_lower(A):
    """Lower Cholesky factor of a symmetric positive definite matrix, in the dtype of A."""
    n = A.shape[0]
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def tri_inverse(L):
    """Inverse of a lower triangular matrix by forward substitution, row by row."""
    n = L.shape[0]
    M = np.zeros_like(L)
    for i in range(n):
        M[i, i] = 1 / L[i, i]
        if i:
            M[i, :i] = -(L[i, :i] @ M[:i, :i]) * M[i, i]
    return M


def _forward_rows(LA, R):
    """LA^-1 R for a small lower triangular LA, row after row (the Cholesky rows W / V)."""
    out = np.zeros_like(R)
    for t in range(LA.shape[0]):
        out[t] = (R[t] - LA[t, :t] @ out[:t]) / LA[t, t]
    return out


class GreedyState:
    """What the kernels hold for a selected list A at order n (all longdouble, length n unless
    noted): nom, prec, den, delta (thresholded; entries of A are NaN), W and V [|A|, n]."""

    def __init__(self, nom, prec, den, delta, W, V, sel):
        self.nom, self.prec, self.den, self.delta, self.W, self.V, self.sel = (nom, prec, den,
                                                                               delta, W, V, sel)


class LongdoubleGreedy:
    def __init__(self, Sigma, eps=0.0):
        self.S = np.array(Sigma, dtype=LD)
        self.N = self.S.shape[0]
        self.eps = LD(eps)
        A = self.S.copy()
        A[np.diag_indices(self.N)] += self.eps
        self.L = chol_lower(A)
        self.M = tri_inverse(self.L)
        self._colsq, self._qcol = {}, {}

    def colsq(self, n):
        """Q_yy = |M e_y|^2 of the leading block of order n."""
        if n not in self._colsq:
            Mn = self.M[:n, :n]
            self._colsq[n] = np.sum(Mn * Mn, axis=0)
        return self._colsq[n]

    def mcol(self, a, n):
        """M e_a at order n (zero above row a)."""
        return self.M[:n, a]

    def qcol(self, a, n):
        """Q e_a = M^T (M e_a) at order n."""
        if (n, a) not in self._qcol:
            self._qcol[n, a] = self.M[a:n, a] @ self.M[a:n, :n]
        return self._qcol[n, a]

    def state(self, A, n=None, thr=0.0):
        n = self.N if n is None else int(n)
        A = [int(a) for a in A]
        assert len(set(A)) == len(A) and all(0 <= a < n for a in A)
        m = len(A)
        sel = np.zeros(n, dtype=bool)
        sel[A] = True
        nom = np.diag(self.S)[:n].copy()
        prec = self.colsq(n).copy()
        W = np.zeros((m, n), dtype=LD)
        V = np.zeros((m, n), dtype=LD)
        if m:
            SA = self.S[A][:, :n]
            W = _forward_rows(chol_lower(SA[:, A] + self.eps * np.eye(m, dtype=LD)), SA)
            QA = np.stack([self.qcol(a, n) for a in A])
            V = _forward_rows(chol_lower(QA[:, A].copy()), QA)
            nom -= np.sum(W * W, axis=0)
            prec -= np.sum(V * V, axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            den = 1 / prec - self.eps
            delta = np.where((np.abs(nom) < thr) | (np.abs(den) < thr), LD(0), nom / den)
        delta[sel] = np.nan
        return GreedyState(nom, prec, den, delta, W, V, sel)

    def picks(self, k, n=None, blocked=None, placed=(), lazy=True, cache_init=np.inf):
        """k picks after `placed` by the policy emulator on this reference's own deltas (rounded
        to fp64): the CPU stand-in for a device run."""
        n = self.N if n is None else int(n)
        A = [int(a) for a in placed]
        cache = np.full(n, float(cache_init))
        off = np.zeros(n, dtype=bool) if blocked is None else np.array(blocked, dtype=bool)
        off[A] = True
        for _ in range(k):
            d = self.state(A[:], n).delta.astype(np.float64)
            y, _, cache = lazy_round(cache, d, off, lazy)
            A.append(y)
            off[y] = True
        return A[len(placed):]


# ---- comparing one round of a run (the fp64 host restatement, or the device) with the state ----
def round_errors(ref, n, picks, r, delta, piv, xcol, blocked=None):
    """Errors of round r of a run whose picks so far were picks[:r] and whose pick is picks[r].

    delta [n]: compared for every i neither in picks[:r] nor blocked, relative.
    piv [>= 2 + 2 r]: nom_y and P_yy of the pick relative; W[0..r)[y] and V[0..r)[y] normwise
    (|error| / max |row t|).  xcol [n] (None: not compared; unused in round 0): column
    a = picks[r-1] of L^-1, normwise in rows >= a; ``xcol_above`` is the number of non-zero
    entries above row a (must be 0).
    Also returns min |nom| and min |den| over the compared candidates (the threshold distance)."""
    A, y = [int(a) for a in picks[:r]], int(picks[r])
    st = ref.state(A, n)
    use = ~st.sel
    if blocked is not None:
        use &= ~np.asarray(blocked, dtype=bool)
    assert use[y]
    d = np.asarray(delta, dtype=np.float64)[:n].astype(LD)
    out = {"delta": float(np.max(np.abs(d[use] - st.delta[use]) / np.abs(st.delta[use]))),
           "min_nom": float(np.min(np.abs(st.nom[use]))),
           "min_den": float(np.min(np.abs(st.den[use])))}
    p = np.asarray(piv, dtype=np.float64).astype(LD)
    out["nom_y"] = float(abs(p[0] - st.nom[y]) / abs(st.nom[y]))
    out["prec_y"] = float(abs(p[1] - st.prec[y]) / abs(st.prec[y]))
    out["W"] = out["V"] = out["xcol"] = 0.0
    out["xcol_above"] = 0
    if r:
        out["W"] = float(np.max(np.abs(p[2:2 + r] - st.W[:, y]) / np.max(np.abs(st.W), axis=1)))
        out["V"] = float(np.max(np.abs(p[2 + r:2 + 2 * r] - st.V[:, y])
                                / np.max(np.abs(st.V), axis=1)))
    if r and xcol is not None:
        a = A[-1]
        x = np.asarray(xcol, dtype=np.float64)[:n]
        col = ref.mcol(a, n)
        out["xcol"] = float(np.max(np.abs(x[a:].astype(LD) - col[a:])) / np.max(np.abs(col[a:])))
        out["xcol_above"] = int(np.count_nonzero(x[:a]))
    return out


ERROR_KEYS = ("delta", "nom_y", "prec_y", "W", "V", "xcol")


def worst(errs, keys=ERROR_KEYS):
    return max(e[k] for e in errs for k in keys)


def backend_forced_rounds(Sigma, n, picks, eps=0.0):
    """tests/numpy_greedy_backend.NumpyGreedyBackend (fp64, host LAPACK, the kernels' incremental
    algorithm) driven through len(picks) rounds whose picks are given: per round (delta, piv,
    xcol) as the device holds them after that round."""
    from tests.numpy_greedy_backend import NumpyGreedyBackend
    K = np.ascontiguousarray(np.asarray(Sigma, dtype=np.float64)[:n, :n])
    b = NumpyGreedyBackend(K, len(picks), jitter=eps)
    b.init()
    rounds = []
    for r, y in enumerate(picks):
        y = int(y)
        b.update(r, 0, n)
        d = b.delta().numpy()
        # the tail of NumpyGreedyBackend.select for a given pick
        b.selected.append(y)
        b.sel_delta.append(d[y])
        b.sel[y] = True
        p = b.piv().numpy()
        p[:] = 0.0
        p[0], p[1] = b.nom[y], b.prec[y]
        p[2:2 + r] = b.W[:r, y]
        p[2 + r:2 + 2 * r] = b.V[:r, y]
        rounds.append((d.copy(), p.copy(), b.M[:, picks[r - 1]].copy() if r else None))
    return rounds


def backend_errors(ref, Sigma, n, picks, eps=0.0, blocked=None, first=0):
    """round_errors of the fp64 restatement over rounds first .. len(picks) - 1."""
    rounds = backend_forced_rounds(Sigma, n, picks, eps)
    return [round_errors(ref, n, picks, r, *rounds[r], blocked=blocked)
            for r in range(first, len(picks))]


# ---- the lazy policy ----
def lazy_round(cache, delta, blocked, lazy=True):
    """One selection round.  cache [n]: the lazy cache before the round; delta [n]: this round's
    fresh deltas (entries of blocked candidates are never read); blocked [n]: selected or masked.
    Returns (pick, evaluated candidates in the reference's order, cache after the round).

    lazy: placement_algorithm2.py:173-208 — take the arg-max of the cache (value, then lower
    index); if it was evaluated this round select it, else evaluate it and look again.
    full greedy (:105-145): every unblocked candidate is evaluated, the arg-max of delta is
    selected, the cache is not used."""
    cache = np.array(cache, dtype=np.float64)
    delta = np.asarray(delta, dtype=np.float64)
    blocked = np.asarray(blocked, dtype=bool)
    if blocked.all():
        return -1, [], cache
    if not lazy:
        y = int(np.argmax(np.where(blocked, -np.inf, delta)))
        return y, [int(i) for i in np.flatnonzero(~blocked)], cache
    uptodate = np.zeros(len(cache), dtype=bool)
    evaluated = []
    while True:
        y = int(np.argmax(np.where(blocked, -np.inf, cache)))
        if uptodate[y]:
            return y, evaluated, cache
        cache[y] = delta[y]
        uptodate[y] = True
        evaluated.append(y)


# ---- the inputs of tests/test_gpu_greedy_state.py, and the conditions they must meet ----
NOISE = 1e-2 + 1e-6
FIXTURES = {
    # name: (kind, grid shape, (jitter eps, threshold, cache_init))
    "F1": ("eq", (13, 10, 8), (0.0, 1e-8, np.inf)),
    "F2": ("matern52", (9, 9, 8), (0.0, 1e-8, np.inf)),
    "F3": ("eq", (9, 9, 8), (1e-6, 1e-7, 1e8)),
}
F1_ORDERS = (2, 130, 512, 513, 1024, 1025, 1039, 1040)
ROUNDS = 6
PLACED = [3, 517, 1030, 64, 1023, 1024]
MIN_DISTANCE = 1e-6      # of |nom| and |den| from the kernels' zeroing thresholds (<= 1e-7)
TOL_FACTOR = 16.0
TOL_CEILING = 1e-11
COND_RANGE = (1e3, 2e4)  # cond(K) of the inputs: 8.5e3 (eq) and 6.3e3 (matern52) at 1040


def rounds_at(n):
    return ROUNDS if n >= ROUNDS else min(4, n)


def third_mask(n):
    """Blocks every third location (the candidates of tests/test_gpu_constrained.py)."""
    return np.arange(n) % 3 == 1


def fixture_cov(name):
    from oracle import gp as ogp
    from vgposp_amd.data_generation import grid_points, grid_spacing
    kind, shape, _ = FIXTURES[name]
    X = grid_points(shape, jitter=0.05, seed=3)
    return ogp.kernel_matrix(kind, X, X, 1.0, 2 * grid_spacing(shape))[0] + NOISE * np.eye(len(X))


_built = {}


def fixture(name):
    """(K fp64, LongdoubleGreedy of it, params) — built once per process."""
    if name not in _built:
        require_longdouble()
        K = fixture_cov(name)
        _built[name] = (K, LongdoubleGreedy(K, FIXTURES[name][2][0]), FIXTURES[name][2])
    return _built[name]


def tolerance(e_cpu):
    """The device's tolerance from the fp64 restatement's error on the same Sigma and picks."""
    tol = TOL_FACTOR * e_cpu
    assert tol <= TOL_CEILING, (f"16 e_cpu = {tol:.3e} is above the ceiling {TOL_CEILING:.0e}: "
                                "the input is too ill-conditioned for this test")
    return tol
