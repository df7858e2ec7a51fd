"""CPU: the longdouble reference of the greedy kernels' state and the lazy-policy emulator
(tests/greedy_state_reference.py) are themselves checked here, against oracle.placement and
tests/numpy_greedy_backend, and the conditions that tests/test_gpu_greedy_state.py puts on its
inputs are asserted for every one of them, so a violated condition shows up without a GPU."""
import numpy as np
import pytest

from oracle import gp as ogp
from oracle import placement as op
from tests import greedy_state_reference as R
from tests.numpy_greedy_backend import NumpyGreedyBackend

LD = np.longdouble
# fp64 restatements against longdouble at n <= 216, cond(K) < 1e4: n cond u = 2e-10 is the
# worst-case bound; the ceiling the device tests use is asked of the host restatements too
FP64_RTOL = R.TOL_CEILING


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def grid216():
    R.require_longdouble()
    from vgposp_amd.data_generation import grid_points, grid_spacing
    shape = (6, 6, 6)
    X = grid_points(shape, jitter=0.05, seed=3)
    K = ogp.kernel_matrix("eq", X, X, 1.0, 2 * grid_spacing(shape))[0] + R.NOISE * np.eye(216)
    return K, {eps: R.LongdoubleGreedy(K, eps) for eps in (0.0, 1e-6)}


def _rel(got, want, use):
    return float(np.max(np.abs(np.asarray(got)[use].astype(LD) - want[use]) / np.abs(want[use])))


@pytest.mark.parametrize("eps", [0.0, 1e-6])
@pytest.mark.parametrize("m", [0, 1, 5])
def test_longdouble_deltas_match_the_fp64_restatements(grid216, eps, m):
    K, refs = grid216
    ref = refs[eps]
    A = [107, 3, 215, 64, 150][:m]
    st = ref.state(A, thr=op.DELTA_EPS)
    use = ~st.sel
    assert not np.isnan(st.delta[use]).any() and np.isnan(st.delta[~use]).all()
    # the residuals that define the factor and the inverse, in longdouble
    Kj = K.astype(LD) + LD(eps) * np.eye(216, dtype=LD)
    assert np.max(np.abs(ref.L @ ref.L.T - Kj)) < 1e-17
    assert np.max(np.abs(ref.M @ ref.L - np.eye(216, dtype=LD))) < 1e-15
    # oracle.placement.all_deltas: the same quantities from a dense inverse of Sigma_SS
    d, nom, den = op.all_deltas(K, A, eps)
    e_all = max(_rel(d, st.delta, use), _rel(nom, st.nom, use), _rel(den, st.den, use))
    # NumpyGreedyBackend: the kernels' incremental algorithm
    picks = A + [int(np.flatnonzero(use)[0])]
    errs = R.backend_errors(ref, K, 216, picks, eps)
    e_inc = R.worst(errs)
    print(f"n 216 eps {eps:g} |A| {m}: all_deltas {e_all:.2e}, incremental {e_inc:.2e} "
          f"(bound {FP64_RTOL:.0e})")
    assert e_all <= FP64_RTOL and e_inc <= FP64_RTOL


@pytest.mark.parametrize("n", [1, 2, 130, 215])
def test_leading_block_reuse(grid216, n):
    """The leading blocks of L and M are the factor and inverse of the leading block of Sigma:
    the state at order n from the 216-order factorization against a factorization at n."""
    K, refs = grid216
    A = [a for a in (107, 3, 64, 0, 1) if a < n][:max(0, min(3, n - 1))]
    for eps, big in refs.items():
        small = R.LongdoubleGreedy(K[:n, :n], eps)
        assert np.array_equal(small.L, big.L[:n, :n])
        # u_ld = 5.4e-20: rows of M are formed by the same recurrence, sums possibly blocked
        # differently
        assert np.max(np.abs(small.M - big.M[:n, :n])) <= 1e-16 * np.max(np.abs(small.M))
        a, b = small.state(A), big.state(A, n)
        use = ~a.sel
        for f in ("nom", "prec", "den", "delta"):
            x, y = getattr(a, f)[use], getattr(b, f)[use]
            assert np.max(np.abs(x - y) / np.abs(x)) <= 1e-16, f
        assert np.max(np.abs(a.W - b.W), initial=0) <= 1e-17 and \
            np.max(np.abs(a.V - b.V), initial=0) <= 1e-14 * np.max(np.abs(a.V), initial=1)


@pytest.mark.parametrize("cache_init", [np.inf, 50.0])
@pytest.mark.parametrize("lazy", [True, False])
def test_emulator_reproduces_the_numpy_backend(grid216, lazy, cache_init):
    K, _ = grid216
    n, k = 216, 8
    b = NumpyGreedyBackend(K, k)
    b.init()
    b.cache[:] = cache_init
    refreshed = 0
    for r in range(k):
        b.update(r, 0, n)
        before, blocked = b.cache.copy(), b.sel.copy()
        d = b.delta().numpy().copy()
        b.select(r, lazy, 0, n)
        y, ev, after = R.lazy_round(before, d, blocked, lazy)
        assert y == b.selected[r]
        assert np.array_equal(_bits(after), _bits(b.cache))
        assert len(set(ev)) == len(ev) and not blocked[ev].any()
        untouched = np.ones(n, dtype=bool)
        untouched[ev] = False
        if lazy:
            assert np.array_equal(_bits(after[ev]), _bits(d[ev]))
            assert np.array_equal(_bits(after[untouched]), _bits(before[untouched]))
            refreshed += len(ev)
            # the same decisions as the scan of placement_algorithm2.py:53-67
            c2 = before.copy()
            y2, ev2 = op.lazy_select(c2, d, blocked)
            assert (y2, ev2) == (y, ev) and np.array_equal(_bits(c2), _bits(after))
        else:
            assert len(ev) == n - r and np.array_equal(_bits(after), _bits(before))
    if lazy:
        # infinite: round 0 evaluates everyone.  50.0: the stale 50.0 entries shut out every
        # fresh delta below them, and the rounds evaluate fewer than everyone
        assert (refreshed >= n) if np.isinf(cache_init) else (0 < refreshed < n)


def test_emulator_ties_and_mask():
    cache = np.array([np.inf, 5.0, np.inf, 5.0, 7.0])
    delta = np.array([np.nan, 5.0, 5.0, 5.0, 1.0])
    blocked = np.array([True, False, False, False, False])
    y, ev, after = R.lazy_round(cache, delta, blocked)
    assert (y, ev) == (1, [2, 4, 1])               # ties: the lower index first
    assert np.array_equal(after[1:], [5.0, 5.0, 5.0, 1.0]) and np.isinf(after[0])
    assert R.lazy_round(cache, delta, blocked, lazy=False)[:2] == (1, [1, 2, 3, 4])
    assert R.lazy_round(cache, delta, np.ones(5, dtype=bool))[0] == -1


# ---- the conditions on the inputs of tests/test_gpu_greedy_state.py ----
def _gpu_inputs():
    for n in R.F1_ORDERS:
        yield f"F1-{n}", "F1", n, False, (), None
    yield "F2", "F2", None, False, (), None
    yield "F3", "F3", None, False, (), None
    yield "F1-cache_init-50", "F1", None, False, (), 50.0
    yield "F1-cache_init-tied", "F1", None, False, (), "tied"
    yield "F1-masked", "F1", None, True, (), None
    yield "F1-placed", "F1", None, False, tuple(R.PLACED), None


@pytest.mark.parametrize("case", list(_gpu_inputs()), ids=lambda c: c[0])
def test_conditions_on_the_gpu_inputs(case):
    """Threshold distance, conditioning and the tolerance ceiling, with the picks of the policy
    emulator on the longdouble deltas standing in for the device's (the GPU tests assert the same
    on the device's own picks)."""
    _, name, n, masked, placed, cache_init = case
    K, ref, (eps, thr, cinit) = R.fixture(name)
    n = K.shape[0] if n is None else n
    assert thr <= 1e-7 < R.MIN_DISTANCE
    if n == K.shape[0]:
        cond = np.linalg.cond(K)
        assert R.COND_RANGE[0] <= cond <= R.COND_RANGE[1], cond
    blocked = R.third_mask(n) if masked else None
    k = 2 if placed else R.rounds_at(n)
    if cache_init == "tied":  # the largest round-0 delta (test_policy_tied_cache_init)
        cache_init = float(np.nanmax(ref.state([], n).delta.astype(np.float64)))
    picks = list(placed) + ref.picks(k, n, blocked=blocked, placed=placed,
                                     cache_init=cinit if cache_init is None else cache_init)
    errs = R.backend_errors(ref, K, n, picks, eps, blocked=blocked, first=max(len(placed) - 1, 0))
    e_cpu = max(e["delta"] for e in errs)
    tol = R.tolerance(e_cpu)
    lo_nom, lo_den = min(e["min_nom"] for e in errs), min(e["min_den"] for e in errs)
    print(f"{case[0]}: n {n} rounds {len(errs)} e_cpu {e_cpu:.2e} (all quantities "
          f"{R.worst(errs):.2e}) tol {tol:.2e} min|nom| {lo_nom:.2e} min|den| {lo_den:.2e}")
    assert lo_nom >= R.MIN_DISTANCE and lo_den >= R.MIN_DISTANCE
