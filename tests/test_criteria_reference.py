"""CPU: the references of the variance-reduction and entropy placements
(tests/numpy_criteria_greedy.py) against definitions that share nothing with them, and the
conditions the inputs of tests/test_gpu_criteria.py must meet."""
import itertools

import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests.greedy_state_reference import require_longdouble


def _posterior(S, A):
    A = list(A)
    return S - S[:, A] @ np.linalg.solve(S[np.ix_(A, A)], S[A, :])


def _small(n=6, seed=1):
    B = np.random.default_rng(seed).standard_normal((n, n + 2))
    return B @ B.T / n + 0.1 * np.eye(n)


def test_first_variance_pick_is_the_brute_force_argmin():
    S = _small()
    traces = [np.trace(_posterior(S, [y])) for y in range(6)]
    for run in (C.reference_run, C.incremental_run):
        rd = run(S, "variance", 1)[0]
        assert rd.pick == int(np.argmin(traces))
        np.testing.assert_allclose(np.asarray(np.trace(S) - rd.delta, dtype=np.float64), traces,
                                   rtol=1e-12)


def test_two_variance_picks_against_exhaustive_greedy():
    S = _small(7, seed=3)
    T = np.array([1, 0, 1, 1, 0, 1, 0], dtype=bool)
    picks = [r.pick for r in C.reference_run(S, "variance", 2, targets=T)]
    first = int(np.argmin([np.trace(_posterior(S, [y])[np.ix_(T, T)]) for y in range(7)]))
    second = min((y for y in range(7) if y != first),
                 key=lambda y: np.trace(_posterior(S, [first, y])[np.ix_(T, T)]))
    assert picks == [first, second]


@pytest.mark.parametrize("name", ["F2", "F3"])
def test_deltas_sum_to_the_trace_reduction(name):
    """sum_r delta_r = tr_T(Sigma) - tr_T(Sigma | A), by a direct solve."""
    require_longdouble()
    S = C.fixture_cov(name)
    n = S.shape[0]
    T, cand = C.odd_even(n)
    rounds = C.reference_run(S, "variance", 8, T, cand)
    A = [r.pick for r in rounds]
    direct = np.trace(S[np.ix_(T, T)]) - np.trace(_posterior(S, A)[np.ix_(T, T)])
    total = float(sum(r.pick_delta for r in rounds))
    assert abs(total - direct) / direct <= 1e-12
    inc = C.incremental_run(S, "variance", 8, T, cand)
    assert [r.pick for r in inc] == A
    assert abs(sum(r.pick_delta for r in inc) - direct) / direct <= 1e-12


def _pivoted_cholesky_pivots(S, k):
    """numpy's diagonal-pivoted (outer-product) Cholesky: the pivot order and the pivots."""
    R = np.array(S, dtype=np.float64)
    piv, val = [], []
    for _ in range(k):
        d = np.diag(R).copy()
        d[piv] = -np.inf
        a = int(np.argmax(d))
        piv.append(a)
        val.append(R[a, a])
        R = R - np.outer(R[:, a], R[a, :]) / R[a, a]
    return piv, val


@pytest.mark.parametrize("name", ["F1", "F2", "F3"])
def test_entropy_is_the_pivoted_cholesky(name):
    require_longdouble()
    S = C.fixture_cov(name)
    k = C.rounds_of(name)
    piv, val = _pivoted_cholesky_pivots(S, k)
    rounds = C.reference(name, "plain", "entropy")
    assert [r.pick for r in rounds] == piv
    np.testing.assert_allclose(np.array([r.pick_delta for r in rounds], dtype=np.float64), val,
                               rtol=1e-10)


@pytest.mark.parametrize("name,config,criterion", C.CONFIGS,
                         ids=["-".join(c) for c in C.CONFIGS])
def test_restatement_and_gap(name, config, criterion):
    """The float64 incremental form reproduces the longdouble picks, every candidate's delta in
    every round to 1e-9 of the round's pick delta (and nom, s, W as the GPU test measures them);
    and the condition on the inputs: the best and the second-best delta of a round differ by
    >= 1e-6 relative, exact ties aside, which resolve to the lower index."""
    require_longdouble()
    S = C.fixture_cov(name)
    T, cand = C.config_masks(name, config)
    T = None if criterion == "entropy" else T
    ref = C.reference(name, config, criterion)
    inc = C.incremental_run(S, criterion, C.rounds_of(name), T, cand)
    assert [r.pick for r in inc] == [r.pick for r in ref]
    gaps = C.round_gaps(ref, cand)
    assert all(low for _, low in gaps)
    assert min(g for g, _ in gaps) >= C.MIN_GAP, min(g for g, _ in gaps)
    smax = float(np.max(np.diag(S)))
    worst = 0.0
    for a, b in zip(inc, ref):
        scale = float(b.pick_delta)
        worst = max(worst,
                    float(np.max(np.abs(a.delta - b.delta))) / scale,
                    float(np.max(np.abs(a.nom - b.nom))) / smax,
                    float(np.max(np.abs(a.w - b.w))) / smax)
        if criterion == "variance":
            worst = max(worst, float(np.max(np.abs(a.s - b.s))) / scale)
    print(f"criteria restatement {name}-{config}-{criterion}: worst error {worst:.2e}, "
          f"smallest gap {min(g for g, _ in gaps):.2e}")
    assert worst <= C.STATE_TOL / 10, worst   # an order of magnitude below the device's 1e-9


def test_exact_tie_goes_to_the_lower_index():
    S = np.eye(5) * 2.0
    S[1, 1] = S[3, 3] = 3.0
    for criterion in ("variance", "entropy"):
        for run in (C.reference_run, C.incremental_run):
            assert [r.pick for r in run(S, criterion, 2)] == [1, 3]


def test_threshold_zeroes_delta():
    S = np.diag([1.0, 1e-9, 2.0])
    for criterion in ("variance", "entropy"):
        rd = C.incremental_run(S, criterion, 1)[0]
        assert rd.delta[1] == 0.0 and rd.pick == 2


def test_placed_continues_a_free_run():
    S = C.fixture_cov("F3")
    free = C.incremental_run(S, "variance", 8)
    picks = [r.pick for r in free]
    cont = C.incremental_run(S, "variance", 4, placed=picks[:4])
    assert [r.pick for r in cont] == picks
    np.testing.assert_allclose([r.pick_delta for r in cont[4:]],
                               [r.pick_delta for r in free[4:]], rtol=1e-9)
    assert list(itertools.islice((r.pick for r in cont), 4)) == picks[:4]
