"""CPU: the references of the variance-reduction placement for targets outside V
(tests/numpy_cross_criteria.py) against each other, against the in-V reference, against a direct
solve, and the conditions the inputs of tests/test_gpu_cross_criteria.py must meet."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_cross_criteria as X
from tests.greedy_state_reference import require_longdouble


@pytest.mark.parametrize("name,cfg", X.CONFIGS, ids=["-".join(c) for c in X.CONFIGS])
def test_restatement_and_gap(name, cfg):
    """The float64 incremental form reproduces the longdouble picks and state (measured as the GPU
    test measures them) an order of magnitude below the device's 1e-9; every round's best and
    second-best delta differ by >= 1e-6 relative, and the pick is the lowest index of the best."""
    require_longdouble()
    S, R = X.fixture(name)
    om, cand = X.config(name, cfg)
    ref = X.reference(name, cfg)
    inc = X.incremental_run(S, R, X.K_ROUNDS, om, cand)
    assert [r.pick for r in inc] == [r.pick for r in ref]
    gaps = C.round_gaps(ref, cand)
    assert all(low for _, low in gaps)
    assert min(g for g, _ in gaps) >= X.MIN_GAP, min(g for g, _ in gaps)
    smax = float(np.max(np.diag(S)))
    worst = 0.0
    for a, b in zip(inc, ref):
        scale = float(b.pick_delta)
        worst = max(worst,
                    float(np.max(np.abs(a.delta - b.delta))) / scale,
                    float(np.max(np.abs(a.s - b.s))) / scale,
                    float(np.max(np.abs(a.nom - b.nom))) / smax,
                    float(np.max(np.abs(a.w - b.w))) / smax,
                    float(np.max(np.abs(a.u - b.u))) / smax)
    print(f"cross criteria restatement {name}-{cfg}: worst error {worst:.2e}, "
          f"smallest gap {min(g for g, _ in gaps):.2e}")
    assert worst <= X.STATE_TOL / 10, worst
    if cand is not None:
        assert cand[[r.pick for r in ref]].all()


@pytest.mark.parametrize("name", ["F1", "F2"])
def test_rows_of_sigma_as_targets_reproduce_the_in_v_reference(name):
    """R = Sigma[T, :], omega = 1 is the in-V rule with targets T."""
    require_longdouble()
    S = C.fixture_cov(name)
    T, cand = C.odd_even(S.shape[0])
    want = C.reference_run(S, "variance", 8, targets=T, candidates=cand)
    got = X.reference_run(S, S[T], 8, candidates=cand)
    assert [r.pick for r in got] == [r.pick for r in want]
    for a, b in zip(got, want):
        assert (np.abs(a.delta - b.delta) <= 1e-12 * np.abs(b.delta)).all()   # (0 where picked)
        assert abs(a.pick_delta - b.pick_delta) <= 1e-12 * b.pick_delta


@pytest.mark.parametrize("name,cfg", X.CONFIGS + [("X3", "plain")],
                         ids=["-".join(c) for c in X.CONFIGS] + ["X3-plain"])
def test_deltas_sum_to_the_weighted_variance_reduction(name, cfg):
    """sum_r delta_r = omega . (prior - posterior variance) = omega . diag(R_A Sigma_AA^-1 R_A^T),
    the posterior by a direct solve; per target it is sum_r U_r[v]^2."""
    require_longdouble()
    S, R = X.fixture(name)
    om, cand = X.config(name, cfg)
    k = 8
    for run in (X.reference_run, X.incremental_run):
        rounds = run(S, R, k, om, cand)
        A = [r.pick for r in rounds]
        removed = np.sum(R[:, A] * np.linalg.solve(S[np.ix_(A, A)], R[:, A].T).T, axis=1)
        direct = float((np.ones(len(removed)) if om is None else om) @ removed)
        total = float(sum(r.pick_delta for r in rounds))
        assert abs(total - direct) <= 1e-10 * direct, (total, direct)
        per_target = np.sum(np.array([r.u for r in rounds], dtype=np.float64) ** 2, axis=0)
        assert np.max(np.abs(per_target - removed)) <= 1e-10 * np.max(removed)


def test_singular_fixture_restatement_and_gap():
    """X3 (rank 40, no jitter), the ten rounds the GPU test runs."""
    require_longdouble()
    S, R = X.fixture("X3")
    ref = X.reference_run(S, R, 10)
    inc = X.incremental_run(S, R, 10)
    assert [r.pick for r in inc] == [r.pick for r in ref]
    gaps = C.round_gaps(ref, None)
    assert all(low for _, low in gaps) and min(g for g, _ in gaps) >= X.MIN_GAP
    for a, b in zip(inc, ref):
        assert abs(a.pick_delta - b.pick_delta) <= X.STATE_TOL / 10 * b.pick_delta


def test_first_pick_is_the_brute_force_argmin():
    rng = np.random.default_rng(2)
    B = rng.standard_normal((6 + 9, 8))
    G = B @ B.T / 8
    S, R = G[:6, :6] + 0.1 * np.eye(6), G[6:, :6]
    om = rng.uniform(0.5, 2.0, 9)
    post = [om @ (np.diag(G[6:, 6:]) - R[:, y] ** 2 / S[y, y]) for y in range(6)]
    for run in (X.reference_run, X.incremental_run):
        rd = run(S, R, 1, om)[0]
        assert rd.pick == int(np.argmin(post))
        np.testing.assert_allclose(
            np.asarray(om @ np.diag(G[6:, 6:]) - rd.delta, dtype=np.float64), post, rtol=1e-12)


def test_tie_threshold_and_placed():
    S = np.diag([2.0, 3.0, 1e-9, 3.0])
    R = np.array([[1.0, 1.5, 1.0, 1.5], [0.5, 0.0, 2.0, 0.0]])
    for run in (X.reference_run, X.incremental_run):
        rd = run(S, R, 2)
        assert [r.pick for r in rd] == [1, 3]           # the tie goes to the lower index
        assert rd[0].delta[2] == 0.0                    # below the threshold
    S, R = X.fixture("X3")
    free = X.incremental_run(S, R, 8)
    cont = X.incremental_run(S, R, 4, placed=[r.pick for r in free[:4]])
    assert [r.pick for r in cont] == [r.pick for r in free]
    np.testing.assert_allclose([r.pick_delta for r in cont[4:]],
                               [r.pick_delta for r in free[4:]], rtol=1e-9)
