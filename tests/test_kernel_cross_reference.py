"""CPU: the longdouble kernels of tests/numpy_kernel_cross.py against the float64 oracle, against
the fixtures the matrix-free rounds are judged on, and the conditions the inputs of
tests/test_gpu_matrix_free_criteria.py must meet."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_cross_criteria as X
from tests import numpy_kernel_cross as K
from tests.greedy_state_reference import require_longdouble


@pytest.mark.parametrize("d", [1, 3, 5, 8])
@pytest.mark.parametrize("kind", K.KINDS)
def test_longdouble_kernels_against_the_oracle(kind, d):
    from oracle import gp as ogp
    rng = np.random.default_rng(10 * d + len(kind))
    Xt, Xs = rng.random((37, d)), rng.random((29, d))
    Xt[:5] = Xs[:5]                      # r = 0
    amp, ls = 1.3, float(rng.uniform(0.3, 1.0))
    got = K.kernel_ld(kind, Xt, Xs, amp, ls)
    want = ogp.kernel_matrix(kind, Xt, Xs, amp, ls)[0]
    err = float(np.max(np.abs(got - want) / want))
    print(f"{kind} d {d}: longdouble kernel against the oracle {err:.2e}")
    assert err <= 1e-13
    np.testing.assert_allclose(np.asarray(np.diag(got[:5, :5]), dtype=np.float64), amp * amp,
                               rtol=1e-15)


def test_one_dimensional_points_as_vectors():
    x, y = np.linspace(0, 1, 7), np.linspace(0, 1, 5)
    a = K.kernel_ld("matern52", x, y, 1.0, 0.4)
    b = K.kernel_ld("matern52", x[:, None], y[:, None], 1.0, 0.4)
    assert a.shape == (7, 5) and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(X.FIXTURES))
def test_fixture_points_reproduce_the_fixtures_cross_covariance(name):
    """diag(a_t) K diag(a_s) from the fixture's points is the R the references of
    tests/numpy_cross_criteria.py run on: what lets the matrix-free rounds reuse them."""
    _, R = X.fixture(name)
    kind, Xs, Xt, amp, ls, a_s, a_t = K.fixture_points(name)
    got = K.cross_ld(kind, Xt, Xs, amp, ls, a_t, a_s)
    assert got.shape == R.shape
    err = float(np.max(np.abs(got - R) / R))
    print(f"{name}: generated R against joint_cov {err:.2e}")
    assert err <= 1e-13
    # three or four 512-target chunks with a ragged tail
    P = R.shape[0]
    assert -(-P // 512) >= 3 and P % 512 != 0


def test_gemv_t_reference_and_bound():
    rng = np.random.default_rng(0)
    R = K.cross_ld("eq", rng.random((50, 2)), rng.random((7, 2)), 1.1, 0.5,
                   rng.uniform(1, 2, 50), rng.uniform(1, 2, 7))
    x = rng.standard_normal(50)
    x[::3] = 0.0
    for sq in (False, True):
        want, weight = K.gemv_t_ld(R, x, sq)
        M = np.asarray(R, dtype=np.float64) ** (2 if sq else 1)
        assert (np.abs(M.T @ x - want) <= K.gemv_t_bound(50, weight, sq)).all()
        assert (weight >= np.abs(want)).all()
    assert (K.gemv_t_bound(50, weight, True) > K.gemv_t_bound(50, weight, False)).all()


def test_five_dimensional_case_gap_and_restatement():
    """The 3^5 sites / 4^5 targets case: every round's best and second-best delta differ by
    >= 1e-6 relative, and the float64 restatement of the algorithm gives the reference's picks."""
    require_longdouble()
    (Xs, Xt, ls, S, R), ref = K.d5_reference()
    assert Xs.shape == (243, 5) and Xt.shape == (1024, 5) and len(ref) == K.D5_K
    gaps = C.round_gaps(ref, None)
    assert all(low for _, low in gaps)
    print(f"5-D case: smallest gap {min(g for g, _ in gaps):.2e}")
    assert min(g for g, _ in gaps) >= X.MIN_GAP
    inc = X.incremental_run(S, R, K.D5_K)
    assert [r.pick for r in inc] == [r.pick for r in ref]
    assert np.array_equal(S, S.T)
