"""CPU: the longdouble generated covariance of tests/numpy_site_kernel.py against the fixtures of
tests/numpy_criteria_greedy.py it restates, and the conditions under which the references of those
fixtures serve tests/test_gpu_site_kernel_criteria.py.

F1 and F2 are D (K + 1e-2 I) D with D = diag(a): as a generated covariance, scale = a and
diag = 1.01 a^2.  The matrices agree to 1e-13 relative, so the longdouble rounds of the fixtures are
the rounds of the generated matrix as long as every round's best and second-best delta are at
least 1e-6 apart, which is asserted here on the generated matrix itself."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_kernel_cross as K
from tests import numpy_site_kernel as SK
from tests.greedy_state_reference import require_longdouble

CONFIGS = [(f, c, "variance") for f in ("F1", "F2") for c in ("plain", "random", "oddeven")] \
    + [(f, "plain", "entropy") for f in ("F1", "F2")]


@pytest.mark.parametrize("name", ["F1", "F2"])
def test_generated_fixture_equals_the_assembled_one(name):
    require_longdouble()
    want = C.fixture_cov(name)
    got = SK.site_cov_ld(*SK.fixture_site(name))
    rel = float(np.max(np.abs(got - want.astype(C.LD)) / np.abs(want)))
    print(f"{name}: generated against assembled, worst relative difference {rel:.1e}")
    assert got.shape == want.shape and rel <= 1e-13
    assert np.array_equal(got, got.T)


def test_definition_of_the_diagonal_and_of_coincident_points():
    X = np.random.default_rng(0).random((7, 3))
    X[5] = X[2]
    a = np.random.default_rng(1).uniform(0.5, 2.0, 7)
    S = SK.site_cov_ld("matern32", X, 1.3, 0.6, a)
    assert np.allclose(np.diag(S).astype(np.float64), a * a * 1.69, rtol=1e-15)
    assert abs(float(S[2, 5]) - a[2] * a[5] * 1.69) <= 1e-15 * 8     # not the diagonal
    dg = np.arange(1.0, 8.0)
    S = SK.site_cov_ld("eq", X, 1.3, 0.6, a, dg)
    assert np.array_equal(np.diag(S).astype(np.float64), dg)
    plain = K.kernel_ld("eq", X, X, 1.3, 0.6)
    off = ~np.eye(7, dtype=bool)
    al = a.astype(C.LD)
    assert np.array_equal(S[off], (plain * (al[:, None] * al[None, :]))[off])
    want, weight = SK.symv_ld(S, np.ones(7), squared=True)
    assert np.allclose((S * S).sum(1).astype(np.float64), want.astype(np.float64), rtol=1e-15)
    assert (SK.symv_bound(7, weight, True) > SK.symv_bound(7, weight, False)).all()


@pytest.mark.parametrize("name,config,criterion", CONFIGS, ids=["-".join(c) for c in CONFIGS])
def test_rounds_and_gaps_on_the_generated_matrix(name, config, criterion):
    """The rounds of the generated matrix pick what the fixture's reference picks, and their gaps
    are at least MIN_GAP (measured: >= 3.7e-4 for variance, >= 1.7e-5 for entropy)."""
    require_longdouble()
    T, cand = C.config_masks(name, config)
    T = None if criterion == "entropy" else T
    rounds = C.reference_run(SK.fixture_cov(name), criterion, C.K_ROUNDS, T, cand)
    ref = C.reference(name, config, criterion)
    assert [r.pick for r in rounds] == [r.pick for r in ref]
    gaps = C.round_gaps(rounds, cand)
    print(f"{name}-{config}-{criterion}: smallest gap {min(g for g, _ in gaps):.1e}")
    assert all(g >= C.MIN_GAP and lowest for g, lowest in gaps)
    scale = max(float(r.pick_delta) for r in ref)
    assert max(float(np.max(np.abs(a.delta - b.delta))) for a, b in zip(rounds, ref)) \
        <= 1e-11 * scale
