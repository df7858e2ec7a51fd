"""CPU: the conditions under which the GPU tests of a factored covariance (tests/
test_gpu_factor_criteria.py, tests/test_gpu_factor_symv.py) mean something, and the host layer's
argument errors.

* On the longdouble Sigma = F F^T + diag(noise) of every fixture the best and the second-best delta
  of every round are at least MIN_GAP apart, so a pick is decided by the arithmetic and not by
  rounding (smallest gap over the 24 combinations with the numpy-centred F: 9.0e-5).
* The float64 incremental form the kernels run gives the same picks.
* The moment-matrix identity of the squared pass equals (Sigma o Sigma) x.
* The factor ``FactoredCovariance.from_samples`` defines reproduces the oracle's empirical_cov.
"""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_cov as FC
from tests.greedy_state_reference import require_longdouble

CASES = [(fx, cfg, crit) for fx in FC.FIXTURES for cfg in FC.CONFIGS for crit in FC.CRITERIA]


def _factor(fx):
    name, S, rel = fx
    T, noise = FC.sample_fixture(name, S, noise_rel=rel)
    return FC.factor_of(T), noise


@pytest.mark.parametrize("fx,config,criterion", CASES,
                         ids=[f"{FC.fixture_id(f)}-{c}-{r}" for f, c, r in CASES])
def test_gaps_and_incremental_picks(fx, config, criterion):
    require_longdouble()
    assert len(CASES) == 24
    F, noise = _factor(fx)
    ref = FC.reference(F, noise, fx + ("numpy",), config, criterion)
    T, cand = C.config_masks(fx[0], config)
    gaps = C.round_gaps(ref, cand)
    print(f"{FC.fixture_id(fx)}-{config}-{criterion}: smallest gap "
          f"{min(g for g, _ in gaps):.1e}")
    assert len(gaps) == C.K_ROUNDS
    assert all(gap >= C.MIN_GAP and lowest for gap, lowest in gaps), gaps
    Sigma = np.asarray(FC.factor_cov_ld(F, noise), dtype=np.float64)
    inc = C.incremental_run(Sigma, criterion, C.K_ROUNDS, None if criterion == "entropy" else T,
                            cand)
    assert [r.pick for r in inc] == [r.pick for r in ref]


@pytest.mark.parametrize("fx", FC.FIXTURES, ids=[FC.fixture_id(f) for f in FC.FIXTURES])
def test_moment_matrix_identity(fx):
    """fsymv_ld never forms Sigma; against the products with the formed matrix, both passes."""
    require_longdouble()
    F, noise = _factor(fx)
    n, S = F.shape
    rng = np.random.default_rng(3)
    x = rng.standard_normal(n)
    x[rng.permutation(n) < n // 3] = 0.0
    Sigma = FC.factor_cov_ld(F, noise)
    xl = x.astype(FC.LD)
    for squared, direct in ((False, Sigma @ xl), (True, (Sigma * Sigma) @ xl)):
        want, weight = FC.fsymv_ld(F, noise, x, squared)
        assert (weight > 0).all()
        err = float(np.max(np.abs(want - direct) / weight))
        print(f"{FC.fixture_id(fx)} squared={squared}: {err:.1e} of the weight")
        # both sides are longdouble: far inside the float64 bound the GPU test uses
        assert err <= FC.fsymv_bound(n, S, squared)
        assert err <= 1e3 * float(np.finfo(FC.LD).eps) * (n + 2 * S)


def test_samples_are_centred_and_the_factor_is_the_empirical_covariance():
    from oracle import covariance as ocov
    for tr_stdev in (1.0, 2.5):
        T, _ = FC.sample_fixture("F2", 75)
        assert abs(float(T.mean()) - 3.0) < 0.5                      # the mean the centring removes
        F = FC.factor_of(T, tr_stdev)
        assert np.max(np.abs(F.sum(axis=1))) < 1e-12
        want = ocov.empirical_cov(T, tr_stdev=tr_stdev)
        got = F @ F.T
        assert np.max(np.abs(got - want)) <= 1e-13 * float(np.max(np.diag(want)))
        assert np.max(np.abs(got - np.cov(T / tr_stdev, bias=True))) \
            <= 1e-13 * float(np.max(np.diag(want)))


def test_host_layer_argument_errors():
    """Raised before any device work: no GPU is needed."""
    from vgposp_amd import placement_criteria as PC
    from vgposp_amd.placement_algorithm2 import placement_from_samples
    F = np.random.default_rng(0).standard_normal((20, 6))
    fac = PC.FactoredCovariance(F, noise=0.1)
    assert (fac.N, fac.S) == (20, 6)
    for kw in (dict(diag=np.ones(20)), dict(cross_cov=np.ones((5, 20))),
               dict(cross_kernel=object())):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=f"{name} and a FactoredCovariance exclude"):
            PC.CriterionPlacement(fac, 3, **kw)
    with pytest.raises(ValueError, match="FactoredCovariance exclude"):
        PC.placement_variance_reduction(fac, 3, cross_cov=np.ones((5, 20)))
    with pytest.raises(ValueError, match="FactoredCovariance exclude"):
        PC.placement_variance_reduction(fac, 0, cross_kernel=object())
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="noise must be finite and not negative"):
            PC.FactoredCovariance(F, noise=bad)
        v = np.zeros(20)
        v[7] = bad
        with pytest.raises(ValueError, match="noise must be finite and not negative"):
            PC.FactoredCovariance(F, noise=v)
        with pytest.raises(ValueError, match="noise must be finite and not negative"):
            placement_from_samples(F, 3, noise=bad)
    with pytest.raises(ValueError, match="noise must have length 20"):
        PC.FactoredCovariance(F, noise=np.ones(19))
    with pytest.raises(ValueError, match=r"F must be \[N, S\]"):
        PC.FactoredCovariance(np.ones(5))
    with pytest.raises(ValueError, match="1 <= S <= 4096"):
        PC.FactoredCovariance(np.ones((3, 4097)))
    with pytest.raises(ValueError, match="1 <= S <= 4096"):
        PC.FactoredCovariance(np.ones((3, 0)))
    with pytest.raises(ValueError, match="mutual-information placement factors"):
        placement_from_samples(F, 3, criterion="mi", cov="factored")
    with pytest.raises(ValueError, match="mutual-information placement factors"):
        placement_from_samples(F, 3, criterion="mi")                 # factored is the default
    with pytest.raises(ValueError, match="unknown cov"):
        placement_from_samples(F, 3, cov="matrix_free")
    with pytest.raises(ValueError, match="unknown criterion"):
        placement_from_samples(F, 3, criterion="trace")
    with pytest.raises(ValueError, match="tr_stdev must be a finite, positive scalar"):
        placement_from_samples(F, 3, tr_stdev=0.0)
    with pytest.raises(ValueError, match=r"samples must be \[N, S\]"):
        placement_from_samples(np.ones(7), 3)
