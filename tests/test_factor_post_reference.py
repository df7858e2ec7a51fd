"""CPU: what the GPU tests of the field reconstruction on a factored covariance
(tests/test_gpu_factor_post.py) take their tolerance from, the identities that tie it to the
variance-criterion rounds, and the host layer's argument errors.

On every fixture (numpy_factor_post.FIXTURES: F1 / F2, S = 75, 96, 300, noise 1e-2 and 1e-3 of the
nugget) with the first 16 mutual-information picks of the longdouble reference as sensors, at
obs_noise = 0 and 1e-2 of the mean diagonal, with and without a prior mean: the float64
restatement (tests/numpy_factor_post.py, the arithmetic of csrc/criteria.hip's vgposp_fpost_*)
against the longdouble reference on the assembled Sigma.  Its worst error e_cpu is printed and
passes greedy_state_reference.tolerance (16 e_cpu <= 1e-11)."""
import json
import os

import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_cov as FC
from tests import numpy_factor_mi as FM
from tests import numpy_factor_post as FP
from tests.greedy_state_reference import LD, require_longdouble, tolerance

IDS = [FP.fixture_id(f) for f in FP.FIXTURES]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "factor_post_sensors.json")


def _case(fx):
    F, noise = FP.fixture_factor(fx)
    return F, noise, FP.fixture_sensors(fx, F, noise), FP.sigma_ld(F, noise, fx + ("numpy",))


@pytest.mark.parametrize("fx", FP.FIXTURES, ids=IDS)
def test_restatement_error(fx):
    require_longdouble()
    assert len(FP.FIXTURES) == 12
    F, noise, sensors, Sigma = _case(fx)
    n = len(F)
    worst = 0.0
    for rel in FP.OBS_NOISE_REL:
        s2 = FP.obs_noise_of(F, noise, rel)
        for mu in (None, FP.prior_mean(n)):
            Y = FP.readings(F, noise, sensors, mu=mu)
            ref = FP.Reference(Sigma, sensors, s2, Y, mu)
            g = FP.FactorPost(F, noise, sensors, s2)
            e = FP.errors(ref, g.variance(), g.mean(Y, mu))
            worst = max(worst, e["var"], e["mean"])
            rest = np.setdiff1d(np.arange(n), sensors)
            assert float(np.min(ref.var[rest])) > 0.0 and float(np.min(ref.dg - ref.var)) >= 0.0
    print(f"factor post {FP.fixture_id(fx)}: e_cpu {worst:.1e}, floor "
          f"{FP.error_floor(fx[1], FP.K_SENSORS):.1e}")
    tolerance(worst)                                    # 16 e_cpu <= 1e-11


@pytest.mark.parametrize("fx", FP.FIXTURES, ids=IDS)
def test_identities(fx):
    """At obs_noise = 0: a sensor's own variance is 0 and the mean there is the reading; the
    variance is the nom of a forced variance-criterion run on the same sensors, and what it took
    off the prior is the sum of that run's deltas."""
    require_longdouble()
    F, noise, sensors, Sigma = _case(fx)
    n = len(F)
    mu = FP.prior_mean(n)
    Y = FP.readings(F, noise, sensors, mu=mu)
    g = FP.FactorPost(F, noise, sensors, 0.0)
    var, mean = g.variance(), g.mean(Y, mu)
    ref = FP.Reference(Sigma, sensors, 0.0, Y, mu)
    tol = tolerance(max(max(FP.errors(ref, var, mean).values()),
                        FP.error_floor(fx[1], FP.K_SENSORS)))
    assert np.max(np.abs(var[sensors]) / g.dg[sensors]) <= tol
    assert np.max(np.abs(mean[sensors] - Y) / np.asarray(ref.scale[sensors], dtype=np.float64)) \
        <= tol
    assert float(np.max(np.abs(ref.var[sensors]) / ref.dg[sensors])) <= 1e-15
    rounds = C.reference_run(Sigma, "variance", 0, placed=sensors)
    nom = rounds[-1].nom
    assert float(np.max(np.abs(ref.var - nom) / ref.dg)) <= 1e-15
    assert np.max(np.abs(var.astype(LD) - nom) / ref.dg) <= tol
    removed = sum(r.pick_delta for r in rounds)
    assert abs(float((np.sum(ref.dg - ref.var) - removed) / removed)) <= 1e-15
    assert abs(float((np.sum((g.dg - var).astype(LD)) - removed) / removed)) <= tol


def test_sensors_are_the_recorded_ones():
    """tests/golden/factor_post_sensors.json holds the sensors of every fixture, so that the GPU
    tests need no n x n longdouble factorization to choose them: they are the first 16 picks of
    numpy_factor_mi.reference_picks."""
    require_longdouble()
    with open(GOLDEN) as f:
        recorded = json.load(f)
    assert sorted(recorded) == sorted(IDS)
    for fx in FP.FIXTURES:
        F, noise = FP.fixture_factor(fx)
        assert recorded[FP.fixture_id(fx)] == FP.fixture_sensors(fx, F, noise), fx


def test_edge_shapes_restatement():
    """The edge shapes of the GPU test are well-posed: the restatement agrees with the reference
    inside the tolerance the device is held to (shapes whose S the longdouble products make slow
    are left to the GPU test)."""
    require_longdouble()
    shapes = [s for s in FP.edge_shapes() if s[1] <= 300]
    assert len(shapes) == len(FP.edge_shapes()) - 1
    for n, S, k, B in shapes:
        F, noise, sensors, Y, mu = FP.edge_case(n, S, k, B)
        ref = FP.Reference(FC.factor_cov_ld(F, noise), sensors, 0.0, Y, mu)
        g = FP.FactorPost(F, noise, sensors, 0.0)
        e = FP.errors(ref, g.variance(), g.mean(Y, mu) if B else None)
        tolerance(max(max(e.values()), FP.error_floor(S, k)))


def test_singular_sensors_raise_in_the_restatement():
    F, _ = FM.random_factor(40, 5, 11)
    F[7] = F[3]
    with pytest.raises(np.linalg.LinAlgError):
        FP.FactorPost(F, None, [3, 7], 0.0)
    FP.FactorPost(F, None, [3, 7], 1e-3)


# ---- the host layer's errors, all before any device work ----
@pytest.fixture(scope="module")
def PC():
    from vgposp_amd import placement_criteria
    return placement_criteria


def _fac(PC, n=30, S=6, noise=0.1):
    return PC.FactoredCovariance(np.random.default_rng(0).standard_normal((n, S)), noise)


def test_host_layer_argument_errors(PC):
    fac = _fac(PC)
    R = PC.FieldReconstruction
    with pytest.raises(ValueError, match="FactoredCovariance"):
        R(np.eye(4), [0, 1])
    with pytest.raises(ValueError, match="more than once"):
        R(fac, [1, 2, 1])
    with pytest.raises(ValueError, match="outside"):
        R(fac, [1, 30])
    with pytest.raises(ValueError, match="outside"):
        R(fac, [-1, 3])
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        R(fac, [])
    big = PC.FactoredCovariance(np.zeros((1100, 2)), 0.1)
    with pytest.raises(ValueError, match=r"\[1, 1024\]"):
        R(big, np.arange(1025))
    for bad in (-1e-3, float("nan"), float("inf"), [0.1]):
        with pytest.raises(ValueError, match="obs_noise"):
            R(fac, [0, 1], obs_noise=bad)
    with pytest.raises(ValueError, match="max_readings"):
        R(fac, [0, 1], max_readings=0)
    # zero noise and obs_noise = 0: k <= S
    bare = _fac(PC, noise=0.0)
    with pytest.raises(ValueError, match="singular"):
        R(bare, np.arange(7))
    R(bare, np.arange(6))
    R(bare, np.arange(7), obs_noise=1e-3)
    R(fac, np.arange(7))
    rec = R(fac, [4, 9, 2])
    for bad in (np.zeros(2), np.zeros((2, 3)), np.zeros((3, 2, 1)), np.zeros(())):
        with pytest.raises(ValueError, match="readings"):
            rec.mean(bad)
    with pytest.raises(ValueError, match="mean must have length"):
        rec.mean(np.zeros(3), mean=np.zeros(5))
    assert fac._uploaded is False and rec._ready is False      # nothing touched a device


def test_reconstruct_from_samples_argument_errors(PC):
    from vgposp_amd import placement_algorithm2 as pa2
    assert pa2.reconstruct_from_samples.__doc__ and pa2.placement_from_samples
    T = np.random.default_rng(1).standard_normal((20, 5))
    for f in (PC.reconstruct_from_samples, pa2.reconstruct_from_samples):
        with pytest.raises(ValueError, match="samples"):
            f(T[0], [0], [1.0])
        with pytest.raises(ValueError, match="more than once"):
            f(T, [3, 3], [1.0, 2.0])
        with pytest.raises(ValueError, match="outside"):
            f(T, [20], [1.0])
