"""GPU: the field reconstruction from placed sensors on a factored covariance (vgposp_fpost_*
through placement_criteria.FieldReconstruction) against the longdouble reference of
tests/numpy_factor_post.py on Sigma = F F^T + diag(noise), with F the factor read back from the
device.

Errors: the variance as |dvar_i| / dg_i, the mean as |dmean_ib| / (|mu_i| + sum_j |c_ij alpha_jb|)
with the denominator from the reference.  The tolerance is
greedy_state_reference.tolerance(max(e_cpu, floor)) = 16 max(e_cpu, floor): e_cpu the error of the
float64 numpy restatement on the same factor, sensors and readings (at most 2.1e-15 on the
numpy-centred fixtures, tests/test_factor_post_reference.py), floor =
numpy_factor_post.error_floor(S, k) = (ceil(S / 4) + ceil(k / 16) + 12) eps."""
import json
import os

import numpy as np
import pytest

from tests import numpy_factor_cov as FC
from tests import numpy_factor_mi as FM
from tests import numpy_factor_post as FP
from tests.greedy_state_reference import require_longdouble, tolerance

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "factor_post_sensors.json")
EDGES = FP.edge_shapes()


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def PC():
    from vgposp_amd import placement_criteria
    return placement_criteria


_dev = {}


def _host(t):
    return t.cpu().numpy().copy()


def _fixture(PC, fx):
    """(FactoredCovariance from the samples, its factor read back, noise, the longdouble Sigma of
    it, the fixture's sensors), built once per process and never written."""
    if fx not in _dev:
        name, S, rel = fx
        T, noise = (a.copy() for a in FC.sample_fixture(name, S, noise_rel=rel))
        fac = PC.FactoredCovariance.from_samples(T, noise=noise)
        F = _host(fac.F)
        with open(GOLDEN) as f:
            sensors = json.load(f)[FP.fixture_id(fx)]
        _dev[fx] = fac, F, noise, FP.sigma_ld(F, noise, fx + ("device",)), sensors
    return _dev[fx]


def _compare(PC, fac, F, noise, sensors, s2, Y, mu, Sigma, label, modes=("var", "mean", "both")):
    """Variance only, mean only and both in one pass, each within the tolerance; the sensor rows;
    info 0.  Returns the FieldReconstruction."""
    S, k = F.shape[1], len(sensors)
    ref = FP.Reference(Sigma, sensors, s2, Y, mu)
    cpu = FP.FactorPost(F, noise, sensors, s2)
    e_cpu = max(FP.errors(ref, cpu.variance(), None if Y is None else cpu.mean(Y, mu)).values())
    tol = tolerance(max(e_cpu, FP.error_floor(S, k)))
    B = 0 if Y is None else Y.shape[1]
    rec = PC.FieldReconstruction(fac, sensors, obs_noise=s2, max_readings=max(B, 1))
    got = {}
    if "var" in modes:
        got["var"] = {"var": _host(rec.variance())}
    if Y is not None and "mean" in modes:
        got["mean"] = {"mean": _host(rec.mean(Y, mean=mu))}
    if Y is not None and "both" in modes:
        m, v = rec.mean_and_variance(Y, mean=mu)
        got["both"] = {"var": _host(v), "mean": _host(m)}
    sens = np.asarray(sensors)
    for mode, out in got.items():
        e = FP.errors(ref, out.get("var"), out.get("mean"))
        print(f"factor post {label} [{mode}]: e_cpu {e_cpu:.1e}, tolerance {tol:.1e}, device "
              + " ".join(f"{key} {v:.1e}" for key, v in e.items()))
        for key, v in e.items():
            assert v <= tol, (mode, key, v, tol)
        if s2 == 0.0 and (noise is not None or k <= S):
            # the sensors see themselves exactly
            if "var" in out:
                assert np.max(np.abs(out["var"][sens]) / cpu.dg[sens]) <= tol, mode
            if "mean" in out:
                scale = np.asarray(ref.scale[sens], dtype=np.float64)
                assert np.max(np.abs(out["mean"].reshape(len(F), -1)[sens] - Y) / scale) <= tol, \
                    mode
    if "both" in got and "var" in got:
        assert np.array_equal(got["both"]["var"], got["var"]["var"])      # the same arithmetic
    assert int(rec.info[0]) == 0
    rec.check()
    return rec


@pytest.mark.parametrize("fx", FP.FIXTURES, ids=[FP.fixture_id(f) for f in FP.FIXTURES])
def test_fixtures(PC, fx):
    """k = 16, B = 3, with and without a prior mean, at obs_noise = 0 and 1e-2 of the mean
    diagonal."""
    require_longdouble()
    assert len(FP.FIXTURES) == 12
    fac, F, noise, Sigma, sensors = _fixture(PC, fx)
    assert len(sensors) == FP.K_SENSORS
    before = _host(fac.F).tobytes(), _host(fac.noise).tobytes()
    for rel in FP.OBS_NOISE_REL:
        s2 = FP.obs_noise_of(F, noise, rel)
        for mu in (None, FP.prior_mean(len(F))):
            Y = FP.readings(F, noise, sensors, mu=mu)
            assert Y.shape == (16, 3)
            _compare(PC, fac, F, noise, sensors, s2, Y, mu, Sigma,
                     f"{FP.fixture_id(fx)} obs {rel:g} mu {mu is not None}")
    assert (_host(fac.F).tobytes(), _host(fac.noise).tobytes()) == before       # only read


@pytest.mark.parametrize("fx", [FP.FIXTURES[0], FP.FIXTURES[9]],
                         ids=[FP.fixture_id(FP.FIXTURES[0]), FP.fixture_id(FP.FIXTURES[9])])
def test_against_the_variance_criterion_rounds(PC, fx):
    """The library's own second route: the nom of CriterionPlacement's forced rounds on the same
    sensors is the posterior variance."""
    require_longdouble()
    fac, F, noise, Sigma, sensors = _fixture(PC, fx)
    ref = FP.Reference(Sigma, sensors, 0.0)
    cpu = FP.FactorPost(F, noise, sensors, 0.0)
    tol = tolerance(max(FP.errors(ref, cpu.variance())["var"],
                        FP.error_floor(F.shape[1], len(sensors))))
    g = PC.CriterionPlacement(fac, 1, "variance", placed=sensors).init()
    nom = _host(g.state()["nom"])
    var = _host(PC.FieldReconstruction(fac, sensors).variance())
    err = float(np.max(np.abs(var - nom) / cpu.dg))
    print(f"factor post {FP.fixture_id(fx)}: |variance - nom| / dg {err:.1e}, tolerance {tol:.1e}")
    assert err <= tol


@pytest.mark.parametrize("n,S,k,B", EDGES, ids=[f"n{n}-S{S}-k{k}-B{B}" for n, S, k, B in EDGES])
def test_edge_shapes(PC, n, S, k, B):
    """n around a 16-row block, a wave's 32 rows and a workgroup's 128; S around a pair, the
    K-tile of 32 and the largest; k and B around a 16-column fragment and the 64-column panel;
    variance only, mean only and both."""
    require_longdouble()
    F, noise, sensors, Y, mu = FP.edge_case(n, S, k, B)
    fac = PC.FactoredCovariance(F, noise=noise)
    _compare(PC, fac, F, noise, sensors, 0.0, Y, mu, FC.factor_cov_ld(F, noise),
             f"edge n={n} S={S} k={k} B={B}")


@pytest.mark.parametrize("fx,pad,shift", [(FP.FIXTURES[2], 3, 0), (FP.FIXTURES[2], 2, 1),
                                           (FP.FIXTURES[6], 1, 0)],
                         ids=["S96-odd-pitch", "S96-even-pitch-off-16-bytes", "S75-even-pitch"])
def test_a_pitched_factor(PC, fx, pad, shift):
    """F as a view of a wider buffer, NaN in the padding: an odd pitch and an even pitch that
    starts 8 bytes off a 16-byte boundary take the 8-byte loads; S = 75 at the aligned pitch 76
    takes the 16-byte loads with a lone last column."""
    import torch
    require_longdouble()
    fac, F, noise, Sigma, sensors = _fixture(PC, fx)
    n, S = F.shape
    ld = S + pad
    flat = torch.full((n * ld + 2,), float("nan"), dtype=torch.float64, device="cuda")
    view = flat[shift:shift + n * ld].view(n, ld)[:, :S]
    view.copy_(fac.F)
    pit = PC.FactoredCovariance(view, noise=noise)
    assert pit.F.data_ptr() == flat.data_ptr() + 8 * shift and pit.args()[3] == ld
    vec = pit.F.data_ptr() % 16 == 0 and ld % 2 == 0
    assert vec == (fx[1] == 75)
    mu = FP.prior_mean(n)
    Y = FP.readings(F, noise, sensors, mu=mu)
    _compare(PC, pit, F, noise, sensors, 0.0, Y, mu, Sigma, f"pitch {ld} shift {shift}")
    assert bool(torch.isnan(flat[-1]))


def test_sensors_at_the_first_and_last_rows_and_at_a_waves_last_row(PC):
    require_longdouble()
    n, S = 200, 75
    F, noise = FM.random_factor(n, S, 4242)
    sensors = [0, n - 1, 31, 127, 15, 16, 128]
    mu = FP.prior_mean(n)
    Y = FP.readings(F, noise, sensors, mu=mu)
    fac = PC.FactoredCovariance(F, noise=noise)
    _compare(PC, fac, F, noise, sensors, 0.0, Y, mu, FC.factor_cov_ld(F, noise), "row ends")


def test_no_noise_with_obs_noise(PC):
    """noise = None: G is positive definite through obs_noise alone, k > S included."""
    require_longdouble()
    for n, S, k, B in ((200, 75, 16, 3), (120, 5, 9, 2)):
        F, _, sensors, Y, mu = FP.edge_case(n, S, k, B, noise=False)
        fac = PC.FactoredCovariance(F)
        assert fac.noise is None
        s2 = FP.obs_noise_of(F, None, 1e-2)
        _compare(PC, fac, F, None, sensors, s2, Y, mu, FC.factor_cov_ld(F, None),
                 f"no noise n={n} S={S} k={k}")


def test_singular_sensors_are_reported_and_write_nothing(PC):
    """noise None, obs_noise 0 and two sensors whose rows of F are equal: info > 0, check()
    raises, and the outputs keep what they were filled with."""
    import torch
    from vgposp_amd import linalg
    F, _ = FM.random_factor(40, 4, 11)
    F[3] = F[7] = [2.0, 0.0, 0.0, 0.0]              # G = [[4, 4], [4, 4]]: the pivot is exactly 0
    fac = PC.FactoredCovariance(F)
    rec = PC.FieldReconstruction(fac, [3, 7])
    var = torch.full((40,), -7.0, dtype=torch.float64, device="cuda")
    out = torch.full((40, 2), -7.0, dtype=torch.float64, device="cuda")
    rec.variance(out=var)
    rec.mean(np.ones((2, 2)), out=out)
    assert int(rec.info[0]) > 0
    with pytest.raises(linalg.CholeskyError):
        rec.check()
    assert bool((var == -7.0).all()) and bool((out == -7.0).all())
    # the same sensors with an obs_noise are fine
    ok = PC.FieldReconstruction(fac, [3, 7], obs_noise=1e-3)
    ok.variance(out=var)
    ok.check()
    assert bool((var > -1e-12).all())


def test_repeatability(PC):
    """Two applies after one init, and a second FieldReconstruction on the same inputs, are
    bit-identical; F and noise are only read."""
    import torch
    fx = FP.FIXTURES[5]
    fac, F, noise, _, sensors = _fixture(PC, fx)
    before = _host(fac.F).tobytes(), _host(fac.noise).tobytes()
    mu = FP.prior_mean(len(F))
    Y = FP.readings(F, noise, sensors, B=70, mu=mu)
    a = PC.FieldReconstruction(fac, sensors, obs_noise=1e-3)
    v1, m1 = a.variance(), a.mean(Y, mean=mu)
    v2, m2 = a.variance(), a.mean(Y, mean=mu)
    b = PC.FieldReconstruction(fac, sensors, obs_noise=1e-3)
    m3, v3 = b.mean_and_variance(Y, mean=mu)
    for x, y in ((v1, v2), (m1, m2), (v1, v3), (m1, m3)):
        assert torch.equal(x, y)
    assert m1.shape == (len(F), 70) and a.mean(Y[:, 0], mean=mu).shape == (len(F),)
    # one slice of 128 columns and two of 64 + 6 are the same numbers up to the order in which
    # the small products behind alpha and Z sum (the prior mean is between 1 and 4)
    c = PC.FieldReconstruction(fac, sensors, obs_noise=1e-3, max_readings=128)
    assert torch.allclose(c.mean(Y, mean=mu), m1, rtol=1e-12, atol=1e-12)
    assert bool((a.stddev() >= 0).all())
    assert torch.equal(a.stddev(), v1.clamp(min=0).sqrt())
    assert (_host(fac.F).tobytes(), _host(fac.noise).tobytes()) == before


def test_reconstruct_from_samples(PC):
    from vgposp_amd.placement_algorithm2 import reconstruct_from_samples
    require_longdouble()
    fx = FP.FIXTURES[0]
    fac, F, noise, Sigma, sensors = _fixture(PC, fx)
    T = FC.sample_fixture(fx[0], fx[1], noise_rel=fx[2])[0].copy()
    mu = T.mean(axis=1)
    Y = FP.readings(F, noise, sensors, mu=mu)
    mean, var = reconstruct_from_samples(T, sensors, Y, noise=noise)
    ref = FP.Reference(Sigma, sensors, 0.0, Y, mu)
    cpu = FP.FactorPost(F, noise, sensors, 0.0)
    tol = tolerance(max(max(FP.errors(ref, cpu.variance(), cpu.mean(Y, mu)).values()),
                        FP.error_floor(F.shape[1], len(sensors))))
    e = FP.errors(ref, _host(var), _host(mean))
    assert max(e.values()) <= tol, (e, tol)
    one = reconstruct_from_samples(T, sensors, Y[:, 1], noise=noise)[0]
    assert one.shape == (len(F),)
    assert np.max(np.abs(_host(one) - ref.mean[:, 1]) / ref.scale[:, 1]) <= tol
