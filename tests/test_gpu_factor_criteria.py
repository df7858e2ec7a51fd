"""GPU: the variance-reduction and entropy placements on a covariance given by a factor (the
vgposp_critf_* entries through placement_criteria.FactoredCovariance) against the longdouble rounds
of tests/numpy_criteria_greedy.py on Sigma = F F^T + diag(noise), with F the factor read back from
the object: what the device centred is what the reference runs on (tests/
test_factor_cov_reference.py shows on the CPU that the rounds' gaps hold for these fixtures).

Tolerance 1e-9 (the project's tolerance for deltas): delta and s relative to the round's pick
delta, nom and the new row of W relative to max diag Sigma.  F1 (n = 1,320) spans six 256-row
workgroups, F2 (n = 819) four, both with a ragged last one; S = 75 takes the 8-byte loads."""
import os

import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_cov as FC
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu
TOL = C.STATE_TOL
CASES = [(fx, cfg, crit) for fx in FC.FIXTURES for cfg in FC.CONFIGS for crit in FC.CRITERIA]


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
    """(FactoredCovariance, its factor on the host, noise, the dense Sigma on the device), built
    once and never written."""
    import torch
    from vgposp_amd.covariance import empirical_cov
    if fx not in _dev:
        name, S, rel = fx
        T, noise = (a.copy() for a in FC.sample_fixture(name, S, noise_rel=rel))
        fac = PC.FactoredCovariance.from_samples(T, noise=noise)
        assert (fac.N, fac.S) == T.shape and (fac.noise is None) == (rel == 0.0)
        Sigma = empirical_cov(T)
        torch.diagonal(Sigma).add_(torch.as_tensor(noise, device="cuda"))
        _dev[fx] = fac, _host(fac.F), noise, Sigma
    return _dev[fx]


def test_from_samples_is_the_empirical_covariance(PC):
    """F F^T of the centred copy equals covariance.empirical_cov and numpy's biased covariance;
    the mean 3.0 of the samples is gone; tr_stdev scales it."""
    from vgposp_amd.covariance import empirical_cov
    T = FC.sample_fixture("F2", 75)[0].copy()
    for tr_stdev in (1.0, 2.5):
        fac = PC.FactoredCovariance.from_samples(T, tr_stdev=tr_stdev)
        F = _host(fac.F)
        assert np.max(np.abs(F.sum(axis=1))) < 1e-12
        want = np.cov(T / tr_stdev, bias=True)
        smax = float(np.max(np.diag(want)))
        assert np.max(np.abs(F @ F.T - want)) <= 1e-13 * smax
        assert np.max(np.abs(_host(empirical_cov(T, tr_stdev=tr_stdev)) - want)) <= 1e-13 * smax
        assert np.max(np.abs(F - FC.factor_of(T, tr_stdev))) <= 1e-14


@pytest.mark.parametrize("fx,config,criterion", CASES,
                         ids=[f"{FC.fixture_id(f)}-{c}-{r}" for f, c, r in CASES])
def test_picks_and_state(PC, fx, config, criterion):
    """Every round of the reference: the pick, then the whole state; beside it the dense run on
    empirical_cov(samples) + diag(noise), whose picks are the same and whose deltas lie within
    1e-9."""
    require_longdouble()
    fac, F, noise, Sigma = _fixture(PC, fx)
    before = _host(fac.F).tobytes(), (None if fac.noise is None else _host(fac.noise).tobytes())
    T, cand = C.config_masks(fx[0], config)
    T = None if criterion == "entropy" else T
    ref = FC.reference(F, noise, fx + ("device",), config, criterion)
    gaps = C.round_gaps(ref, cand)
    assert all(gap >= C.MIN_GAP and lowest for gap, lowest in gaps), gaps
    g = PC.CriterionPlacement(fac, C.K_ROUNDS, criterion, candidates=cand, targets=T).init()
    dense = PC.CriterionPlacement(Sigma, C.K_ROUNDS, criterion, candidates=cand, targets=T).init()
    smax = float(np.max(np.sum(F * F, axis=1) + noise))
    worst = {"delta": 0.0, "s": 0.0, "nom": 0.0, "W": 0.0, "dense": 0.0}
    for r, want in enumerate(ref):
        g.step()
        dense.step()
        st = g.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        assert int(dense.selected[r]) == want.pick, r
        scale = float(want.pick_delta)
        err = {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
               "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
               "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax,
               "dense": abs(float(g.sel_delta[r]) - float(dense.sel_delta[r])) / scale}
        if criterion == "variance":
            err["s"] = np.max(np.abs(_host(st["s"]) - want.s)) / scale
        for key, e in err.items():
            worst[key] = max(worst[key], float(e))
        assert abs(float(g.sel_delta[r]) - scale) <= TOL * scale, r
    print(f"factored criteria {FC.fixture_id(fx)}-{config}-{criterion}: "
          + " ".join(f"{key} {v:.1e}" for key, v in worst.items())
          + f", smallest gap {min(gap for gap, _ in gaps):.1e}")
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert [int(p) for p in dense.result()[0]] == [int(p) for p in picks]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (C.K_ROUNDS,)
    if cand is not None:
        assert cand[picks].all()
    assert g.state()["W"].shape == (C.K_ROUNDS, fac.N)
    assert _host(fac.F).tobytes() == before[0]                        # the factor is only read
    assert (None if fac.noise is None else _host(fac.noise).tobytes()) == before[1]


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_placed_continues_a_free_run(PC, criterion):
    fac, F, noise, _ = _fixture(PC, FC.FIXTURES[0])
    picks, deltas = PC.CriterionPlacement(fac, 8, criterion).run().result()
    ref = FC.reference(F, noise, FC.FIXTURES[0] + ("device",), "plain", criterion)
    assert [int(p) for p in picks] == [w.pick for w in ref[:8]]
    g = PC.CriterionPlacement(fac, 4, criterion, placed=picks[:4]).run()
    more, dmore = g.result()
    assert [int(p) for p in more] == [int(p) for p in picks[4:]]
    np.testing.assert_allclose(dmore, deltas[4:], rtol=TOL, atol=0)
    assert g.state()["W"].shape == (8, fac.N)


def test_two_runs_are_bit_identical(PC):
    fac = _fixture(PC, FC.FIXTURES[2])[0]
    a = PC.CriterionPlacement(fac, 6, "variance").run()
    b = PC.CriterionPlacement(fac, 6, "variance").run()
    assert _host(a.sel_delta).tobytes() == _host(b.sel_delta).tobytes()
    for key in ("nom", "s", "delta", "W"):
        assert _host(a.state()[key]).tobytes() == _host(b.state()[key]).tobytes(), key


@pytest.mark.parametrize("fx", [FC.FIXTURES[0], FC.FIXTURES[2]],
                         ids=[FC.fixture_id(FC.FIXTURES[0]), FC.fixture_id(FC.FIXTURES[2])])
def test_a_pitched_factor_gives_the_same_state(PC, fx):
    """F as a view of a wider buffer (pitch S + 3, NaN in the padding): the same picks, the state
    within 1e-9 of the contiguous run (S = 96 moves to the 8-byte loads, S = 75 to the 16-byte
    ones, which add in the same order)."""
    import torch
    fac, F, noise, _ = _fixture(PC, fx)
    n, S = F.shape
    base = torch.full((n, S + 3), float("nan"), dtype=torch.float64, device="cuda")
    base[:, :S] = fac.F
    view = base[:, :S]
    pit = PC.FactoredCovariance(view, noise=noise)
    assert pit.F.data_ptr() == base.data_ptr() and pit.args()[3] == S + 3   # used where it lies
    a = PC.CriterionPlacement(fac, 6, "variance").run()
    b = PC.CriterionPlacement(pit, 6, "variance").run()
    assert _host(a.selected).tolist() == _host(b.selected).tolist()
    smax = float(np.max(np.sum(F * F, axis=1) + noise))
    scale = float(a.sel_delta[5])
    for key, rel in (("nom", smax), ("W", smax), ("s", scale), ("delta", scale)):
        diff = float(np.max(np.abs(_host(a.state()[key]) - _host(b.state()[key]))))
        assert diff <= TOL * rel, (key, diff)


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_rank_exhaustion(PC, criterion):
    """S = 6 samples: rank 5 after the centring, no noise.  Five picks use the covariance up;
    rounds 6 to 8 see every conditional variance below the threshold, score 0 everywhere and take
    the lowest free indices, as the longdouble reference does."""
    require_longdouble()
    T = np.random.default_rng(17).standard_normal((600, 6)) + 3.0
    fac = PC.FactoredCovariance.from_samples(T)
    F = _host(fac.F)
    ref = C.reference_run(FC.factor_cov_ld(F), criterion, 8)
    # The rounds whose pick the arithmetic decides.  Under the variance rule the last ones before
    # the rank runs out are ties by construction: on a residual v v^T of rank one every
    # delta_y = sum_v C_vy^2 / C_yy is |v|^2, and rounding picks.
    gaps = C.round_gaps(ref[:5], None)
    sure = next((r for r, (gap, low) in enumerate(gaps) if not (gap >= C.MIN_GAP and low)), 5)
    assert sure >= (5 if criterion == "entropy" else 3), gaps
    g = PC.CriterionPlacement(fac, 8, criterion).run()
    picks, deltas = g.result()
    picks = [int(p) for p in picks]
    assert picks[:sure] == [w.pick for w in ref[:sure]] and len(set(picks)) == 8
    if sure == 5:
        assert picks == [w.pick for w in ref]
    free = [i for i in range(600) if i not in picks[:5]]
    assert picks[5:] == free[:3]                                     # the lowest free indices
    assert (deltas[5:] == 0.0).all() and all(float(w.pick_delta) == 0.0 for w in ref[5:])
    for r in range(sure):
        assert abs(deltas[r] - float(ref[r].pick_delta)) <= TOL * float(ref[r].pick_delta)
    st = g.state()
    smax = float(np.max(np.sum(F * F, axis=1)))
    assert np.max(np.abs(_host(st["nom"]))) <= TOL * smax               # nothing is left
    assert (_host(st["W"][5:]) == 0.0).all()                             # and nothing was added


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_placement_from_samples(PC, criterion):
    from vgposp_amd.placement_algorithm2 import placement_from_samples
    name, S, rel = FC.FIXTURES[0]
    T, noise = (a.copy() for a in FC.sample_fixture(name, S, noise_rel=rel))
    _, F, _, _ = _fixture(PC, FC.FIXTURES[0])
    targets, cand = C.config_masks(name, "random")
    kw = dict(criterion=criterion, noise=noise, candidates=cand)
    if criterion == "variance":
        kw["targets"] = targets
    fact = placement_from_samples(T, 8, **kw)
    dense = placement_from_samples(T, 8, cov="dense", **kw)
    ref = FC.reference(F, noise, FC.FIXTURES[0] + ("device",), "random", criterion)
    assert [int(a) for a in fact] == [int(a) for a in dense] == [w.pick for w in ref[:8]]
    assert all(isinstance(a, np.int64) for a in fact)
    assert placement_from_samples(T, 0, **kw) == []
    # tr_stdev rescales Sigma and the noise alike: the same picks
    scaled = placement_from_samples(2.0 * T, 8, tr_stdev=2.0, **kw)
    assert [int(a) for a in scaled] == [int(a) for a in fact]
    # the mutual-information placement runs on the assembled matrix
    mi = placement_from_samples(T, 4, criterion="mi", noise=noise, cov="dense")
    assert len(set(int(a) for a in mi)) == 4
