"""CPU: the conditions under which the GPU tests of the mutual-information placement on a factored
covariance (tests/test_gpu_factor_mi.py) mean something, and the host layer's argument errors.

On the longdouble Sigma = F F^T + diag(noise) of every fixture and configuration, over 16 rounds:
the best and the second-best delta are at least MIN_GAP apart, |nom| and |den| stay MIN_DISTANCE
away from the zeroing threshold, the float64 Woodbury restatement (tests/numpy_factor_mi.py, the
arithmetic of csrc/criteria.hip's vgposp_fmi_*) picks the longdouble arg-max, and its worst state
error e_cpu passes greedy_state_reference.tolerance (16 e_cpu <= 1e-11)."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_mi as FM
from tests.greedy_state_reference import LD, require_longdouble, tolerance

CASES = [(fx, cfg) for fx in FM.FIXTURES for cfg in FM.CONFIGS]
IDS = [f"{FM.fixture_id(f)}-{c}" for f, c in CASES]


def _checked_run(ref, F, noise, k, cand, placed=()):
    """The free restatement after ``placed``; asserts gaps, distances and picks per round and
    returns (picks, errors)."""
    g = FM.FactorMI(F, noise, candidates=cand)
    picks, errs = [], []
    for a in placed:
        picks.append(g.round(forced=a))
    for r in range(len(placed), len(placed) + k):
        picks.append(g.round())
        e = FM.state_errors(ref, picks, r, g.state(), cand)
        assert e["gap"] >= C.MIN_GAP, (r, e["gap"])
        assert e["min_nom"] >= FM.THRESHOLD + FM.MIN_DISTANCE, (r, e["min_nom"])
        assert e["min_den"] >= FM.THRESHOLD + FM.MIN_DISTANCE, (r, e["min_den"])
        assert picks[r] == e["argmax"], (r, picks[r], e["argmax"])
        errs.append(e)
    return picks, errs


@pytest.mark.parametrize("fx,config", CASES, ids=IDS)
def test_gaps_picks_and_restatement_error(fx, config):
    require_longdouble()
    assert len(CASES) == 9
    F, noise = FM.fixture_factor(fx)
    ref = FM.reference(F, noise, fx + ("numpy",))
    _, cand = C.config_masks(fx[0], config)
    picks, errs = _checked_run(ref, F, noise, FM.ROUNDS, cand)
    assert picks == FM.reference_picks(ref, FM.ROUNDS, cand)
    if cand is not None:
        assert cand[picks].all()
    e_cpu = FM.worst(errs)
    print(f"factor MI {FM.fixture_id(fx)}-{config}: e_cpu {e_cpu:.1e}, smallest gap "
          f"{min(e['gap'] for e in errs):.1e}, min |nom| {min(e['min_nom'] for e in errs):.1e}, "
          f"min |den| {min(e['min_den'] for e in errs):.1e}")
    tolerance(e_cpu)                                    # 16 e_cpu <= 1e-11
    # a forced run through the same picks is the same run
    assert FM.worst(FM.forced_run_errors(ref, F, noise, picks, cand)) == e_cpu


@pytest.mark.parametrize("fx", FM.FIXTURES, ids=[FM.fixture_id(f) for f in FM.FIXTURES])
def test_woodbury_diagonal_and_columns(fx):
    """Q_yy and the columns Q e_a of the closed forms against the longdouble inverse of Sigma
    (M^T M of its Cholesky factor): relative for the diagonal, normwise for a column, both inside
    the ceiling the state tolerance has."""
    require_longdouble()
    F, noise = FM.fixture_factor(fx)
    n = F.shape[0]
    ref = FM.reference(F, noise, fx + ("numpy",))
    g = FM.FactorMI(F, noise)
    want = ref.colsq(n)
    ed = float(np.max(np.abs(g.qdiag.astype(LD) - want) / want))
    ec = es = 0.0
    for a in (0, 1, n // 2, n - 2, n - 1):
        q = ref.qcol(a, n)
        ec = max(ec, float(np.max(np.abs(g.q_col(a).astype(LD) - q)) / np.max(np.abs(q))))
        s = ref.S[a, :n]
        es = max(es, float(np.max(np.abs(g.sigma_col(a).astype(LD) - s)) / np.max(np.abs(s))))
    print(f"Woodbury {FM.fixture_id(fx)}: diagonal {ed:.1e}, columns {ec:.1e}, "
          f"Sigma columns {es:.1e}")
    assert max(ed, ec, es) <= 1e-11 / 16


def test_placed_runs_as_forced_rounds():
    require_longdouble()
    fx = FM.FIXTURES[1]
    F, noise = FM.fixture_factor(fx)
    ref = FM.reference(F, noise, fx + ("numpy",))
    placed = [5, 400, 77]
    picks, errs = _checked_run(ref, F, noise, 6, None, placed)
    assert picks[:3] == placed and len(set(picks)) == 9
    assert picks[3:] == FM.reference_picks(ref, 6, None, placed)
    tolerance(FM.worst(errs))
    # the picks of a free run, handed over as `placed`, continue that run
    free = FM.reference_picks(ref, 6)
    assert FM.reference_picks(ref, 3, None, free[:3]) == free[3:]


@pytest.mark.parametrize("n,S", [s for s in FM.EDGE_SHAPES if s[1] <= 300],
                         ids=[f"n{n}-S{S}" for n, S in FM.EDGE_SHAPES if S <= 300])
def test_edge_shapes_hold_their_gaps(n, S):
    """The seeded random factors of the GPU test's edge shapes: gaps, distances and picks as for
    the fixtures (S = 4,096 is checked by the GPU test itself, on the same reference)."""
    require_longdouble()
    F, noise = FM.random_factor(n, S, FM.edge_seed(n, S))
    assert (noise >= 1e-2 * np.sum(F * F, axis=1)).all()
    ref = FM.reference(F, noise, ("edge", n, S))
    picks, errs = _checked_run(ref, F, noise, FM.edge_rounds(n), None)
    assert picks == FM.reference_picks(ref, FM.edge_rounds(n))
    tolerance(max(FM.worst(errs), FM.edge_error_floor(S, FM.edge_rounds(n))))


def test_exhausted_candidates():
    F, noise = FM.random_factor(40, 5, seed=1)
    g = FM.FactorMI(F, noise, candidates=[3, 17])
    assert sorted([g.round(), g.round()]) == [3, 17]
    before = {k: v.copy() for k, v in g.state().items() if k != "delta"}
    assert g.round() == -1 and g.round() == -1
    for k, v in before.items():
        assert np.array_equal(g.state()[k], v), k


def test_host_layer_argument_errors():
    """Raised before any device work: no GPU is needed."""
    from vgposp_amd import placement_criteria as PC
    from vgposp_amd.placement_algorithm2 import placement_from_samples
    F = np.random.default_rng(0).standard_normal((20, 6))
    part = np.full(20, 0.1)
    part[7] = 0.0
    for noise in (0.0, part, np.zeros(20)):
        fac = PC.FactoredCovariance(F, noise=noise)
        for make in (lambda: PC.FactoredMIPlacement(fac, 3),
                     lambda: PC.placement_mutual_information(fac, 3),
                     lambda: PC.placement_mutual_information(fac, 0),
                     lambda: placement_from_samples(F, 3, criterion="mi", noise=noise),
                     lambda: placement_from_samples(F, 0, criterion="mi", noise=noise,
                                                    cov="factored")):
            with pytest.raises(ValueError, match="mutual-information placement factors") as ei:
                make()
            assert "Woodbury" in str(ei.value) and "invertible" in str(ei.value)
    with pytest.raises(ValueError, match="noise must be finite and not negative"):
        placement_from_samples(F, 3, criterion="mi", noise=-1.0)
    with pytest.raises(ValueError, match="targets apply to criterion='variance'"):
        placement_from_samples(F, 3, criterion="mi", noise=0.1, targets=[1, 2])
    with pytest.raises(ValueError, match=r"samples must be \[N, S\]"):
        placement_from_samples(np.ones(7), 3, criterion="mi", noise=0.1)
    with pytest.raises(ValueError, match="1 <= S <= 4096"):
        placement_from_samples(np.ones((3, 4097)), 2, criterion="mi", noise=0.1)
    with pytest.raises(ValueError, match="1 <= S <= 4096"):
        PC.FactoredCovariance(np.ones((3, 0)), noise=0.1)
    good = PC.FactoredCovariance(F, noise=0.1)
    assert good.noise_is_positive() and not PC.FactoredCovariance(F, noise=part).noise_is_positive()
    for k in (0, 21, -2):
        with pytest.raises(ValueError, match=r"k must be in \[1, 20\]"):
            PC.FactoredMIPlacement(good, k)
    with pytest.raises(ValueError, match="candidates mask must have length 20"):
        PC.FactoredMIPlacement(good, 3, candidates=np.ones(19, dtype=bool))
    with pytest.raises(ValueError):
        PC.FactoredMIPlacement(good, 3, candidates=[25])
    with pytest.raises(ValueError):
        PC.placement_mutual_information(good, 0, placed=[20])
    with pytest.raises(ValueError, match="threshold must not be negative"):
        PC.FactoredMIPlacement(good, 3, threshold=-1.0)
    with pytest.raises(ValueError, match="needs a placement_criteria.FactoredCovariance"):
        PC.FactoredMIPlacement(F, 3)
    with pytest.raises(ValueError, match="needs a placement_criteria.FactoredCovariance"):
        PC.placement_mutual_information(F @ F.T, 3)
