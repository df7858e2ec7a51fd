"""GPU: variance-reduction placement for targets outside V (the vgposp_critx_* entries through
placement_criteria.CriterionPlacement(cross_cov=...)) against the longdouble reference of
tests/numpy_cross_criteria.py: the picks, and after every round the whole state.

Tolerance 1e-9 (the project's tolerance for deltas): delta and s relative to the round's pick
delta, nom and the new rows of W and U relative to max diag Sigma.  The float64 restatement of the
same algorithm stays below 1e-10 on these inputs (tests/test_cross_criteria_reference.py, which
also asserts the >= 1e-6 gap between the best and the second-best delta of every round that makes
the picks comparable at all)."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_cross_criteria as X
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu
TOL = X.STATE_TOL


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def PC():
    from vgposp_amd import placement_criteria
    return placement_criteria


_dev = {}


def _fixture(name):
    """(Sigma, R) on the device, uploaded once and never written."""
    import torch
    if name not in _dev:
        _dev[name] = tuple(torch.tensor(M, device="cuda") for M in X.fixture(name))
    return _dev[name]


def _host(t):
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("name,cfg", X.CONFIGS, ids=["-".join(c) for c in X.CONFIGS])
def test_picks_and_state(PC, name, cfg):
    """X1 (n = 504, P = 1,680: four 512-row tiles of R with a ragged end, seven 256-target chunks)
    and X2 (n = 420, P = 1,287, odd), plain and with weights (a tenth of them zero) and 60 %
    candidates."""
    require_longdouble()
    S, R = _fixture(name)
    before = _host(S), _host(R)
    om, cand = X.config(name, cfg)
    ref = X.reference(name, cfg)
    g = PC.CriterionPlacement(S, X.K_ROUNDS, "variance", candidates=cand, cross_cov=R,
                              target_weights=om).init()
    smax = float(np.max(np.diag(before[0])))
    worst = {"delta": 0.0, "s": 0.0, "nom": 0.0, "W": 0.0, "U": 0.0}
    for r, want in enumerate(ref):
        g.step()
        st = g.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        scale = float(want.pick_delta)
        err = {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
               "s": np.max(np.abs(_host(st["s"]) - want.s)) / scale,
               "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
               "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax,
               "U": np.max(np.abs(_host(st["U"][r]) - want.u)) / smax}
        for key, e in err.items():
            worst[key] = max(worst[key], float(e))
        assert abs(float(g.sel_delta[r]) - float(want.pick_delta)) <= TOL * scale, r
    print(f"cross criteria {name}-{cfg}: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (X.K_ROUNDS,)
    if cand is not None:
        assert cand[picks].all()
    st = g.state()
    assert st["U"].shape == (X.K_ROUNDS, R.shape[0]) and st["W"].shape == (X.K_ROUNDS, S.shape[0])
    removed = np.sum(np.array([w.u for w in ref], dtype=np.float64) ** 2, axis=0)
    assert np.max(np.abs(_host(g.variance_removed()) - removed)) <= TOL * smax
    assert _host(S).tobytes() == before[0].tobytes()      # Sigma and R are only read
    assert _host(R).tobytes() == before[1].tobytes()


def test_placed_continues_a_free_run(PC):
    S, R = _fixture("X1")
    om, cand = X.config("X1", "weighted")
    kw = dict(candidates=cand, cross_cov=R, target_weights=om)
    picks, deltas = PC.CriterionPlacement(S, 8, "variance", **kw).run().result()
    assert [int(p) for p in picks] == [w.pick for w in X.reference("X1", "weighted")[:8]]
    g = PC.CriterionPlacement(S, 4, "variance", placed=picks[:4], **kw).run()
    more, dmore = g.result()
    assert [int(p) for p in more] == [int(p) for p in picks[4:]]
    np.testing.assert_allclose(dmore, deltas[4:], rtol=TOL, atol=0)
    assert g.state()["U"].shape == (8, R.shape[0])


def test_rows_of_sigma_as_targets_give_the_in_v_run(PC):
    """R = Sigma[T, :] with unit weights is the existing rule with targets T (fixture F1 of
    tests/numpy_criteria_greedy.py, T = the odd, S = the even indices)."""
    import torch
    S = torch.tensor(C.fixture_cov("F1"), device="cuda")
    T, cand = C.odd_even(S.shape[0])
    want, dwant = PC.CriterionPlacement(S, 8, "variance", candidates=cand,
                                        targets=T).run().result()
    R = S[torch.as_tensor(np.flatnonzero(T), device="cuda")]
    got, dgot = PC.CriterionPlacement(S, 8, "variance", candidates=cand,
                                      cross_cov=R).run().result()
    assert [int(p) for p in got] == [int(p) for p in want]
    np.testing.assert_allclose(dgot, dwant, rtol=TOL, atol=0)


def test_singular_joint_covariance_without_jitter(PC):
    """X3: [Sigma; R] = Z Z^T / 40 of rank 40 (200 locations, 300 targets)."""
    require_longdouble()
    S, R = X.fixture("X3")
    ref = X.reference_run(S, R, 10)
    g = PC.CriterionPlacement(np.array(S), 10, "variance", cross_cov=np.array(R)).run()
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    want = np.array([w.pick_delta for w in ref], dtype=np.float64)
    assert np.max(np.abs(deltas - want) / want) <= TOL
    assert np.isfinite(_host(g.state()["s"])).all()


def test_row_pitched_view_and_two_runs(PC):
    """R as a view into a wider NaN-filled buffer (ldr = n + 3 > n, odd: the 8-byte load path)
    gives the picks and, to 1e-9, the deltas of the contiguous R; two runs on the same buffer are
    bit-identical in every part of the state."""
    import torch
    S, R = _fixture("X2")
    P, n = R.shape
    want, dwant = PC.CriterionPlacement(S, 6, "variance", cross_cov=R).run().result()
    wide = torch.full((P, n + 3), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, :n] = R
    view = wide[:, :n]
    assert view.stride(0) == n + 3
    a = PC.CriterionPlacement(S, 6, "variance", cross_cov=view).run()
    assert a.R.data_ptr() == wide.data_ptr()                 # used where it lies
    got, dgot = a.result()
    assert [int(p) for p in got] == [int(p) for p in want]
    np.testing.assert_allclose(dgot, dwant, rtol=TOL, atol=0)
    b = PC.CriterionPlacement(S, 6, "variance", cross_cov=view).run()
    assert _host(a.sel_delta).tobytes() == _host(b.sel_delta).tobytes()
    for key in ("nom", "s", "delta", "W", "U"):
        assert _host(a.state()[key]).tobytes() == _host(b.state()[key]).tobytes(), key


def test_host_entry_point(PC):
    S, R = X.fixture("X3")
    om, cand = X.weighted_config(200, 300)
    want = [r.pick for r in X.incremental_run(S, R, 4, om, cand, placed=[7, 100])]
    got = PC.placement_variance_reduction(np.array(S), 4, candidates=cand, placed=[7, 100],
                                          cross_cov=np.array(R), target_weights=om)
    assert [int(a) for a in got] == want[2:] and all(isinstance(a, np.int64) for a in got)
    assert PC.placement_variance_reduction(np.array(S), 0, cross_cov=np.array(R)) == []


def test_argument_errors(PC):
    from vgposp_amd.data_generation import grid_points
    from vgposp_amd.placement_algorithm2 import placement_from_points
    S, R = (np.array(M) for M in X.fixture("X3"))
    with pytest.raises(ValueError, match="exclude each other"):
        PC.CriterionPlacement(S, 3, cross_cov=R, targets=[1, 2])
    with pytest.raises(ValueError, match="variance' only"):
        PC.CriterionPlacement(S, 3, "entropy", cross_cov=R)
    with pytest.raises(ValueError, match="target_weights need cross_cov"):
        PC.CriterionPlacement(S, 3, "entropy", target_weights=np.ones(300))
    with pytest.raises(ValueError, match="target_weights need cross_cov"):
        PC.placement_variance_reduction(S, 3, target_weights=np.ones(300))
    with pytest.raises(ValueError, match="target_weights need cross_cov"):
        PC.placement_variance_reduction(S, 0, target_weights=np.ones(300))    # at k < 1 too
    with pytest.raises(ValueError, match=r"cross_cov must be \[P, 200\]"):
        PC.CriterionPlacement(S, 3, cross_cov=R[:, :199])
    with pytest.raises(ValueError, match=r"cross_cov must be \[P, 200\]"):
        PC.CriterionPlacement(S, 3, cross_cov=R[0])
    with pytest.raises(ValueError, match="target_weights must have length 300"):
        PC.CriterionPlacement(S, 3, cross_cov=R, target_weights=np.ones(299))
    for bad in (-1.0, np.nan, np.inf):
        w = np.ones(300)
        w[17] = bad
        with pytest.raises(ValueError, match="finite and not negative"):
            PC.CriterionPlacement(S, 3, cross_cov=R, target_weights=w)
    with pytest.raises(ValueError, match="needs cross_cov"):
        PC.CriterionPlacement(S, 3).variance_removed()
    Xs = grid_points((4, 4, 4), jitter=0.05, seed=0)
    Xt = grid_points((5, 5, 5), jitter=0.05, seed=1)
    for rule in ("mi", "entropy"):
        with pytest.raises(ValueError, match="target_points apply"):
            placement_from_points(Xs, 3, criterion=rule, target_points=Xt)
    with pytest.raises(ValueError, match="exclude each other"):
        placement_from_points(Xs, 3, criterion="variance", target_points=Xt, targets=[1, 2])
    with pytest.raises(ValueError, match=r"target_points must be \[P, 3\]"):
        placement_from_points(Xs, 3, criterion="variance", target_points=Xt[:, :2])
    with pytest.raises(ValueError, match="target_weights need target_points"):
        placement_from_points(Xs, 3, criterion="variance", target_weights=np.ones(64))
