"""GPU: greedy placement by variance reduction and by entropy (csrc/criteria.hip through
placement_criteria.CriterionPlacement) against the longdouble reference of
tests/numpy_criteria_greedy.py: the picks, and after every round the whole state.

Tolerance 1e-9 (the project's tolerance for deltas): delta and s relative to the round's pick
delta, nom and the new row of W relative to max diag Sigma.  The float64 restatement of the same
algorithm stays below 1e-13 on these inputs (tests/test_criteria_reference.py, which also asserts
the >= 1e-6 gap between the best and the second-best delta of every round that makes the picks
comparable at all)."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu
TOL = C.STATE_TOL


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def PC():
    from vgposp_amd import placement_criteria
    return placement_criteria


_dev = {}


def _cov(name):
    """The fixture on the device, uploaded once and never written."""
    import torch
    if name not in _dev:
        _dev[name] = torch.tensor(C.fixture_cov(name), device="cuda")   # (a copy: read-only host)
    return _dev[name]


def _host(t):
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("name,config,criterion", C.CONFIGS,
                         ids=["-".join(c) for c in C.CONFIGS])
def test_picks_and_state(PC, name, config, criterion):
    """Both rules on F1 (n = 1,320: three 512-row tiles, two 1,024-candidate chunks) and F2
    (n = 819, odd), plain, with random targets (half of V) / candidates (60 %) and with T = the odd,
    S = the even indices; F3 (rank 40 of 200) without any jitter."""
    require_longdouble()
    S = _cov(name)
    before = _host(S)
    T, cand = C.config_masks(name, config)
    T = None if criterion == "entropy" else T
    ref = C.reference(name, config, criterion)
    k = C.rounds_of(name)
    g = PC.CriterionPlacement(S, k, criterion, candidates=cand, targets=T).init()
    smax = float(np.max(np.diag(before)))
    worst = {"delta": 0.0, "s": 0.0, "nom": 0.0, "W": 0.0}
    for r, want in enumerate(ref):
        g.step()
        st = g.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        scale = float(want.pick_delta)
        err = {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
               "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
               "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax}
        if criterion == "variance":
            err["s"] = np.max(np.abs(_host(st["s"]) - want.s)) / scale
        for key, e in err.items():
            worst[key] = max(worst[key], float(e))
        assert abs(float(g.sel_delta[r]) - float(want.pick_delta)) <= TOL * scale, r
    print(f"criteria {name}-{config}-{criterion}: " +
          " ".join(f"{key} {v:.1e}" for key, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (k,)
    if cand is not None:
        assert cand[picks].all()
    assert _host(S).tobytes() == before.tobytes()      # Sigma is only read


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_placed_continues_a_free_run(PC, criterion):
    S = _cov("F1")
    picks, deltas = PC.CriterionPlacement(S, 8, criterion).run().result()
    g = PC.CriterionPlacement(S, 4, criterion, placed=picks[:4]).run()
    more, dmore = g.result()
    assert [int(p) for p in more] == [int(p) for p in picks[4:]]
    np.testing.assert_allclose(dmore, deltas[4:], rtol=TOL, atol=0)
    assert g.state()["W"].shape == (8, S.shape[0])


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_factored_buffer_gives_the_same_bits(PC, criterion):
    """On a clone that GreedyPlacement.init() factored in place (L^-1 below the diagonal, Sigma
    strictly above it) with diag = the saved diagonal: the same loads in the same order, so picks
    and deltas are bit-identical to the run on the raw Sigma."""
    import torch
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    S = _cov("F1")
    T, cand = C.config_masks("F1", "random")
    kw = dict(candidates=cand, targets=None if criterion == "entropy" else T)
    picks, deltas = PC.CriterionPlacement(S, C.K_ROUNDS, criterion, **kw).run().result()
    F = S.clone()
    diag = torch.diagonal(F).clone()
    mi = GreedyPlacement(F, 2).init()
    mi.check()
    n = F.shape[0]
    low = torch.tril_indices(n, n, -1, device=F.device)
    assert not torch.equal(F[low[0], low[1]], S[low[0], low[1]])      # really factored
    fpicks, fdeltas = PC.CriterionPlacement(F, C.K_ROUNDS, criterion, diag=diag,
                                            **kw).run().result()
    assert [int(p) for p in fpicks] == [int(p) for p in picks]
    assert fdeltas.tobytes() == deltas.tobytes()


def test_two_runs_are_bit_identical(PC):
    S = _cov("F2")
    a = PC.CriterionPlacement(S, 6, "variance").run()
    b = PC.CriterionPlacement(S, 6, "variance").run()
    assert _host(a.sel_delta).tobytes() == _host(b.sel_delta).tobytes()
    for key in ("nom", "s", "delta", "W"):
        assert _host(a.state()[key]).tobytes() == _host(b.state()[key]).tobytes(), key


def test_host_entry_points(PC):
    K = np.array(C.fixture_cov("F3"))
    want = [r.pick for r in C.incremental_run(K, "variance", 5)]
    got = PC.placement_variance_reduction(K, 5)
    assert [int(a) for a in got] == want and all(isinstance(a, np.int64) for a in got)
    want = [r.pick for r in C.incremental_run(K, "entropy", 5)]
    assert [int(a) for a in PC.placement_entropy(K, 5)] == want
    T, cand = C.odd_even(200)
    want = [r.pick for r in C.incremental_run(K, "variance", 4, T, cand, placed=[7, 100])]
    got = PC.placement_variance_reduction(K, 4, candidates=cand, placed=[7, 100],
                                          targets=np.flatnonzero(T))
    assert [int(a) for a in got] == want[2:]
    assert PC.placement_variance_reduction(K, 0) == [] and PC.placement_entropy(K, -1) == []


def test_argument_errors(PC):
    from vgposp_amd.data_generation import grid_points
    from vgposp_amd.placement_algorithm2 import placement_from_points
    K = np.array(C.fixture_cov("F3"))
    with pytest.raises(ValueError, match="targets mask must have length"):
        PC.placement_variance_reduction(K, 3, targets=np.ones(199, dtype=bool))
    with pytest.raises(ValueError, match="targets index 200"):
        PC.placement_variance_reduction(K, 3, targets=[1, 200])
    with pytest.raises(ValueError, match="exceeds the 2 candidates"):
        PC.placement_variance_reduction(K, 3, candidates=[4, 5, 6], placed=[5])
    with pytest.raises(ValueError, match="outside"):
        PC.placement_entropy(K, 0, candidates=[300])                   # validated at k < 1 too
    with pytest.raises(ValueError, match="targets mask must have length"):
        PC.placement_variance_reduction(K, 0, targets=np.ones(3, dtype=bool))
    with pytest.raises(ValueError, match="unknown criterion"):
        PC.CriterionPlacement(K, 3, "trace")
    with pytest.raises(ValueError, match="targets apply"):
        PC.CriterionPlacement(K, 3, "entropy", targets=[1, 2])
    with pytest.raises(ValueError, match="diag must have length"):
        PC.CriterionPlacement(K, 3, diag=np.ones(5))
    X = grid_points((4, 4, 4), jitter=0.05, seed=0)
    with pytest.raises(ValueError, match="targets apply"):
        placement_from_points(X, 3, criterion="mi", targets=[1, 2])
    with pytest.raises(ValueError, match="targets apply"):
        placement_from_points(X, 3, targets=[1, 2])
    with pytest.raises(ValueError, match="unknown criterion"):
        placement_from_points(X, 3, criterion="trace")
