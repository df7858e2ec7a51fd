"""GPU: the mutual-information placement on a factored covariance (vgposp_fmi_* through
placement_criteria.FactoredMIPlacement) against greedy_state_reference.LongdoubleGreedy on
Sigma = F F^T + diag(noise), with F the factor read back from the device.

After every round the whole state is compared (tests/numpy_factor_mi.state_errors): delta for every
unselected location (blocked ones included), nom, prec, and the rows of W and V; the pick is the
reference's arg-max.  The tolerance is greedy_state_reference.tolerance(e_cpu) = 16 e_cpu, with
e_cpu the error of the float64 numpy restatement on the same factor and picks
(tests/test_factor_mi_reference.py shows on the CPU that the gaps hold and e_cpu <= 1.3e-14 for the
numpy-centred factors).  The edge shapes take 16 max(e_cpu, numpy_factor_mi.edge_error_floor): on a
tiny input the restatement can be exact by accident."""
import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_factor_cov as FC
from tests import numpy_factor_mi as FM
from tests.greedy_state_reference import require_longdouble, tolerance

pytestmark = pytest.mark.gpu
CASES = [(fx, cfg) for fx in FM.FIXTURES for cfg in FM.CONFIGS]
STATE = ("nom", "prec", "delta", "W", "V")


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


def _host_state(g):
    return {k: _host(v) for k, v in g.state().items()}


def _fixture(PC, fx):
    """(FactoredCovariance from the samples, its factor read back, noise, the reference on it),
    built once per process and never written."""
    if fx not in _dev:
        name, S, rel = fx
        T, noise = (a.copy() for a in FC.sample_fixture(name, S, noise_rel=rel))
        fac = PC.FactoredCovariance.from_samples(T, noise=noise)
        F = _host(fac.F)
        _dev[fx] = fac, F, noise, FM.reference(F, noise, fx + ("device",))
    return _dev[fx]


def _run_and_compare(PC, fac, ref, F, noise, k, cand=None, placed=(), floor=0.0, label=""):
    """k free rounds after ``placed``: gaps on the reference, picks, the state after every round
    within the tolerance, info 0.  Returns the placement."""
    placed = [int(a) for a in placed]
    want = placed + FM.reference_picks(ref, k, cand, placed)
    cpu = FM.forced_run_errors(ref, F, noise, want, cand, first=len(placed))
    e_cpu = FM.worst(cpu)
    tol = tolerance(max(e_cpu, floor))
    assert all(e["gap"] >= C.MIN_GAP for e in cpu), [e["gap"] for e in cpu]
    g = PC.FactoredMIPlacement(fac, k, candidates=cand, placed=placed or None).init()
    assert _host(g.selected[:len(placed)]).tolist() == placed
    errs = []
    for r in range(len(placed), len(placed) + k):
        g.step()
        pick = int(g.selected[r])
        assert pick == want[r], (r, pick, want[r])
        e = FM.state_errors(ref, want, r, _host_state(g), cand)
        assert pick == e["argmax"], (r, pick, e["argmax"])
        errs.append(e)
    worst = {key: max(e[key] for e in errs) for key in FM.ERROR_KEYS}
    print(f"factor MI {label}: e_cpu {e_cpu:.1e}, tolerance {tol:.1e}, device "
          + " ".join(f"{key} {v:.1e}" for key, v in worst.items())
          + f", smallest gap {min(e['gap'] for e in errs):.1e}")
    for key, v in worst.items():
        assert v <= tol, (key, v, tol)
    assert int(g.info[0]) == 0                        # C is positive definite whenever d > 0
    picks, deltas = g.result()
    assert [int(p) for p in picks] == want[len(placed):]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (k,)
    for r, d in enumerate(deltas):
        st = ref.state(want[:len(placed) + r]).delta[want[len(placed) + r]]
        assert abs(d - float(st)) <= tol * abs(float(st)), r
    return g


@pytest.mark.parametrize("fx,config", CASES, ids=[f"{FM.fixture_id(f)}-{c}" for f, c in CASES])
def test_picks_and_state(PC, fx, config):
    require_longdouble()
    assert len(CASES) == 9
    fac, F, noise, ref = _fixture(PC, fx)
    before = _host(fac.F).tobytes(), _host(fac.noise).tobytes()
    _, cand = C.config_masks(fx[0], config)
    g = _run_and_compare(PC, fac, ref, F, noise, FM.ROUNDS, cand,
                         label=f"{FM.fixture_id(fx)}-{config}")
    if cand is not None:
        assert cand[g.result()[0]].all()
    st = g.state()
    assert st["W"].shape == st["V"].shape == (FM.ROUNDS, fac.N)
    assert (_host(fac.F).tobytes(), _host(fac.noise).tobytes()) == before   # only read


def test_placed_runs_as_forced_rounds(PC):
    require_longdouble()
    fx = FM.FIXTURES[1]
    fac, F, noise, ref = _fixture(PC, fx)
    g = _run_and_compare(PC, fac, ref, F, noise, 6, placed=[5, 400, 77], label="placed")
    assert g.state()["W"].shape == (9, fac.N)
    # the picks of a free run, handed over as `placed`, continue that run
    free = [int(p) for p in PC.placement_mutual_information(fac, 6)]
    assert free == FM.reference_picks(ref, 6)
    more = PC.placement_mutual_information(fac, 3, placed=free[:3])
    assert [int(p) for p in more] == free[3:]
    assert PC.placement_mutual_information(fac, 0) == []


def test_from_samples_against_a_hand_centred_factor(PC):
    """The factor the device centred against the numpy-centred one, uploaded as it is: the same
    picks, each within the tolerance of its own reference."""
    require_longdouble()
    fx = FM.FIXTURES[1]
    fac, F, noise, ref = _fixture(PC, fx)
    Fh, _ = FM.fixture_factor(fx)
    assert np.max(np.abs(F - Fh)) <= 1e-14
    hand = PC.FactoredCovariance(Fh, noise=noise)
    assert _host(hand.F).tobytes() == Fh.tobytes()
    g = _run_and_compare(PC, hand, FM.reference(Fh, noise, fx + ("numpy",)), Fh, noise, FM.ROUNDS,
                         label="hand-centred")
    assert [int(p) for p in g.result()[0]] == FM.reference_picks(ref, FM.ROUNDS)


@pytest.mark.parametrize("fx,pad,shift", [(FM.FIXTURES[0], 3, 0), (FM.FIXTURES[0], 2, 1),
                                           (FM.FIXTURES[1], 1, 0)],
                         ids=["S96-odd-pitch", "S96-even-pitch-off-16-bytes", "S75-even-pitch"])
def test_a_pitched_factor(PC, fx, pad, shift):
    """F as a view of a wider buffer, NaN in the padding: an odd pitch and an even pitch that
    starts 8 bytes off a 16-byte boundary take the 8-byte loads; S = 75 at the aligned pitch 76
    takes the 16-byte loads with a lone last column."""
    import torch
    require_longdouble()
    fac, F, noise, ref = _fixture(PC, fx)
    n, S = F.shape
    ld = S + pad
    flat = torch.full((n * ld + 2,), float("nan"), dtype=torch.float64, device="cuda")
    view = flat[shift:shift + n * ld].view(n, ld)[:, :S]
    view.copy_(fac.F)
    pit = PC.FactoredCovariance(view, noise=noise)
    assert pit.F.data_ptr() == flat.data_ptr() + 8 * shift and pit.args()[3] == ld
    vec = pit.F.data_ptr() % 16 == 0 and ld % 2 == 0
    assert vec == (fx[1] == 75)
    _run_and_compare(PC, pit, ref, F, noise, FM.ROUNDS, label=f"pitch {ld} shift {shift}")
    assert bool(torch.isnan(flat[-1]))


@pytest.mark.parametrize("n,S", FM.EDGE_SHAPES, ids=[f"n{n}-S{S}" for n, S in FM.EDGE_SHAPES])
def test_edge_shapes(PC, n, S):
    """S around a wave's 128 columns and odd, n around a wave's 64 rows and a workgroup's 256,
    S > n, and S = 4,096 (u_a read through L2 beside f_a in LDS)."""
    require_longdouble()
    F, noise = FM.random_factor(n, S, FM.edge_seed(n, S))
    ref = FM.reference(F, noise, ("edge", n, S))
    fac = PC.FactoredCovariance(F, noise=noise)
    k = FM.edge_rounds(n)
    _run_and_compare(PC, fac, ref, F, noise, k, floor=FM.edge_error_floor(S, k),
                     label=f"edge n={n} S={S}")


def test_exhausted_candidates_leave_later_rounds_inert(PC):
    """Two candidates, four rounds: rounds 2 and 3 select -1 and change nothing."""
    import torch
    F, noise = FM.random_factor(40, 5, seed=1)
    g = PC.FactoredMIPlacement(PC.FactoredCovariance(F, noise=noise), 4)
    allowed = np.zeros(40, dtype=np.uint8)
    allowed[[3, 17]] = 1
    g._allowed_dev = torch.as_tensor(allowed, device="cuda")   # (the constructor refuses k > 2)
    g.init()
    g.step()
    g.step()
    assert sorted(_host(g.selected[:2]).tolist()) == [3, 17]
    cpu = FM.FactorMI(F, noise, candidates=[3, 17])
    assert [cpu.round(), cpu.round()] == _host(g.selected[:2]).tolist()
    before = {k: v[:2] if k in "WV" else v for k, v in _host_state(g).items() if k != "delta"}
    g.step()
    g.step()
    assert _host(g.selected).tolist()[2:] == [-1, -1]
    assert _host(g.sel_delta).tolist()[2:] == [0.0, 0.0]
    after = _host_state(g)
    for key, v in before.items():
        assert np.array_equal(after[key][:2] if key in "WV" else after[key], v), key
    with pytest.raises(RuntimeError, match="found no candidate"):
        g.result()


def test_two_runs_are_bit_identical(PC):
    import torch
    fac = _fixture(PC, FM.FIXTURES[2])[0]
    a = PC.FactoredMIPlacement(fac, 6).run()
    b = PC.FactoredMIPlacement(fac, 6).run()
    assert torch.equal(a.selected, b.selected) and torch.equal(a.sel_delta, b.sel_delta)
    for key in STATE:
        assert torch.equal(a.state()[key], b.state()[key]), key


def test_placement_from_samples(PC):
    from vgposp_amd.placement_algorithm2 import placement_from_samples
    require_longdouble()
    fx = FM.FIXTURES[0]
    _, _, noise, ref = _fixture(PC, fx)
    T = FC.sample_fixture(fx[0], fx[1], noise_rel=fx[2])[0].copy()
    _, cand = C.config_masks(fx[0], "random")
    got = placement_from_samples(T, 8, criterion="mi", noise=noise, candidates=cand)
    assert [int(a) for a in got] == FM.reference_picks(ref, 8, cand)
    assert all(isinstance(a, np.int64) for a in got)
    assert placement_from_samples(T, 0, criterion="mi", noise=noise) == []
    # twice the samples under tr_stdev = 2 are the same factor: the same picks
    scaled = placement_from_samples(2.0 * T, 8, criterion="mi", noise=noise, tr_stdev=2.0,
                                    candidates=cand)
    assert [int(a) for a in scaled] == [int(a) for a in got]
    with pytest.raises(ValueError, match="mutual-information placement factors"):
        placement_from_samples(T, 8, criterion="mi", noise=0.0)
