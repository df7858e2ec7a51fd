"""GPU: the mutual-information placement on a factor against the dense path on the assembled
matrix, at 16^3 = 4,096 sites: ``FactoredMIPlacement`` on the centred samples and
``GreedyPlacement(empirical_cov(samples) + diag(noise)).run(16, lazy=False)``, which factors the
stored Sigma.  The gap between the best and the second-best delta of every dense round is asserted
first (>= MIN_GAP), so a pick is decided by the arithmetic; then the 16 picks are equal and every
pick's delta agrees to the project's 1e-9."""
import ctypes

import numpy as np
import pytest

from tests import numpy_criteria_greedy as C

pytestmark = pytest.mark.gpu
SHAPE = (16, 16, 16)
CASES = (("eq", 128), ("matern52", 300))
ROUNDS = 16


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


_built = {}


def _fixture(kind, S):
    """(samples [4096, S], noise [4096]): samples = chol(grid_cov) z + 3 as
    numpy_factor_cov.sample_fixture draws them (seed 21), noise = 1e-2 diag / 1.01."""
    if (kind, S) not in _built:
        Sigma = C.grid_cov(kind, SHAPE, 11)
        z = np.random.default_rng(21).standard_normal((Sigma.shape[0], S))
        _built[kind, S] = np.linalg.cholesky(Sigma) @ z + 3.0, 1e-2 * np.diag(Sigma) / 1.01
    return _built[kind, S]


def _dense_deltas(g):
    """The dense run's delta vector [n] in its workspace."""
    import torch
    from vgposp_amd._lib import call
    from vgposp_amd.linalg import _p
    d = ctypes.c_void_p()
    call("vgposp_greedy_buffers", _p(g.ws), g.n, g.kmax, ctypes.byref(d), None, None)
    off = d.value - g.ws.data_ptr()
    return g.ws[off:off + 8 * g.n].view(torch.float64)


@pytest.mark.parametrize("kind,S", CASES, ids=[f"{k}-S{s}" for k, s in CASES])
def test_picks_and_deltas_equal_the_dense_full_greedy(kind, S):
    import torch
    from vgposp_amd import placement_criteria as PC
    from vgposp_amd.covariance import empirical_cov
    from vgposp_amd.placement_algorithm2 import GreedyPlacement, placement_from_samples
    T, noise = _fixture(kind, S)
    n = T.shape[0]
    assert n == 4096
    Sigma = empirical_cov(T)
    torch.diagonal(Sigma).add_(torch.as_tensor(noise, device="cuda"))
    dense = GreedyPlacement(Sigma, ROUNDS).init()
    fac = PC.FactoredCovariance.from_samples(T, noise=noise)
    g = PC.FactoredMIPlacement(fac, ROUNDS).init()
    gaps, diffs = [], []
    taken = np.zeros(n, dtype=bool)
    for r in range(ROUNDS):
        dense.step(lazy=False)
        g.step()
        d = _dense_deltas(dense).cpu().numpy()
        top = np.sort(d[~taken])[::-1]
        gaps.append(float((top[0] - top[1]) / abs(top[0])))
        assert gaps[-1] >= C.MIN_GAP, (r, gaps[-1])
        want, got = int(dense.selected[r]), int(g.selected[r])
        assert want == C.argmax_low(d, ~taken)
        assert got == want, (r, got, want)
        taken[want] = True
        dd, gd = float(dense.sel_delta[r]), float(g.sel_delta[r])
        diffs.append(abs(gd - dd) / abs(dd))
    print(f"factor MI against the dense path, {kind} S={S}: smallest gap {min(gaps):.1e}, "
          f"worst pick-delta difference {max(diffs):.1e}")
    assert max(diffs) <= C.STATE_TOL, diffs
    picks = [int(p) for p in g.result()[0]]
    assert picks == [int(p) for p in dense.result()[0]]
    assert int(g.info[0]) == 0
    got = placement_from_samples(T, ROUNDS, "mi", noise)
    assert [int(p) for p in got] == picks
