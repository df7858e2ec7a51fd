"""Every dispatch rung of the C4 bounds kernels (exact_greedy.hip, launch_bounds_reg), on the
smallest grids that still hold a full K-step ball in the interior.  The other C4 tests reach only
the rungs their bound targets choose (K_lo = 3, K_hi = 5).

The seven-point reach table of K = 1 .. 8 steps has T = 7, 25, 63, 129, 231, 377, 575, 833 nodes:
* vgposp_exact_bounds (candidate ranges): the grouped kernel (K <= 3), rungs 3, 4, 6, 9 of the
  register kernel (K = 4 .. 7) and the generic kernel (K = 8).  Rung 2 (64 < T <= 128) has no K.
* vgposp_exact_tighten_pending / vgposp_exact_pretighten (candidate lists): rungs 4, 4, 6, 9, 14
  for K = 4 .. 8."""
import math

import numpy as np
import pytest
import torch

from oracle import placement as op
from oracle import taper as lp
from vgposp_amd.data_generation import grid_points, grid_spacing

pytestmark = pytest.mark.gpu

SHIFT = 0.01 + 1e-6
MARGIN = 1e-12                    # sparse_placement.BOUND_MARGIN
RANGE_SHAPE, LIST_SHAPE = (9, 10, 11), (12, 11, 10)
LIST_K, LIST_CUTOFF = 8, 2
# Chebyshev: every K whose width 4 rho^2K is below the refusal width of 1/2 on RANGE_SHAPE.  With
# the Gershgorin rho of the dense matrix (0.217 for eq, 0.203 for matern52) the widths of
# K = 1 .. 8 run from 0.19 / 0.17 down to 1e-10 / 3e-11: all eight.
CHEB_K = range(1, 9)


def _grid(shape, seed):
    return grid_points(shape, jitter=0.05, seed=seed), 2.0 * grid_spacing(shape)


@pytest.fixture(scope="module", params=["eq", "matern52"])
def range_problem(request):
    """(greedy, diag of the dense inverse, Gershgorin lambda_min, rho) on RANGE_SHAPE."""
    from vgposp_amd.sparse_placement import ExactWindowGreedy, TaperProblem
    kind, shape = request.param, RANGE_SHAPE
    X, ls = _grid(shape, sum(shape) + 1)
    C = lp.tapered_cov(X, shape, 4.0, kind=kind, ls=ls, diag_shift=SHIFT) + 1e-6 * np.eye(len(X))
    ref = np.diag(np.linalg.inv(C))
    g = ExactWindowGreedy(TaperProblem(X, shape, 4.0, kind, ls=ls, diag_shift=SHIFT), 4, 3)
    lo, hi = g.gershgorin(torch.zeros(g.p.n, dtype=torch.float64, device="cuda"))
    kappa = hi / lo
    return g, ref, lo, (math.sqrt(kappa) - 1.0) / (math.sqrt(kappa) + 1.0)


def _bounds(g, steps, mu, slabs):
    q = torch.zeros(g.p.n, dtype=torch.float64, device="cuda")
    for c0, c1 in slabs:
        assert g.bound_qdiag(q, c0, c1, steps=steps, mu=mu) == steps
    return q


@pytest.mark.parametrize("K", range(1, 9))
@pytest.mark.parametrize("radau", [False, True])
def test_bounds_every_rung(range_problem, K, radau):
    g, ref, lam_min, rho = range_problem
    width = 4.0 * rho ** (2 * K)
    if radau:
        steps, mu = (K, 1.0 + MARGIN, width), lam_min
    else:
        assert K in CHEB_K and width < 0.5
        steps, mu = (K, (1.0 + MARGIN) / (1.0 - width), width), 0.0
    n = g.p.n
    q = _bounds(g, steps, mu, [(0, n)])
    hi = q.cpu().numpy()
    assert np.all(hi >= ref)
    if not radau:
        assert np.all(hi <= ref * steps[1] * (1 + 1e-13))
    # the same bounds, bit for bit, slab by slab
    q3 = _bounds(g, steps, mu, [(0, n // 3), (n // 3, n - 5), (n - 5, n)])
    assert torch.equal(q, q3)


@pytest.fixture(scope="module")
def list_reference():
    shape = LIST_SHAPE
    X, ls = _grid(shape, 3)
    C = lp.tapered_cov(X, shape, 4.0, kind="eq", ls=ls, diag_shift=SHIFT)
    rA, _, rdci = op.placement_window_precision(C, LIST_K, shape, LIST_CUTOFF)
    return X, ls, rA, [rdci[a, i] for i, a in enumerate(rA)]


@pytest.mark.parametrize("K", [4, 5, 6, 7, 8])
@pytest.mark.parametrize("pre", [0, 64])
def test_list_rungs_pick_the_oracles_sensors(list_reference, K, pre):
    """The second bound level at K = 4 .. 8 steps (list rungs 4, 4, 6, 9, 14), on demand
    (tighten_pending) and with 64 candidates pre-tightened: the oracle's picks and deltas."""
    from vgposp_amd.sparse_placement import ExactTaperPlacement
    X, ls, rA, rdelta = list_reference
    run = ExactTaperPlacement(X, LIST_SHAPE, LIST_K, LIST_CUTOFF, 4.0, "eq", ls=ls,
                              diag_shift=SHIFT, method="bounds")
    g = run.greedy
    g.pretighten = pre
    lo = g.bound_qdiag(run.qdiag)
    assert lo is not None and g.tight is not None and g.bound_mu > 0 and lo[0] < K
    g.tight = (K, 1.0 + MARGIN, g.tight[2])      # the Gauss-Radau triple of K steps
    A = [int(a) for a in g.run_bounded(run.qdiag, LIST_K).cpu().numpy()]
    assert A == rA
    np.testing.assert_allclose(g.pick_delta[:LIST_K].cpu().numpy(), rdelta, rtol=1e-10)
    assert g.tightened > 0
    if pre:
        assert g.tightened >= pre
