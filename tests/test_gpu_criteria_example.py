"""GPU: the variance rule's objective against an independent device path, and the example.

On an 8^3 grid with T = the odd and S = the even indices, Sigma = K + (noise + jitter) I as
placement_from_points assembles it: the deltas of the variance rule must sum to what
GaussianProcessRegressionModel.variance (kernel strips, Cholesky + inverse, row sums of squares)
says the sensors took off the targets' variance.  Exact because A and T are disjoint: no target
is itself observed, so the model with predictive noise = noise + jitter describes the same noisy
variables as Sigma."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))

GRID, K = (8, 8, 8), 8
AMP, NOISE, JITTER = 1.0, 1e-2, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _setup():
    from vgposp_amd.data_generation import grid_points, grid_spacing
    X = grid_points(GRID, jitter=0.05, seed=0)
    n = len(X)
    return X, 2.0 * grid_spacing(GRID), np.arange(n) % 2 == 1, np.arange(n) % 2 == 0


def _target_variance(X, ls, T, picks):
    """The model's variance of the noisy variables at the targets given sensors at ``picks``."""
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as tfkern
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=X[T],
        observation_index_points=X[picks], observations=np.zeros(len(picks)),
        observation_noise_variance=NOISE, predictive_noise_variance=NOISE + JITTER, jitter=JITTER)
    return gprm.variance().cpu().numpy()


def test_deltas_sum_to_the_models_variance_reduction():
    from vgposp_amd import linalg
    from vgposp_amd.placement_algorithm2 import placement_from_points
    from vgposp_amd.placement_criteria import CriterionPlacement
    X, ls, T, S = _setup()
    Sigma = linalg.kernel_matrix("eq", X, None, AMP, ls, diag_shift=NOISE + JITTER)[0]
    picks, deltas = CriterionPlacement(Sigma, K, "variance", candidates=S,
                                       targets=T).run().result()
    picks = [int(a) for a in picks]
    assert len(set(picks)) == K and S[picks].all()
    got = placement_from_points(X, K, "eq", AMP, ls, NOISE, JITTER, candidates=S,
                                criterion="variance", targets=T)
    assert [int(a) for a in got] == picks
    prior = AMP * AMP + NOISE + JITTER
    reduction = float(np.sum(prior - _target_variance(X, ls, T, picks)))
    total = float(np.sum(deltas))
    print(f"sum of deltas {total:.15g}, model's reduction {reduction:.15g}, "
          f"relative difference {abs(total - reduction) / reduction:.2e}")
    assert abs(total - reduction) <= 1e-9 * reduction


def test_first_variance_pick_is_the_best_single_sensor():
    """Guaranteed by construction for k = 1 (not for k > 1: greedy is not optimal)."""
    from vgposp_amd.placement_algorithm2 import placement_from_points
    X, ls, T, S = _setup()
    first = {}
    for rule in ("mi", "variance", "entropy"):
        kw = {"targets": T} if rule == "variance" else {}
        a = placement_from_points(X, 1, "eq", AMP, ls, NOISE, JITTER, candidates=S,
                                  criterion=rule, **kw)
        first[rule] = float(np.mean(_target_variance(X, ls, T, [int(a[0])])))
    assert first["variance"] <= first["mi"] and first["variance"] <= first["entropy"], first


def test_example_runs():
    import criteria_compare
    res = criteria_compare.run(GRID, K)
    assert set(res) == {"mi", "variance", "entropy"}
    for rule, r in res.items():
        assert len(r["picks"]) == K and len(set(r["picks"])) == K, rule
        assert 0.0 < r["mean_sd"] <= r["max_sd"] <= 1.0 + 1e-9 and r["seconds"] > 0.0, rule
