"""GPU: the cross-covariance variance rule against an independent device path, and the example.

Sensors on an 8^3 grid with Sigma = K + (noise + jitter) I as placement_from_points assembles it,
targets on a jittered 12^3 mesh with R = K(Xt, X), the latent field without noise: the deltas must
sum to what GaussianProcessRegressionModel.variance (kernel strips, Cholesky + inverse, row sums of
squares; predictive noise 0) says the sensors took off the targets' weighted prior variance
amp^2, and variance_removed() is that difference target by target."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))

GRID, MESH, K = (8, 8, 8), (12, 12, 12), 8
AMP, NOISE, JITTER = 1.0, 1e-2, 1e-6


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _setup():
    from vgposp_amd.data_generation import grid_points, grid_spacing
    X = grid_points(GRID, jitter=0.05, seed=0)
    Xt = grid_points(MESH, jitter=0.3, seed=1)
    rng = np.random.default_rng(3)
    om = rng.uniform(0.5, 2.0, len(Xt))
    om[rng.random(len(Xt)) < 0.1] = 0.0
    return X, Xt, 2.0 * grid_spacing(GRID), om


def _mesh_variance(X, Xt, ls, picks):
    """The model's variance of the latent field at the mesh given sensors at ``picks``."""
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as tfkern
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=Xt,
        observation_index_points=X[picks], observations=np.zeros(len(picks)),
        observation_noise_variance=NOISE, predictive_noise_variance=0.0, jitter=JITTER)
    return gprm.variance().cpu().numpy()


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_deltas_sum_to_the_models_variance_reduction(weighted):
    from vgposp_amd import linalg
    from vgposp_amd.placement_algorithm2 import placement_from_points
    from vgposp_amd.placement_criteria import CriterionPlacement
    X, Xt, ls, om = _setup()
    om = om if weighted else None
    Sigma = linalg.kernel_matrix("eq", X, None, AMP, ls, diag_shift=NOISE + JITTER)[0]
    R = linalg.kernel_matrix("eq", Xt, X, AMP, ls)[0]
    g = CriterionPlacement(Sigma, K, "variance", cross_cov=R, target_weights=om).run()
    picks, deltas = g.result()
    picks = [int(a) for a in picks]
    assert len(set(picks)) == K
    prior = AMP * AMP
    removed = prior - _mesh_variance(X, Xt, ls, picks)
    reduction = float(np.sum(removed) if om is None else om @ removed)
    total = float(np.sum(deltas))
    print(f"sum of deltas {total:.15g}, model's reduction {reduction:.15g}, "
          f"relative difference {abs(total - reduction) / reduction:.2e}")
    assert abs(total - reduction) <= 1e-9 * reduction
    got = g.variance_removed().cpu().numpy()
    print(f"variance_removed: worst difference {np.max(np.abs(got - removed)) / prior:.2e} of "
          "the prior")
    assert got.shape == (len(Xt),) and np.max(np.abs(got - removed)) <= 1e-9 * prior
    again = placement_from_points(X, K, "eq", AMP, ls, NOISE, JITTER, criterion="variance",
                                  target_points=Xt, target_weights=om)
    assert [int(a) for a in again] == picks and all(isinstance(a, np.int64) for a in again)


def test_example_runs():
    import mesh_targets
    res = mesh_targets.run((5, 5, 5), (8, 8, 8), 4)
    assert set(res) == {"mesh", "in-V"}
    for rule, r in res.items():
        assert len(r["picks"]) == 4 and len(set(r["picks"])) == 4, rule
        assert 0.0 < r["mean_var"] <= r["max_var"] <= 1.0 + 1e-9 and r["seconds"] > 0.0, rule
