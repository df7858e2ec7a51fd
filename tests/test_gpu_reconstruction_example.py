"""GPU: examples/sample_reconstruction.run at 8^3 sites, 64 samples, 8 sensors and 16 held-out
snapshots: the RMSE it returns against the same quantity computed in torch on the assembled Sigma
(within 1e-9 relative), and the posterior variance against the prior."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "examples"))


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _dense_rmse(seen, held, picks, noise):
    """The RMSE of mu + Sigma_VA Sigma_AA^-1 (y - mu_A) over all sites, Sigma the assembled
    empirical covariance of ``seen`` plus noise on the diagonal."""
    import torch
    mu = seen.mean(1)
    C = seen - mu[:, None]
    Sigma = C @ C.T / seen.shape[1]
    Sigma.diagonal().add_(noise)
    A = torch.as_tensor(picks, device=seen.device)
    alpha = torch.linalg.solve(Sigma[A][:, A], held[A] - mu[A, None])
    mean = mu[:, None] + Sigma[:, A] @ alpha
    var = Sigma.diagonal() - (Sigma[:, A] * torch.linalg.solve(Sigma[A][:, A], Sigma[A]).T).sum(1)
    return float(((mean - held) ** 2).mean().sqrt()), float(var.mean())


@pytest.mark.parametrize("criterion", ["variance", "mi"])
def test_example_against_the_assembled_covariance(criterion):
    import sample_reconstruction as ex
    sites, S, k, H = (8, 8, 8), 64, 8, 16
    r = ex.run(sites, S, k, criterion, H)
    assert len(r["picks"]) == len(set(r["picks"])) == k
    T = ex.cosine_field_samples(sites, S + H)
    seen, held = T[:, :S].contiguous(), T[:, S:].contiguous()
    want, want_var = _dense_rmse(seen, held, r["picks"], ex.NOISE)
    assert abs(r["rmse"] - want) <= 1e-9 * want, (r["rmse"], want)
    assert abs(r["mean_var"] - want_var) <= 1e-9 * want_var
    want_random, _ = _dense_rmse(seen, held, r["random_picks"], ex.NOISE)
    assert abs(r["rmse_random"] - want_random) <= 1e-9 * want_random
    assert 0.0 < r["mean_var"] < r["prior_var"]
    assert abs(r["prior_std"] ** 2 - r["prior_var"]) <= 1e-12
