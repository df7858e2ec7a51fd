"""Per-feature length scales: fit a 3-D grid field whose true length scale differs by axis with
the isotropic ExponentiatedQuadratic kernel and with FeatureScaled(ExponentiatedQuadratic), the
same Adam settings for both, and print both log marginal likelihoods, the recovered per-axis
scales and the held-out RMSE of each fit.

The field is a sum of sinusoids sin(2 pi x_k / period_k) with periods that differ by
axis, observed on a jittered grid with noise; every fourth point is held out.

    python examples/ard_fit.py [--grid 10 10 10] [--steps 150] [--lr 0.05]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vgposp_amd import distributions as tfd  # noqa: E402
from vgposp_amd import psd_kernels as tfkern  # noqa: E402
from vgposp_amd.data_generation import grid_points  # noqa: E402
from vgposp_amd.optimizers import AdamOptimizer, negate  # noqa: E402
from vgposp_amd.variables import Softplus, Variable  # noqa: E402

PERIODS = np.array([1.5, 4.0, 12.0])  # the field varies fast along x, slowly along z


def field(X, noise_sd=0.05, seed=1):
    rng = np.random.default_rng(seed)
    return np.sin(2 * np.pi * X / PERIODS).sum(1) + rng.normal(0.0, noise_sd, len(X))


def fit(X, y, Xt, yt, ard, steps, lr):
    """-> (final LML, held-out RMSE, effective per-axis length scales)."""
    amp, ls, noise = (Softplus(Variable(v, name=n)) for n, v in
                      (("amplitude", 0.54), ("length_scale", 0.54), ("noise", -3.0)))
    kernel = tfkern.ExponentiatedQuadratic(amp, ls)
    scale = None
    if ard:
        scale = Softplus(Variable(np.full(X.shape[1], 0.54), name="scale_diag"))
        kernel = tfkern.FeatureScaled(kernel, scale)
    gp = tfd.GaussianProcess(kernel, X, observation_noise_variance=noise)
    train_op = AdamOptimizer(lr).minimize(negate(gp.log_prob(y)))
    for _ in range(steps):
        train_op.run()
    lml = float(gp.log_prob(y))
    gprm = tfd.GaussianProcessRegressionModel(kernel, index_points=Xt, observation_index_points=X,
                                              observations=y, observation_noise_variance=noise)
    rmse = float(np.sqrt(np.mean((gprm.mean().cpu().numpy() - yt) ** 2)))
    eff = float(ls.numpy()) * (scale.numpy() if ard else np.ones(X.shape[1]))
    return lml, rmse, eff


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", type=int, nargs=3, default=[10, 10, 10])
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--lr", type=float, default=0.05)
    a = ap.parse_args()
    X = grid_points(tuple(a.grid), jitter=0.3, seed=0)
    y = field(X)
    held = np.arange(len(X)) % 4 == 0
    print(f"{(~held).sum()} training points, {held.sum()} held out; true periods {PERIODS}")
    for name, ard in (("ExponentiatedQuadratic", False), ("FeatureScaled(EQ)", True)):
        lml, rmse, eff = fit(X[~held], y[~held], X[held], y[held], ard, a.steps, a.lr)
        print(f"{name:24s} LML {lml:10.3f}   held-out RMSE {rmse:.4f}   "
              f"length scale per axis {np.array2string(eff, precision=3)}")


if __name__ == "__main__":
    main()
