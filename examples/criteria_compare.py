"""Three placement rules on one field: place k sensors on a jittered grid by mutual information,
by variance reduction and by entropy, and print what each leaves of the field's uncertainty — the
mean and the largest posterior standard deviation over the grid — and the wall time of each.

The standard deviation is the marginal predictive one of a GP regression model conditioned on the
picked locations (``GaussianProcessRegressionModel.stddev``, as examples/variance_map.py).
Variance reduction minimises the mean of the variance by construction (greedily); entropy and
mutual information are the rules it is usually compared with.

    python examples/criteria_compare.py [--grid 16 16 16] [--k 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vgposp_amd import distributions as tfd  # noqa: E402
from vgposp_amd import psd_kernels as tfkern  # noqa: E402
from vgposp_amd.data_generation import grid_points, grid_spacing  # noqa: E402
from vgposp_amd.placement_algorithm2 import placement_from_points  # noqa: E402

AMP, NOISE, JITTER = 1.0, 1e-2, 1e-6   # the placement benchmark's kernel and diagonal shift
RULES = ("mi", "variance", "entropy")


def posterior_stddev(X, picks, ls, chunk_points=None):
    """Predictive stddev of the noise-free field over X given sensors at X[picks] (host array)."""
    kernel = tfkern.ExponentiatedQuadratic(AMP, ls)
    gprm = tfd.GaussianProcessRegressionModel(
        kernel, index_points=X, observation_index_points=X[picks],
        observations=np.zeros(len(picks)), observation_noise_variance=NOISE,
        predictive_noise_variance=0.0, jitter=JITTER)
    return gprm.stddev(chunk_points=chunk_points).cpu().numpy()


def run(grid=(16, 16, 16), k=20, candidates=None, targets=None):
    """-> {rule: {"picks", "mean_sd", "max_sd", "seconds"}} for the three rules.  ``targets``
    reaches the variance rule only (the other two have no target set)."""
    import torch
    X = grid_points(grid, jitter=0.05, seed=0)
    ls = 2.0 * grid_spacing(grid)
    out = {}
    for rule in RULES:
        kw = {"targets": targets} if rule == "variance" else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        picks = placement_from_points(X, k, "eq", AMP, ls, NOISE, JITTER, candidates=candidates,
                                      criterion=rule, **kw)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        picks = [int(a) for a in picks]
        sd = posterior_stddev(X, picks, ls)
        out[rule] = {"picks": picks, "mean_sd": float(sd.mean()), "max_sd": float(sd.max()),
                     "seconds": seconds}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--k", type=int, default=20, help="sensors to place")
    a = ap.parse_args()
    res = run(tuple(a.grid), a.k)
    print(f"grid {tuple(a.grid)}, k = {a.k}")
    print("rule       mean stddev   max stddev   seconds   picks")
    for rule in RULES:
        r = res[rule]
        print(f"{rule:9s}  {r['mean_sd']:11.6f}  {r['max_sd']:11.6f}  {r['seconds']:8.3f}   "
              f"{r['picks']}")


if __name__ == "__main__":
    main()
