"""Placement from points alone: k sensors by variance reduction (or by entropy) on a grid of
admissible sites, once with the covariance Sigma = K(X, X) + (noise + jitter) I assembled on the
device and once with ``cov="matrix_free"``, which never stores Sigma and generates its entries from
the points in every round (placement_criteria.SiteKernel).  Prints both pick lists, the mean
posterior variance each leaves (over the mesh with --mesh, else over the sites), the time and the
device memory held at the peak.

    python examples/points_only_placement.py [--sites 16 16 16] [--k 20]
                                             [--criterion variance|entropy] [--mesh a b c]
                                             [--skip-dense]

--mesh judges the field on a finer mesh instead of the sites (variance rule): both sides are then
generated, and nothing of size N^2 or P N is held.  --skip-dense is for site sets whose Sigma does
not fit the device: 64^3 sites would need 550 GB.
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
ROWS = (("dense", "dense"), ("matrix-free", "matrix_free"))


def posterior_variance(X, Xt, picks, ls):
    """Predictive variance of the noise-free field over Xt given sensors at X[picks] (host)."""
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=Xt,
        observation_index_points=X[picks], observations=np.zeros(len(picks)),
        observation_noise_variance=NOISE, predictive_noise_variance=0.0, jitter=JITTER)
    return gprm.variance().cpu().numpy()


def run(sites=(16, 16, 16), k=20, criterion="variance", mesh=None, dense=True):
    """-> {row: {"picks", "mean_var", "seconds", "peak_bytes"}} for the rows "dense" (unless
    ``dense`` is False) and "matrix-free"."""
    import torch
    X = grid_points(sites, jitter=0.05, seed=0)
    Xt = grid_points(mesh, jitter=0.3, seed=1) if mesh is not None else None
    ls = 2.0 * grid_spacing(sites)
    kw = {"target_points": Xt} if Xt is not None else {}
    out = {}
    for row, cov in ROWS:
        if cov == "dense" and not dense:
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        picks = placement_from_points(X, k, "eq", AMP, ls, NOISE, JITTER, criterion=criterion,
                                      cov=cov, **kw)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        peak = torch.cuda.max_memory_allocated()
        picks = [int(a) for a in picks]
        var = posterior_variance(X, X if Xt is None else Xt, picks, ls)
        out[row] = {"picks": picks, "mean_var": float(var.mean()), "seconds": seconds,
                    "peak_bytes": int(peak)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sites", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--k", type=int, default=20, help="sensors to place")
    ap.add_argument("--criterion", choices=("variance", "entropy"), default="variance")
    ap.add_argument("--mesh", type=int, nargs=3, default=None,
                    help="judge the field on this mesh instead of the sites (variance rule)")
    ap.add_argument("--skip-dense", action="store_true",
                    help="do not assemble Sigma (it may not fit the device)")
    a = ap.parse_args()
    mesh = tuple(a.mesh) if a.mesh else None
    res = run(tuple(a.sites), a.k, a.criterion, mesh, not a.skip_dense)
    print(f"sites {tuple(a.sites)}, k = {a.k}, criterion {a.criterion}, targets "
          f"{'the sites' if mesh is None else mesh}, prior variance {AMP * AMP}")
    print("covariance    mean variance   seconds   device MB   picks")
    for row, _ in ROWS:
        if row in res:
            r = res[row]
            print(f"{row:12s}  {r['mean_var']:13.6f}  {r['seconds']:8.3f}  "
                  f"{r['peak_bytes'] / 1e6:10.1f}   {r['picks']}")


if __name__ == "__main__":
    main()
