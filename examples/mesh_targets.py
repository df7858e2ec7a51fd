"""Sensors on a coarse grid of admissible sites, the field judged on a finer mesh: place k sensors
by variance reduction with the mesh as targets (``target_points``: the cross-covariance K(Xt, X)
of the latent field, one pass over it per round) and with the sites themselves as targets (the
in-V rule), and print what each leaves of the field's uncertainty over the mesh.

The variance is the marginal predictive one of a GP regression model conditioned on the picked
sites (``GaussianProcessRegressionModel.variance``, as examples/variance_map.py), noise-free at the
mesh.  The mesh cells may carry weights (here: all ones unless --weighted, which counts the inner
half of the domain twice).

    python examples/mesh_targets.py [--sites 10 10 10] [--mesh 24 24 24] [--k 20] [--weighted]
                                    [--matrix-free]

--matrix-free never assembles K(Xt, X): its entries are generated from the points in every round
(``cross="matrix_free"``), for a mesh whose cross-covariance does not fit the device.
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
RULES = ("mesh", "in-V")


def mesh_variance(X, Xt, picks, ls, chunk_points=None):
    """Predictive variance of the noise-free field over Xt given sensors at X[picks] (host)."""
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=Xt,
        observation_index_points=X[picks], observations=np.zeros(len(picks)),
        observation_noise_variance=NOISE, predictive_noise_variance=0.0, jitter=JITTER)
    return gprm.variance(chunk_points=chunk_points).cpu().numpy()


def run(sites=(10, 10, 10), mesh=(24, 24, 24), k=20, weights=None, matrix_free=False):
    """-> {rule: {"picks", "mean_var", "max_var", "seconds"}}: "mesh" places for the (weighted)
    posterior variance over the mesh, "in-V" for the one over the sites.  ``mean_var`` is the
    weighted mean over the mesh."""
    import torch
    X = grid_points(sites, jitter=0.05, seed=0)
    Xt = grid_points(mesh, jitter=0.3, seed=1)
    ls = 2.0 * grid_spacing(sites)
    om = np.ones(len(Xt)) if weights is None else np.asarray(weights, dtype=np.float64)
    out = {}
    for rule in RULES:
        kw = {"target_points": Xt, "target_weights": weights} if rule == "mesh" else {}
        if rule == "mesh" and matrix_free:
            kw["cross"] = "matrix_free"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        picks = placement_from_points(X, k, "eq", AMP, ls, NOISE, JITTER, criterion="variance",
                                      **kw)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        picks = [int(a) for a in picks]
        var = mesh_variance(X, Xt, picks, ls)
        out[rule] = {"picks": picks, "mean_var": float(om @ var / om.sum()),
                     "max_var": float(var.max()), "seconds": seconds}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sites", type=int, nargs=3, default=[10, 10, 10])
    ap.add_argument("--mesh", type=int, nargs=3, default=[24, 24, 24])
    ap.add_argument("--k", type=int, default=20, help="sensors to place")
    ap.add_argument("--weighted", action="store_true",
                    help="count the mesh points with |x|_inf <= 1 twice")
    ap.add_argument("--matrix-free", action="store_true",
                    help="generate the mesh's cross-covariance in every round, never store it")
    a = ap.parse_args()
    weights = None
    if a.weighted:
        Xt = grid_points(tuple(a.mesh), jitter=0.3, seed=1)
        weights = np.where(np.abs(Xt).max(axis=1) <= 1.0, 2.0, 1.0)
    res = run(tuple(a.sites), tuple(a.mesh), a.k, weights, a.matrix_free)
    print(f"sites {tuple(a.sites)}, mesh {tuple(a.mesh)}, k = {a.k}, prior variance {AMP * AMP}")
    print("targets   mean variance   max variance   seconds   picks")
    for rule in RULES:
        r = res[rule]
        print(f"{rule:8s}  {r['mean_var']:13.6f}  {r['max_var']:13.6f}  {r['seconds']:8.3f}   "
              f"{r['picks']}")


if __name__ == "__main__":
    main()
