"""Placement from samples alone: k sensors by variance reduction (or by entropy) on the empirical
covariance of S samples of a field per site, the covariance the reference places on
(tfp.stats.covariance of the tracer samples for every pair of locations), once assembled as the
N x N matrix (``cov="dense"``) and once as the factor it is (``cov="factored"``,
placement_criteria.FactoredCovariance: Sigma = F F^T + diag(noise) with F the centred samples over
sqrt(S)), which holds N S doubles instead of N^2.  Prints both pick lists, whether they are the
same, the wall time and the bytes held on the device at the peak.

    python examples/sample_placement.py [--sites 16 16 16] [--samples 128] [--k 20]
                                        [--criterion variance|entropy] [--skip-dense]

The field is synthetic and smooth: a sum of random cosines, evaluated with torch products on the
device (no Cholesky of a prior, so it works at any size).  --skip-dense is for site sets whose
covariance does not fit the device: ``--sites 128 128 128 --samples 256 --skip-dense`` places on
2.1 M sites, whose Sigma would be 35 TB.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vgposp_amd.data_generation import grid_points  # noqa: E402
from vgposp_amd.placement_algorithm2 import placement_from_samples  # noqa: E402

MODES, NOISE, MEAN = 48, 1e-2, 3.0
ROWS = (("dense", "dense"), ("factored", "factored"))


def cosine_field_samples(sites, samples, seed=0, rows=1 << 18):
    """T [N, S] on the device: T[i, s] = MEAN + sum_m A[s, m] cos(X_i . K_m + phi[s, m]) with
    wave vectors of a few periods across the grid, amplitudes falling with |K| and a prior
    variance near 1.  cos(u + phi) = cos u cos phi - sin u sin phi makes it two products."""
    import torch
    X = torch.as_tensor(grid_points(sites, jitter=0.05, seed=seed), device="cuda")
    rng = np.random.default_rng(seed + 1)
    K = rng.standard_normal((MODES, X.shape[1])) * 2.0 * np.pi * 1.5
    amp = np.exp(-0.5 * np.sum(K * K, axis=1) / (2.0 * np.pi * 2.5) ** 2)
    A = rng.standard_normal((samples, MODES)) * amp * np.sqrt(2.0 / np.sum(amp * amp))
    phi = rng.uniform(0.0, 2.0 * np.pi, (samples, MODES))
    Kd = torch.as_tensor(K.T.copy(), device="cuda")
    Ac = torch.as_tensor((A * np.cos(phi)).T.copy(), device="cuda")
    As = torch.as_tensor((A * np.sin(phi)).T.copy(), device="cuda")
    T = torch.empty((X.shape[0], samples), dtype=torch.float64, device="cuda")
    for r0 in range(0, X.shape[0], rows):
        u = X[r0:r0 + rows] @ Kd
        T[r0:r0 + rows] = torch.cos(u) @ Ac - torch.sin(u) @ As + MEAN
    return T


def run(sites=(16, 16, 16), samples=128, k=20, criterion="variance", dense=True):
    """-> {row: {"picks", "seconds", "peak_bytes"}} for the rows "dense" (unless ``dense`` is
    False) and "factored"."""
    import torch
    T = cosine_field_samples(sites, samples)
    out = {}
    for row, cov in ROWS:
        if cov == "dense" and not dense:
            continue
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        held = torch.cuda.memory_allocated()          # the samples themselves: the input
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        picks = placement_from_samples(T, k, criterion=criterion, noise=NOISE, cov=cov)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - t0
        out[row] = {"picks": [int(a) for a in picks], "seconds": seconds,
                    "peak_bytes": int(torch.cuda.max_memory_allocated() - held)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sites", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--samples", type=int, default=128, help="samples of the field per site")
    ap.add_argument("--k", type=int, default=20, help="sensors to place")
    ap.add_argument("--criterion", choices=("variance", "entropy"), default="variance")
    ap.add_argument("--skip-dense", action="store_true",
                    help="do not assemble Sigma (it may not fit the device)")
    a = ap.parse_args()
    res = run(tuple(a.sites), a.samples, a.k, a.criterion, not a.skip_dense)
    n = int(np.prod(a.sites))
    print(f"sites {tuple(a.sites)} ({n:,}), {a.samples} samples, k = {a.k}, criterion "
          f"{a.criterion}; Sigma would be {8.0 * n * n / 1e9:,.1f} GB, the factor is "
          f"{8.0 * n * a.samples / 1e9:,.3f} GB")
    print("covariance    seconds   device MB beside the samples   picks")
    for row, _ in ROWS:
        if row in res:
            r = res[row]
            print(f"{row:12s} {r['seconds']:8.3f}  {r['peak_bytes'] / 1e6:12.1f}"
                  f"                    {r['picks']}")
    if len(res) == 2:
        same = res["dense"]["picks"] == res["factored"]["picks"]
        print("same picks" if same else "DIFFERENT picks")
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
