"""What the sensors are for: place k sensors on the empirical covariance of S samples of a field
per site, then reconstruct further snapshots of the field at ALL sites from their values at the
picks alone, and map the variance that is left (placement_criteria.FieldReconstruction on a
FactoredCovariance: Sigma = F F^T + diag(noise) with F the centred samples over sqrt(S)).  Nothing
of size N x N or N x k is ever allocated.  Prints the RMSE of the reconstruction over all sites
against the prior standard deviation, the mean posterior variance, and the RMSE a random sensor set
of the same size gives.

    python examples/sample_reconstruction.py [--sites 16 16 16] [--samples 128] [--k 20]
                                             [--criterion variance|entropy|mi] [--heldout 16]

The field is the synthetic cosine field of examples/sample_placement.py; the first --samples
snapshots are what the placement sees, the next --heldout are reconstructed.
``--sites 128 128 128 --samples 256 --k 50`` works on 2.1 M sites, whose Sigma would be 35 TB.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

from sample_placement import NOISE, cosine_field_samples  # noqa: E402


def rmse(a, b):
    return float(((a - b) ** 2).mean().sqrt())


def run(sites=(16, 16, 16), samples=128, k=20, criterion="variance", heldout=16, seed=0):
    """-> {"picks", "rmse", "rmse_random", "prior_std", "mean_var", "prior_var", "seconds",
    "peak_bytes", "random_picks"}: the RMSE of the posterior mean of the ``heldout`` further
    snapshots over all sites for the placed sensors and for a random set of the same size, the
    prior standard deviation sqrt(mean diag Sigma), the mean posterior and prior variance, the wall
    time of placement + reconstruction and the device bytes held beside the snapshots at the
    peak."""
    import torch
    from vgposp_amd import placement_criteria as PC
    T = cosine_field_samples(sites, samples + heldout, seed=seed)
    seen, held = T[:, :samples].contiguous(), T[:, samples:].contiguous()
    del T
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    mu = seen.mean(1)
    fac = PC.FactoredCovariance.from_samples(seen, noise=NOISE)
    if criterion == "mi":
        picks = PC.placement_mutual_information(fac, k)
    elif criterion == "entropy":
        picks = PC.placement_entropy(fac, k)
    else:
        picks = PC.placement_variance_reduction(fac, k)
    picks = [int(a) for a in picks]
    rec = PC.FieldReconstruction(fac, picks, max_readings=max(1, min(heldout, 64)))
    mean, var = rec.mean_and_variance(held[picks], mean=mu)
    rec.check()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    peak = int(torch.cuda.max_memory_allocated() - base)
    prior_var = float((fac.F * fac.F).sum(1).mean()) + NOISE
    out = {"picks": picks, "rmse": rmse(mean, held), "prior_std": float(np.sqrt(prior_var)),
           "mean_var": float(var.mean()), "prior_var": prior_var, "seconds": seconds,
           "peak_bytes": peak}
    del mean, var, rec
    rand = np.random.default_rng(seed + 7).choice(fac.N, size=k, replace=False)
    out["random_picks"] = [int(a) for a in rand]
    rr = PC.FieldReconstruction(fac, rand, max_readings=max(1, min(heldout, 64)))
    out["rmse_random"] = rmse(rr.mean(held[out["random_picks"]], mean=mu), held)
    rr.check()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sites", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--samples", type=int, default=128, help="snapshots the placement sees")
    ap.add_argument("--k", type=int, default=20, help="sensors to place")
    ap.add_argument("--criterion", choices=("variance", "entropy", "mi"), default="variance")
    ap.add_argument("--heldout", type=int, default=16, help="further snapshots to reconstruct")
    a = ap.parse_args()
    if a.heldout < 1:
        ap.error("--heldout must be at least 1")
    r = run(tuple(a.sites), a.samples, a.k, a.criterion, a.heldout)
    n = int(np.prod(a.sites))
    print(f"sites {tuple(a.sites)} ({n:,}), {a.samples} samples, k = {a.k}, criterion "
          f"{a.criterion}, {a.heldout} held-out snapshots; Sigma would be "
          f"{8.0 * n * n / 1e9:,.1f} GB, the factor is {8.0 * n * a.samples / 1e9:,.3f} GB")
    print(f"picks {r['picks']}")
    print(f"placement + reconstruction {r['seconds']:.3f} s, {r['peak_bytes'] / 1e6:,.1f} MB on "
          "the device beside the snapshots")
    print(f"RMSE over all sites {r['rmse']:.4f}   (prior standard deviation {r['prior_std']:.4f})")
    print(f"mean posterior variance {r['mean_var']:.4f}   (prior {r['prior_var']:.4f})")
    print(f"RMSE of a random set of {a.k} sensors {r['rmse_random']:.4f}")


if __name__ == "__main__":
    main()
