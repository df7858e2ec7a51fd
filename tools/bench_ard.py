"""Time the FeatureScaled (per-feature length scale) kernels against their isotropic counterparts.

1. ``vgposp_kernel_vjp_scaled`` against ``vgposp_kernel_vjp`` on the two Kzx shapes of the VGP
   configs: C5 (M = 1,024 x N = 65,536, d = 5) and C3 (512 x 262,144, d = 3).  Both stream Kbar
   once (8 B per entry); the scaled entry adds d multiply-adds per entry.  The condition: scaled
   takes less than 2 x isotropic (two isotropic passes, X1bar then X2bar from a transposed Kbar,
   are the only other way to the scale gradient).
2. The C5-shaped VGP training step with FeatureScaled(Matern 5/2) against the isotropic step.

Device events around each call, a warm-up, ``--reps`` repetitions with the variants alternating,
median and spread (min, max) reported.  One JSON document, printed and written to ``--out``.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vgposp_amd import linalg  # noqa: E402
from vgposp_amd.vgp_training import kernel_vjp  # noqa: E402
from vgposp_amd.workloads import vgp_c3_graph, vgp_c5_data  # noqa: E402


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _stats(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)),
            "reps": len(ms)}


def bench_vjp(name, m, n, d, kind, reps, warmup):
    rng = np.random.default_rng(0)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    Z, X = dev(rng.uniform(-2, 2, (m, d))), dev(rng.uniform(-2, 2, (n, d)))
    scale = dev(rng.uniform(0.5, 2.0, d))
    Kbar = torch.randn((m, n), dtype=torch.float64, device="cuda")
    amp, ls = dev(np.array([0.9])), dev(np.array([0.7]))
    Zs, Xs = linalg.scale_points(Z, scale), linalg.scale_points(X, scale)
    variants = {"isotropic": lambda: kernel_vjp(kind, Z, X, amp, ls, Kbar),
                "scaled": lambda: kernel_vjp(kind, Zs, Xs, amp, ls, Kbar, scale=scale)}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():  # alternating
            ms[k].append(_timed(fn))
    nbytes = 8.0 * (m * n + (m + n) * d)  # Kbar once, the points once
    out = {"shape": name, "M": m, "N": n, "d": d, "kind": kind, "algorithmic_bytes": nbytes}
    for k in variants:
        out[k] = _stats(ms[k])
        out[k]["TB_per_s"] = nbytes / (out[k]["median_ms"] * 1e-3) / 1e12
    out["ratio_scaled_over_isotropic"] = out["scaled"]["median_ms"] / out["isotropic"]["median_ms"]
    out["under_2x"] = out["ratio_scaled_over_isotropic"] < 2.0
    return out


def bench_step(reps, warmup, steps, batch=8192):
    X, y, Z = vgp_c5_data()
    N, d = X.shape
    Xd, yd = torch.as_tensor(X, device="cuda"), torch.as_tensor(y, device="cuda")
    rng = np.random.default_rng(1)
    idx = [torch.as_tensor(rng.integers(0, N, batch), device="cuda") for _ in range(steps)]
    ops = {"isotropic": vgp_c3_graph(X, y, Z, batch, kernel="matern52"),
           "feature_scaled": vgp_c3_graph(X, y, Z, batch, kernel="matern52",
                                          scale_diag=np.ones(d))}

    def run(k):
        op, _, xb, yb = ops[k]
        for i in idx:
            op.run({xb: Xd[i], yb: yd[i]})

    for _ in range(warmup):
        for k in ops:
            run(k)
    torch.cuda.synchronize()
    ms = {k: [] for k in ops}
    for _ in range(reps):
        for k in ops:  # alternating
            ms[k].append(_timed(lambda: run(k)) / steps)
    for op, *_ in ops.values():
        op.check()
    out = {"config": "C5", "N": N, "M": len(Z), "d": d, "batch": batch, "kind": "matern52",
           "steps_per_rep": steps}
    for k in ops:
        out[k] = {("ms_per_step_" + s[:-3] if s.endswith("_ms") else s): v
                  for s, v in _stats(ms[k]).items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5, help="VGP steps per timed repetition")
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "profiles", "ard_kernels.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")
    if not torch.cuda.is_available():
        sys.exit("bench_ard.py needs a GPU: nothing is measured without one")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "vjp": [bench_vjp("C5 Kzx", 1024, 65536, 5, "matern52", args.reps, args.warmup),
                   bench_vjp("C3 Kzx", 512, 262144, 3, "eq", args.reps, args.warmup)]}
    if not args.skip_step:
        res["vgp_step"] = bench_step(args.reps, args.warmup, args.steps)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
