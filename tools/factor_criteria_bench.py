#!/usr/bin/env python
"""Measure the passes over a factored Sigma = F F^T + diag(noise) and the placements on it
(csrc/criteria.hip, the vgposp_factor_symv / vgposp_critf entries) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4i into profiles/factor_criteria.json.  The
driver never opens the GPU; each stage is one child process under its own time limit, and a stage
that stops ends the run.  Nothing is fixed in advance: the tool records what it measures.

  stage "pass"   (n, S) = (65,536, 96), (65,536, 300), (262,144, 96), (262,144, 300), (2^21, 256):
                 time per vgposp_factor_symv launch (device events, two warm-ups, the median of
                 ``--reps`` launches with min and max; beside it the library's own ProfScope total
                 through prof_query) and 16 n S bytes over it; the same for the squared pass of the
                 init (three launches).  The factor goes from 50 MB to 4.3 GB, so the rates say
                 whether the second read of F is served by the 256 MiB Infinity Cache.  In the same
                 process: vgposp_symv_upper on the assembled 34 GB Sigma at n = 65,536 and the
                 SiteKernel pass (vgposp_kernel_symv, EQ, d = 3) at n = 65,536 and 262,144.
  stage "place"  50 picks by variance and by entropy at each shape but the first, on the samples of
                 examples/sample_placement.py's cosine field; at n = 65,536 also on the assembled
                 matrix: the same picks.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 1e-2
SHAPES = ((65536, 96), (65536, 300), (262144, 96), (262144, 300), (1 << 21, 256))
SITES = {65536: (64, 32, 32), 262144: (64, 64, 64), 1 << 21: (128, 128, 128)}


def _timing(torch):
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        s, e = ev(), ev()
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)
    return timed


def _launches(timed, fn, reps):
    for _ in range(2):
        fn()
    ms = [timed(fn) for _ in range(reps)]
    return {"ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def _factor(torch, n, S):
    """A random factor with rows of unit expected norm, filled in row chunks."""
    F = torch.empty((n, S), dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n + S)
    for r0 in range(0, n, 1 << 18):
        F[r0:r0 + (1 << 18)].normal_(0.0, S ** -0.5, generator=g)
    return F


def stage_pass(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    torch.cuda.set_device(0)
    timed = _timing(torch)
    out = {"reps": a.reps, "source_hash": _lib.source_hash("criteria_fsymv"), "shapes": []}
    for n, S in SHAPES:
        F = _factor(torch, n, S)
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        noise = torch.full((n,), NOISE, dtype=torch.float64, device="cuda")
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        ws = linalg.workspace(query("vgposp_factor_symv_workspace_bytes", n, S))
        rec = {"n": n, "S": S, "factor_bytes": 8.0 * n * S, "sigma_bytes": 8.0 * n * n,
               "workspace_bytes": ws.numel(), "pass_bytes": 16.0 * n * S}
        for name, reps in (("vgposp_factor_symv", a.reps), ("vgposp_factor_symv_sq", 3)):
            fn = lambda: call(name, _p(F), n, S, F.stride(0), _p(noise), _p(x), _p(y), _p(ws),
                              ws.numel(), _stream())
            r = _launches(timed, fn, reps)
            fam = "criteria_fsymv_sq" if name.endswith("_sq") else "criteria_fsymv"
            _lib.prof_enable(True)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            ms, launches, flops, nbytes = _lib.prof_query(fam)
            _lib.prof_enable(False)
            r["prof_scope_ms_per_launch"] = ms / max(launches, 1)
            if fam == "criteria_fsymv":
                r["bytes_per_s"] = 16.0 * n * S / (r["ms_median"] * 1e-3)
            else:
                r["flops_per_s"] = 4.0 * n * S * S / (r["ms_median"] * 1e-3)
            rec[name[7:]] = r
        if (n, S) == (65536, 300):   # the stored pass on the assembled matrix, the same product
            Sigma = torch.empty((n, n), dtype=torch.float64, device="cuda")
            linalg.gemm(F, F, Sigma, alpha=1.0, transb=True)
            torch.diagonal(Sigma).add_(noise)
            wsu = linalg.workspace(query("vgposp_symv_upper_workspace_bytes", n))
            yu = torch.empty(n, dtype=torch.float64, device="cuda")
            fn = lambda: call("vgposp_symv_upper", _p(Sigma), n, Sigma.stride(0), _p(None), _p(x),
                              _p(yu), _p(wsu), wsu.numel(), _stream())
            rec["symv_upper_stored"] = _launches(timed, fn, a.reps)
            call("vgposp_factor_symv", _p(F), n, S, F.stride(0), _p(noise), _p(x), _p(y), _p(ws),
                 ws.numel(), _stream())
            rec["max_diff_to_stored"] = float((y - yu).abs().max() / yu.abs().max())
            rec["over_stored"] = rec["factor_symv"]["ms_median"] \
                / rec["symv_upper_stored"]["ms_median"]
            del Sigma, wsu, yu
        if S == 300:                 # the generated pass of a SiteKernel at the same n
            X = torch.as_tensor(grid_points(SITES[n], jitter=0.05, seed=0), device="cuda")
            amp_t, ls_t = linalg._vec(1.0), linalg._vec(2.0 * grid_spacing(SITES[n]))
            wk = linalg.workspace(query("vgposp_kernel_symv_workspace_bytes", n))
            fn = lambda: call("vgposp_kernel_symv", KERNEL_KINDS["eq"], _p(X), n, 3, _p(amp_t),
                              _p(ls_t), _p(None), _p(None), _p(x), _p(y), _p(wk), wk.numel(),
                              _stream())
            rec["site_kernel_symv"] = _launches(timed, fn, 5)
            rec["over_site_kernel"] = rec["factor_symv"]["ms_median"] \
                / rec["site_kernel_symv"]["ms_median"]
            del X, wk
        out["shapes"].append(rec)
        del F, ws
        torch.cuda.empty_cache()
    return out


def stage_place(a):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from sample_placement import cosine_field_samples
    from vgposp_amd.covariance import empirical_cov
    from vgposp_amd.placement_criteria import CriterionPlacement, FactoredCovariance
    torch.cuda.set_device(0)
    timed = _timing(torch)
    out = {"k": a.k, "noise": NOISE, "runs": []}
    for n, S in SHAPES[1:]:
        T = cosine_field_samples(SITES[n], S)
        for criterion in ("variance", "entropy"):
            rec = {"n": n, "S": S, "criterion": criterion}
            for label in (("factored", "dense") if n == 65536 else ("factored",)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                t0 = time.perf_counter()
                if label == "dense":
                    cov = empirical_cov(T)
                    torch.diagonal(cov).add_(NOISE)
                else:
                    cov = FactoredCovariance.from_samples(T, noise=NOISE)
                g = CriterionPlacement(cov, a.k, criterion)
                g.run(a.k)
                torch.cuda.synchronize()
                first = time.perf_counter() - t0
                ms = [timed(lambda: g.run(a.k)) for _ in range(3)]
                picks, deltas = g.result()
                rec[label] = {"first_run_seconds_with_setup": first, "ms": ms,
                              "ms_median": statistics.median(ms),
                              "picks": [int(p) for p in picks],
                              "distinct_picks": len(set(int(p) for p in picks)),
                              "sum_of_deltas": float(deltas.sum()),
                              "held_bytes": torch.cuda.memory_allocated() - base,
                              "peak_bytes": torch.cuda.max_memory_allocated() - base,
                              "workspace_bytes": g.ws.numel()}
                del g, cov
            if "dense" in rec:
                rec["same_picks"] = rec["dense"]["picks"] == rec["factored"]["picks"]
            out["runs"].append(rec)
        del T
        torch.cuda.empty_cache()
    return out


def run_child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--k", str(a.k), "--reps",
           str(a.reps)]
    print(f"[factor_criteria_bench] stage {stage}, limit {limit:.0f} s ...", flush=True)
    try:
        p = subprocess.run(cmd, cwd=ROOT, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return None, f"no result within {limit:.0f} s"
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:]), None
    return None, f"exit status {p.returncode}: {p.stderr.strip()[-800:]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_criteria.json"))
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed launches (at least 5)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per stage")
    ap.add_argument("--child", choices=("pass", "place"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        res = stage_pass(a) if a.child == "pass" else stage_place(a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    res = {"tool": "tools/factor_criteria_bench.py", "stopped": None}
    # a stage that stops ends the run: nothing more is started on the device after it
    for stage in ("pass", "place"):
        res[stage], note = run_child(a, stage, a.limit)
        if res[stage] is None:
            res["stopped"] = f"{stage}: {note}"
            break
    if res["stopped"]:
        print(f"[factor_criteria_bench] stopped: {res['stopped']}", flush=True)
    print(f"[factor_criteria_bench] {json.dumps(res)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[factor_criteria_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
