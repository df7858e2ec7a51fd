#!/usr/bin/env python
"""Measure the matrix-free pass and the variance rule on a generated cross-covariance
(csrc/criteria.hip) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4g into profiles/matrix_free_criteria.json.
The driver never opens the GPU; each stage is one child process under its own time limit.

  stage "pass"   n = 4,096 sites (16^3), P = 262,144 targets (64^3), d = 3, EQ and Matern 5/2:
                 time per vgposp_kernel_gemv_t / _sq launch (device events, two warm-ups, the
                 median of ``--reps`` launches with min and max), entries/s, and with the VALU
                 instructions per entry read from the disassembly of the inner loop the share of
                 the fp64 VALU issue rate.  Two yardsticks in the same process, same method:
                 (a) vgposp_gemv_t on the assembled 8.6 GB R (the stored path);
                 (b) vgposp_kernel_matvec(X, Xt, x), the matrix-free product there was before
                     (16 workgroups at this n): the new pass must be faster, the ranges of the
                     launches must not overlap (``faster_than_kernel_matvec``).
                 Then 50 picks at that shape, matrix-free against stored: time and device memory.
  stage "large"  n = 16,384 sites (32 x 32 x 16) judged on the 128^3 mesh, k = 50, once: 51 passes
                 of P n = 3.4e10 entries whose stored R would be 275 GB.  Its time limit is
                 ``--setup`` seconds plus ``--margin`` times 51 P n over the entries/s the first
                 stage measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE, JITTER = 1e-2, 1e-6
KINDS = ("eq", "matern52")
# VALU instructions per generated entry in the main loop of kgemv_t_kernel<kind, 3, SQ> (hipcc -S
# for gfx950: the loop body handles two targets x one column pair, so its count over four)
VALU_PER_ENTRY = {("eq", False): 125 / 4, ("eq", True): 129 / 4,
                  ("matern52", False): 217 / 4, ("matern52", True): 221 / 4}
# fp64 VALU issue rate: 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz (the datasheet's
# 78.6 TFLOP/s of vector fp64 counts an fma as two)
FP64_LANE_OPS = 256 * 4 * 16 * 2.4e9


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


def stage_pass(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    from vgposp_amd.placement_criteria import CriterionPlacement, CrossKernel
    torch.cuda.set_device(0)
    timed = _timing(torch)

    def launches(fn):
        for _ in range(2):
            fn()
        ms = [timed(fn) for _ in range(a.reps)]
        return {"ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}

    sites, mesh, k = tuple(a.sites), tuple(a.mesh), a.k
    X = torch.as_tensor(grid_points(sites, jitter=0.05, seed=0), device="cuda")
    Xt = torch.as_tensor(grid_points(mesh, jitter=0.3, seed=1), device="cuda")
    ls = 2.0 * grid_spacing(sites)
    n, P, d = X.shape[0], Xt.shape[0], X.shape[1]
    amp_t, ls_t = linalg._vec(1.0), linalg._vec(ls)
    x = torch.randn(P, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = linalg.workspace(max(query("vgposp_kernel_gemv_t_workspace_bytes", P, n),
                              query("vgposp_gemv_t_workspace_bytes", P, n)))
    out = {"reps": a.reps, "n": n, "P": P, "d": d, "entries": float(P) * n,
           "stored_bytes": 8.0 * P * n, "points_bytes": 8.0 * (P + n) * d,
           "source_hash": _lib.source_hash("criteria_kgemv_t"), "kinds": {}}
    for kind in KINDS:
        kid = KERNEL_KINDS[kind]
        res = {}
        for name, sq in (("vgposp_kernel_gemv_t", False), ("vgposp_kernel_gemv_t_sq", True)):
            fn = lambda: call(name, kid, _p(Xt), P, _p(X), n, d, _p(amp_t), _p(ls_t), _p(None),
                              _p(None), _p(x), _p(y), _p(ws), ws.numel(), _stream())
            r = launches(fn)
            r["entries_per_s"] = P * n / (r["ms_median"] * 1e-3)
            r["valu_per_entry"] = VALU_PER_ENTRY[kind, sq]
            r["share_of_fp64_valu_issue"] = r["entries_per_s"] * r["valu_per_entry"] / FP64_LANE_OPS
            res[name[7:]] = r
        got = y.clone()
        # (b) the matrix-free product there was: out[j] = sum_v K(X_j, Xt_v) x_v
        yb = torch.empty(n, dtype=torch.float64, device="cuda")
        fn = lambda: call("vgposp_kernel_matvec", kid, _p(X), n, _p(Xt), P, d, _p(amp_t),
                          _p(ls_t), _p(x), 0.0, _p(yb), _stream())
        res["kernel_matvec"] = launches(fn)
        # (a) the stored path on the assembled R
        R = linalg.kernel_matrix(kind, Xt, X, 1.0, ls)[0]
        ya = torch.empty(n, dtype=torch.float64, device="cuda")
        fn = lambda: call("vgposp_gemv_t", _p(R), P, n, R.stride(0), _p(x), _p(ya), _p(ws),
                          ws.numel(), _stream())
        res["gemv_t_stored"] = launches(fn)
        res["gemv_t_stored"]["tbps"] = 8.0 * P * n / res["gemv_t_stored"]["ms_median"] / 1e9
        # the pass against both (sq form last launched: compare the plain form again)
        call("vgposp_kernel_gemv_t", kid, _p(Xt), P, _p(X), n, d, _p(amp_t), _p(ls_t), _p(None),
             _p(None), _p(x), _p(got), _p(ws), ws.numel(), _stream())
        scale = float(ya.abs().max())
        res["max_diff_to_stored"] = float((got - ya).abs().max()) / scale
        res["max_diff_to_kernel_matvec"] = float((got - yb).abs().max()) / scale
        new, old = res["kernel_gemv_t"], res["kernel_matvec"]
        res["over_stored"] = new["ms_median"] / res["gemv_t_stored"]["ms_median"]
        res["kernel_matvec_over_new"] = old["ms_median"] / new["ms_median"]
        res["faster_than_kernel_matvec"] = bool(new["ms_max"] < old["ms_min"])
        out["kinds"][kind] = res
        del R, ya, yb
        torch.cuda.empty_cache()
    # ---- 50 picks, matrix-free against stored (EQ) ----
    S = linalg.kernel_matrix("eq", X, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
    base = torch.cuda.memory_allocated()
    runs = {}
    for label in ("matrix_free", "stored"):
        torch.cuda.reset_peak_memory_stats()
        if label == "stored":
            kw = {"cross_cov": linalg.kernel_matrix("eq", Xt, X, 1.0, ls)[0]}
        else:
            kw = {"cross_kernel": CrossKernel("eq", X, Xt, 1.0, ls)}
        g = CriterionPlacement(S, k, "variance", **kw)
        g.run(k)                                                   # warm-up
        ms = [timed(lambda: g.run(k)) for _ in range(3)]
        picks, deltas = g.result()
        runs[label] = {"ms": ms, "ms_median": statistics.median(ms),
                       "picks": [int(p) for p in picks], "sum_of_deltas": float(deltas.sum()),
                       "held_bytes": torch.cuda.memory_allocated() - base,
                       "peak_bytes": torch.cuda.max_memory_allocated() - base}
        del g, kw
        torch.cuda.empty_cache()
    runs["same_picks"] = runs["matrix_free"]["picks"] == runs["stored"]["picks"]
    runs["k"] = k
    out["placement"] = runs
    return out


def stage_large(a):
    import torch
    from vgposp_amd import linalg
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_criteria import CriterionPlacement, CrossKernel
    torch.cuda.set_device(0)
    sites, mesh, k = tuple(a.large_sites), tuple(a.large_mesh), a.k
    X = torch.as_tensor(grid_points(sites, jitter=0.05, seed=0), device="cuda")
    Xt = torch.as_tensor(grid_points(mesh, jitter=0.3, seed=1), device="cuda")
    ls = 2.0 * grid_spacing(sites)
    n, P = X.shape[0], Xt.shape[0]
    S = linalg.kernel_matrix("eq", X, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    g = CriterionPlacement(S, k, "variance", cross_kernel=CrossKernel("eq", X, Xt, 1.0, ls))
    g.run(k)
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    picks, deltas = g.result()
    return {"n": n, "P": P, "k": k, "passes": k + 1, "entries_per_pass": float(P) * n,
            "stored_bytes": 8.0 * P * n, "seconds": seconds,
            "entries_per_s": (k + 1) * float(P) * n / seconds,
            "peak_bytes": torch.cuda.max_memory_allocated(),
            "sigma_bytes": 8.0 * n * n, "picks": [int(p) for p in picks],
            "distinct_picks": len(set(int(p) for p in picks)),
            "sum_of_deltas": float(deltas.sum()),
            "mean_variance_removed": float(g.variance_removed().mean())}


def run_child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--k", str(a.k), "--reps",
           str(a.reps)]
    for flag in ("sites", "mesh", "large_sites", "large_mesh"):
        cmd += ["--" + flag.replace("_", "-")] + [str(s) for s in getattr(a, flag)]
    print(f"[matrix_free_criteria_bench] stage {stage}, limit {limit:.0f} s ...", flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "matrix_free_criteria.json"))
    ap.add_argument("--sites", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--mesh", type=int, nargs=3, default=[64, 64, 64])
    ap.add_argument("--large-sites", type=int, nargs=3, default=[32, 32, 16])
    ap.add_argument("--large-mesh", type=int, nargs=3, default=[128, 128, 128])
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed launches (at least 5)")
    ap.add_argument("--limit", type=int, default=420, help="seconds for the first stage")
    ap.add_argument("--setup", type=float, default=120.0,
                    help="seconds allowed to the large stage besides its passes (start-up, "
                         "assembling Sigma, the mesh)")
    ap.add_argument("--margin", type=float, default=4.0,
                    help="the large stage's passes may take this many times their predicted time")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--child", choices=("pass", "large"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        res = stage_pass(a) if a.child == "pass" else stage_large(a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    res = {"tool": "tools/matrix_free_criteria_bench.py", "pass": None, "large": None,
           "stopped": None}
    res["pass"], note = run_child(a, "pass", a.limit)
    if res["pass"] is None:
        res["stopped"] = "pass: " + note
    elif not a.skip_large:
        eps = res["pass"]["kinds"]["eq"]["kernel_gemv_t"]["entries_per_s"]
        n = a.large_sites[0] * a.large_sites[1] * a.large_sites[2]
        P = a.large_mesh[0] * a.large_mesh[1] * a.large_mesh[2]
        predicted = (a.k + 1) * float(P) * n / eps
        limit = a.setup + a.margin * predicted
        res["large_limit"] = {"entries_per_s": eps, "predicted_pass_seconds": predicted,
                              "setup_seconds": a.setup, "margin": a.margin, "seconds": limit}
        res["large"], note = run_child(a, "large", limit)
        if res["large"] is None:
            res["stopped"] = "large: " + note
    if res["stopped"]:
        print(f"[matrix_free_criteria_bench] stopped: {res['stopped']}", flush=True)
    print(f"[matrix_free_criteria_bench] {json.dumps(res)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[matrix_free_criteria_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
