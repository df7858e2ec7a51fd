#!/usr/bin/env python
"""Measure the rectangular pass and the cross-covariance variance rule (csrc/criteria.hip) on one
MI355X.

Not bench.py: this records the figures behind DESIGN §4f into profiles/cross_criteria.json, in one
child process under its own time limit (the driver never opens the GPU):

  gemv_t     time per vgposp_gemv_t / vgposp_gemv_t_sq launch (device events, two warm-ups, the
             median of ``--reps`` launches) at P x n = 131,072 x 16,384 and its rate on the
             algorithmic bytes 8 P n (17.18 GB: the bytes of the N = 65,536 triangle).
  symv       in the same process and by the same method, vgposp_symv_upper on the placement
             benchmark's workload (workloads.placement_split, 64 x 32 x 32 -> N = 65,536) over
             8 N (N + 1) / 2 bytes; ``gemv_t_over_symv`` is the ratio of the two rates (expected
             >= 0.95: the rectangular pass has no cross-lane row reduction).  Both also by the
             library's own per-launch timing of the streaming kernel alone (prof_query).
  placement  50 picks at n = 4,096 sites (16^3) judged at P = 262,144 targets (64^3): the whole
             run (init included), and the share of the 51 passes over R in it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE, JITTER = 1e-2, 1e-6


def child(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd._lib import call, query
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    from vgposp_amd.placement_criteria import CriterionPlacement
    from vgposp_amd.workloads import placement_split
    torch.cuda.set_device(0)
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        s, e = ev(), ev()
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    def launches(fn, nbytes, prof_name):
        for _ in range(2):
            fn()
        ms = [timed(fn) for _ in range(a.reps)]
        med = statistics.median(ms)
        _lib.prof_enable(True)
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        pms, cnt, _, by = _lib.prof_query(prof_name)
        _lib.prof_enable(False)
        return {"ms": ms, "ms_median": med, "spread": (max(ms) - min(ms)) / med,
                "tbps_algorithmic": nbytes / med / 1e9,
                "prof": {"ms": pms, "launches": cnt, "algorithmic_bytes": by,
                         "tbps_algorithmic": by / pms / 1e9}}

    out = {"reps": a.reps, "source_hash": _lib.source_hash("criteria_gemv_t")}
    # ---- the rectangular pass ----
    P, n = a.gemv
    R = torch.randn((P, n), dtype=torch.float64, device="cuda")
    x = torch.randn(P, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = linalg.workspace(query("vgposp_gemv_t_workspace_bytes", P, n))
    out["gemv_shape"] = [P, n]
    out["gemv_bytes"] = 8.0 * P * n
    for name, prof in (("vgposp_gemv_t", "criteria_gemv_t"),
                       ("vgposp_gemv_t_sq", "criteria_gemv_t_sq")):
        fn = lambda: call(name, _p(R), P, n, R.stride(0), _p(x), _p(y), _p(ws), ws.numel(),
                          _stream())
        out[name[7:]] = launches(fn, 8.0 * P * n, prof)
    del R, x, y, ws
    torch.cuda.empty_cache()
    # ---- the triangle of the placement benchmark's workload, same process, same method ----
    Xh, ls = placement_split(tuple(a.shape), 0)
    N = len(Xh)
    S = linalg.kernel_matrix("eq", torch.as_tensor(Xh, device="cuda"), None, 1.0, ls,
                             diag_shift=NOISE + JITTER)[0]
    x = torch.randn(N, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")
    ws = linalg.workspace(query("vgposp_symv_upper_workspace_bytes", N))
    tri = 8.0 * N * (N + 1) / 2
    fn = lambda: call("vgposp_symv_upper", _p(S), N, S.stride(0), _p(None), _p(x), _p(y), _p(ws),
                      ws.numel(), _stream())
    out["N"], out["tri_bytes"] = N, tri
    out["symv_upper"] = launches(fn, tri, "criteria_symv")
    del S, x, y, ws
    torch.cuda.empty_cache()
    for key in ("gemv_t", "gemv_t_sq"):
        out[key + "_over_symv"] = (out[key]["tbps_algorithmic"]
                                   / out["symv_upper"]["tbps_algorithmic"])
        out[key + "_over_symv_prof"] = (out[key]["prof"]["tbps_algorithmic"]
                                        / out["symv_upper"]["prof"]["tbps_algorithmic"])
    # ---- 50 picks on coarse sites judged on a fine mesh ----
    sites, mesh, k = tuple(a.sites), tuple(a.mesh), a.k
    X = torch.as_tensor(grid_points(sites, jitter=0.05, seed=0), device="cuda")
    Xt = torch.as_tensor(grid_points(mesh, jitter=0.3, seed=1), device="cuda")
    ls = 2.0 * grid_spacing(sites)
    S = linalg.kernel_matrix("eq", X, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
    R = linalg.kernel_matrix("eq", Xt, X, 1.0, ls)[0]
    g = CriterionPlacement(S, k, "variance", cross_cov=R)
    g.run(k)                                                   # warm-up
    ms = [timed(lambda: g.run(k)) for _ in range(3)]
    picks, deltas = g.result()
    _lib.prof_enable(True)
    g.run(k)
    torch.cuda.synchronize()
    pass_ms, cnt = 0.0, 0
    for prof in ("criteria_gemv_t", "criteria_gemv_t_sq"):
        pms, c, _, _ = _lib.prof_query(prof)
        pass_ms, cnt = pass_ms + pms, cnt + c
    _lib.prof_enable(False)
    total = statistics.median(ms)
    out["placement"] = {"n": int(S.shape[0]), "P": int(R.shape[0]), "k": k,
                        "pass_bytes": 8.0 * R.shape[0] * R.shape[1], "ms": ms,
                        "ms_median": total, "passes": cnt, "passes_ms": pass_ms,
                        "passes_share": pass_ms / total,
                        "ms_per_pass": pass_ms / max(cnt, 1),
                        "picks": [int(p) for p in picks],
                        "sum_of_deltas": float(deltas.sum()),
                        "mean_variance_removed": float(g.variance_removed().mean())}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_criteria.json"))
    ap.add_argument("--gemv", type=int, nargs=2, default=[131072, 16384], metavar=("P", "n"))
    ap.add_argument("--shape", type=int, nargs=3, default=[64, 32, 32],
                    help="grid of the symv workload")
    ap.add_argument("--sites", type=int, nargs=3, default=[16, 16, 16])
    ap.add_argument("--mesh", type=int, nargs=3, default=[64, 64, 64])
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed launches (at least 5)")
    ap.add_argument("--limit", type=int, default=420, help="seconds for the GPU step")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(child(a)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--k", str(a.k), "--reps",
           str(a.reps)]
    for flag in ("gemv", "shape", "sites", "mesh"):
        cmd += ["--" + flag] + [str(s) for s in getattr(a, flag)]
    res = {"tool": "tools/cross_criteria_bench.py", "result": None, "stopped": None}
    print(f"[cross_criteria_bench] gemv {a.gemv}, symv grid {a.shape}, sites {a.sites}, "
          f"mesh {a.mesh}, k = {a.k} ...", flush=True)
    try:
        p = subprocess.run(cmd, cwd=ROOT, timeout=a.limit, capture_output=True, text=True)
        for line in p.stdout.splitlines():
            if line.startswith("RESULT "):
                res["result"] = json.loads(line[7:])
        note = f"exit status {p.returncode}: {p.stderr.strip()[-800:]}"
    except subprocess.TimeoutExpired:
        note = f"no result within {a.limit} s"
    if res["result"] is None:
        res["stopped"] = note
        print(f"[cross_criteria_bench] stopped: {note}", flush=True)
    else:
        print(f"[cross_criteria_bench] {json.dumps(res['result'])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[cross_criteria_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
