#!/usr/bin/env python
"""Measure the mutual-information placement on a factored Sigma = F F^T + D (csrc/criteria.hip, the
vgposp_fmi entries) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4l into profiles/factor_mi.json.  The driver
never opens the GPU; each stage is one child process under its own time limit, and a stage that
stops ends the run.  Nothing is fixed in advance: the tool records what it measures.  Every time is
from device events (the library's ProfScope pairs for a single kernel, torch events around a whole
call), after two warm-ups, as the median of ``--reps`` with min and max; where two sides are
compared they alternate in one process.

  stage "row"    (n, S) = (65,536, 300), (262,144, 96), (262,144, 300), (2^21, 256): the fused
                 two-right-hand-side row stream of a round (scope criteria_fmi_row, round 3)
                 against the single-vector stream the rounds of vgposp_critf_step run on the same
                 factor (factor_row_kernel in its column form: one dot per row and the W downdate,
                 scope criteria_row, round 3), counted twice: what two single-vector passes for
                 s and q would cost.  Both as rates over their byte models.
  stage "init"   vgposp_fmi_init (its scope, and the GEMM launches inside it) beside
                 vgposp_factor_symv_sq, which runs the same two chunked GEMM sweeps.
  stage "place"  50 picks on the samples of examples/sample_placement.py's cosine field: time and
                 device memory held; at n = 65,536, S = 300 also GreedyPlacement on the assembled
                 34 GB matrix, full greedy, from the same process: its factorization and rounds,
                 whether the 50 picks are equal, the worst pick-delta difference and the smallest
                 gap between the best and the second-best delta of the dense rounds.
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 1e-2
SHAPES = ((65536, 300), (262144, 96), (262144, 300), (1 << 21, 256))
SITES = {65536: (64, 32, 32), 262144: (64, 64, 64), 1 << 21: (128, 128, 128)}
ROUND = 3


def _stats(ms):
    return {"ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


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


def _factor(torch, n, S):
    """A random factor with rows of unit expected norm, filled in row chunks."""
    F = torch.empty((n, S), dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n + S)
    for r0 in range(0, n, 1 << 18):
        F[r0:r0 + (1 << 18)].normal_(0.0, S ** -0.5, generator=g)
    return F


def _scoped(torch, _lib, fn, scopes):
    """One call of fn under the library's per-launch events: {scope: ms}."""
    _lib.prof_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {s: _lib.prof_query(s)[0] for s in scopes}
    finally:
        _lib.prof_enable(False)


def stage_row(a):
    import torch
    from vgposp_amd import _lib
    from vgposp_amd import placement_criteria as PC
    torch.cuda.set_device(0)
    out = {"reps": a.reps, "round": ROUND, "source_hash": _lib.source_hash("criteria_fmi_row"),
           "shapes": []}
    for n, S in SHAPES:
        fac = PC.FactoredCovariance(_factor(torch, n, S), noise=NOISE)
        mi = PC.FactoredMIPlacement(fac, ROUND + 1).init()
        en = PC.CriterionPlacement(fac, ROUND + 1, "entropy").init()
        for r in range(ROUND):
            mi._step(r)
            en._step(r)
        fused, single = [], []
        for i in range(2 + a.reps):           # the same round again and again, sides alternated
            f = _scoped(torch, _lib, lambda: mi._step(ROUND), ["criteria_fmi_row"])
            s = _scoped(torch, _lib, lambda: en._step(ROUND), ["criteria_row"])
            if i >= 2:
                fused.append(f["criteria_fmi_row"])
                single.append(s["criteria_row"])
        fb = 8.0 * n * S + 8.0 * n * (2 * ROUND + 6)
        sb = 8.0 * n * S + 8.0 * n * (5 + ROUND)
        rec = {"n": n, "S": S, "factor_bytes": 8.0 * n * S, "fused": _stats(fused),
               "single": _stats(single), "fused_bytes": fb, "two_pass_bytes": 2 * sb}
        rec["fused"]["bytes_per_s"] = fb / (rec["fused"]["ms_median"] * 1e-3)
        rec["single"]["bytes_per_s"] = sb / (rec["single"]["ms_median"] * 1e-3)
        rec["two_pass_ms_median"] = 2.0 * rec["single"]["ms_median"]
        rec["fused_over_two_pass"] = rec["fused"]["ms_median"] / rec["two_pass_ms_median"]
        out["shapes"].append(rec)
        del mi, en, fac
        torch.cuda.empty_cache()
    large = [r for r in out["shapes"] if r["n"] >= 262144]
    out["fused_faster_at_the_three_large_shapes"] = all(r["fused_over_two_pass"] < 1.0
                                                        for r in large)
    return out


def stage_init(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd import placement_criteria as PC
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    torch.cuda.set_device(0)
    timed = _timing(torch)
    out = {"reps": a.reps, "kmax": a.k, "shapes": []}
    for n, S in SHAPES:
        fac = PC.FactoredCovariance(_factor(torch, n, S), noise=NOISE)
        mi = PC.FactoredMIPlacement(fac, a.k)
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        ws = linalg.workspace(query("vgposp_factor_symv_workspace_bytes", n, S))
        sq = lambda: call("vgposp_factor_symv_sq", *fac.args(), _p(x), _p(y), _p(ws), ws.numel(),
                          _stream())
        init, symv_sq = [], []
        for i in range(2 + a.reps):
            t0, t1 = timed(mi.init), timed(sq)
            if i >= 2:
                init.append(t0)
                symv_sq.append(t1)
        scopes = _scoped(torch, _lib, mi.init, ["criteria_fmi_init", "gemm_f64", "row_sumsq"])
        mi.check()
        rec = {"n": n, "S": S, "init": _stats(init), "factor_symv_sq": _stats(symv_sq),
               "init_scope_ms": scopes["criteria_fmi_init"], "init_gemm_ms": scopes["gemm_f64"],
               "init_row_sumsq_ms": scopes["row_sumsq"], "workspace_bytes": mi.ws.numel(),
               "init_flops": 4.0 * n * S * S + 8.0 * S ** 3 / 3.0}
        rec["init"]["flops_per_s"] = rec["init_flops"] / (rec["init"]["ms_median"] * 1e-3)
        rec["init_over_symv_sq"] = rec["init"]["ms_median"] / rec["factor_symv_sq"]["ms_median"]
        out["shapes"].append(rec)
        del mi, fac, ws
        torch.cuda.empty_cache()
    return out


def _dense_deltas(torch, g):
    from vgposp_amd._lib import call
    from vgposp_amd.linalg import _p
    d = ctypes.c_void_p()
    call("vgposp_greedy_buffers", _p(g.ws), g.n, g.kmax, ctypes.byref(d), None, None)
    off = d.value - g.ws.data_ptr()
    return g.ws[off:off + 8 * g.n].view(torch.float64)


def stage_place(a):
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    from sample_placement import cosine_field_samples
    from vgposp_amd.covariance import empirical_cov
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    from vgposp_amd.placement_criteria import FactoredCovariance, FactoredMIPlacement
    torch.cuda.set_device(0)
    timed = _timing(torch)
    out = {"k": a.k, "noise": NOISE, "runs": []}
    for n, S in SHAPES:
        T = cosine_field_samples(SITES[n], S)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        fac = FactoredCovariance.from_samples(T, noise=NOISE)
        g = FactoredMIPlacement(fac, a.k)
        g.run(a.k)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        runs = [timed(lambda: g.run(a.k)) for _ in range(3)]
        inits = [timed(g.init) for _ in range(3)]
        picks, deltas = g.run(a.k).result()
        rec = {"n": n, "S": S, "first_run_seconds_with_setup": first, "run": _stats(runs),
               "init": _stats(inits), "picks": [int(p) for p in picks],
               "distinct_picks": len(set(int(p) for p in picks)), "info": int(g.info[0]),
               "sum_of_deltas": float(deltas.sum()),
               "held_bytes": torch.cuda.memory_allocated() - base,
               "peak_bytes": torch.cuda.max_memory_allocated() - base,
               "factor_bytes": 8 * n * S, "workspace_bytes": g.ws.numel(),
               "sigma_bytes_never_allocated": 8 * n * n}
        rec["rounds_ms_median"] = rec["run"]["ms_median"] - rec["init"]["ms_median"]
        if (n, S) == (65536, 300):   # the dense path on the assembled matrix, full greedy
            Sigma = empirical_cov(T)
            torch.diagonal(Sigma).add_(NOISE)
            d = GreedyPlacement(Sigma, a.k)
            init_ms = timed(d.init)
            d.check()
            taken = np.zeros(n, dtype=bool)
            step_ms, gaps = [], []
            for r in range(a.k):
                step_ms.append(timed(lambda: d.step(lazy=False)))
                dv = _dense_deltas(torch, d).cpu().numpy()
                top = np.sort(dv[~taken])[::-1]
                gaps.append(float((top[0] - top[1]) / abs(top[0])))
                taken[int(d.selected[r])] = True
            dp, dd, _ = d.result()
            dp = [int(p) for p in dp]
            same = next((r for r in range(a.k) if dp[r] != rec["picks"][r]), a.k)
            diff = [abs(float(deltas[r]) - float(dd[r])) / abs(float(dd[r])) for r in range(same)]
            rec["dense"] = {"init_ms": init_ms, "rounds_ms": sum(step_ms), "picks": dp,
                            "workspace_bytes": d.ws.numel(), "smallest_gap": min(gaps),
                            "gaps": gaps, "same_picks": same == a.k, "equal_leading_picks": same,
                            "worst_pick_delta_difference": max(diff) if diff else None}
            del d, Sigma
        out["runs"].append(rec)
        del g, fac, T
        torch.cuda.empty_cache()
    return out


STAGES = {"row": stage_row, "init": stage_init, "place": stage_place}


def run_child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--k", str(a.k), "--reps",
           str(a.reps)]
    print(f"[factor_mi_bench] stage {stage}, limit {limit:.0f} s ...", flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_mi.json"))
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions (at least 5)")
    ap.add_argument("--limit", type=int, default=240, help="seconds per stage")
    ap.add_argument("--child", choices=tuple(STAGES))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(STAGES[a.child](a)), flush=True)
        return 0
    res = {"tool": "tools/factor_mi_bench.py", "stopped": None}
    # a stage that stops ends the run: nothing more is started on the device after it
    for stage in STAGES:
        res[stage], note = run_child(a, stage, a.limit)
        if res[stage] is None:
            res["stopped"] = f"{stage}: {note}"
            break
    if res["stopped"]:
        print(f"[factor_mi_bench] stopped: {res['stopped']}", flush=True)
    print(f"[factor_mi_bench] {json.dumps(res)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[factor_mi_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
