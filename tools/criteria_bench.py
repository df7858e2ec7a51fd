#!/usr/bin/env python
"""Measure the variance-reduction and entropy placements (csrc/criteria.hip) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4e into profiles/criteria_placement.json.
On the placement benchmark's workload (workloads.placement_split, 64 x 32 x 32 -> N = 65,536,
k = 50), in one child process under its own time limit (the driver never opens the GPU):

  symv       time per vgposp_symv_upper launch (device events, warm-up, the median of ``--reps``
             launches) and its rate on the algorithmic bytes 8 n (n + 1) / 2; the same for the
             squared pass of the initial score, and for the pass on the buffer the MI path
             factored in place (diag = the saved diagonal).
  yardstick  in the same process, the library's own per-launch timing (prof_query) of the
             column-norm pass greedy_trmv_kernel<true> ("greedy_colsq") of the MI init, and of
             "criteria_symv" by the same method, both over their algorithmic bytes.
  rounds     the whole k picks of each rule (init included) beside the MI rounds, and the MI
             factorization + inverse.
  variance   the mean posterior variance of the noisy field over all locations that each rule's
             picks leave (nom of a CriterionPlacement conditioned on the picks).
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
    from vgposp_amd.linalg import _p, _stream
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    from vgposp_amd.placement_criteria import CriterionPlacement
    from vgposp_amd.workloads import placement_split
    torch.cuda.set_device(0)
    shape, k = tuple(a.shape), a.k
    Xh, ls = placement_split(shape, 0)
    X = torch.as_tensor(Xh, device="cuda")
    N = len(Xh)
    S = linalg.kernel_matrix("eq", X, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
    tri = 8.0 * N * (N + 1) / 2
    ev = lambda: torch.cuda.Event(enable_timing=True)

    def timed(fn):
        torch.cuda.synchronize()
        s, e = ev(), ev()
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    ws = linalg.workspace(query("vgposp_symv_upper_workspace_bytes", N))
    x = torch.randn(N, dtype=torch.float64, device="cuda")
    y = torch.empty(N, dtype=torch.float64, device="cuda")

    def symv(name, diag=None):
        fn = lambda: call(name, _p(S), N, S.stride(0), _p(diag), _p(x), _p(y), _p(ws), ws.numel(),
                          _stream())
        for _ in range(2):
            fn()
        ms = [timed(fn) for _ in range(a.reps)]
        med = statistics.median(ms)
        return {"ms": ms, "ms_median": med, "spread": (max(ms) - min(ms)) / med,
                "tbps_algorithmic": tri / med / 1e9}

    out = {"N": N, "k": k, "shape": list(shape), "reps": a.reps, "tri_bytes": tri,
           "source_hash": _lib.source_hash("criteria_symv")}
    out["symv_upper"] = symv("vgposp_symv_upper")
    out["symv_upper_sq"] = symv("vgposp_symv_upper_sq")

    def rule(criterion, diag=None):
        g = CriterionPlacement(S, k, criterion, diag=diag)
        g.run(k)                                                   # warm-up
        ms = [timed(lambda: g.run(k)) for _ in range(3)]
        picks, deltas = g.result()
        return g, {"ms": ms, "ms_median": statistics.median(ms),
                   "picks": [int(p) for p in picks], "sum_of_deltas": float(deltas.sum())}

    picks = {}
    for criterion in ("variance", "entropy"):
        g, out[criterion] = rule(criterion)
        picks[criterion] = out[criterion]["picks"]
        del g
    # the MI path on the same buffer, factored in place; its column-norm pass is the yardstick
    diag = torch.diagonal(S).clone()
    mi = GreedyPlacement(S, k)
    _lib.prof_enable(True)
    init_ms = timed(mi.init)
    mi.check()
    ms, cnt, _, by = _lib.prof_query("greedy_colsq")
    _lib.prof_enable(False)
    out["yardstick_greedy_colsq"] = {"ms": ms, "launches": cnt, "algorithmic_bytes": by,
                                     "tbps_algorithmic": by / ms / 1e9}
    step_ms = timed(lambda: [mi.step(True) for _ in range(k)])
    picks["mi"] = [int(p) for p in mi.result()[0]]
    out["mi"] = {"factor_inverse_init_ms": init_ms, "rounds_ms": step_ms,
                 "ms_per_round": step_ms / k, "picks": picks["mi"]}
    # the factored buffer: the same pass with diag, by events and by the library's own timing
    out["symv_upper_factored"] = symv("vgposp_symv_upper", diag)
    _lib.prof_enable(True)
    for _ in range(a.reps):
        call("vgposp_symv_upper", _p(S), N, S.stride(0), _p(diag), _p(x), _p(y), _p(ws),
             ws.numel(), _stream())
    torch.cuda.synchronize()
    ms, cnt, _, by = _lib.prof_query("criteria_symv")
    _lib.prof_enable(False)
    out["symv_upper_prof"] = {"ms": ms, "launches": cnt, "algorithmic_bytes": by,
                              "tbps_algorithmic": by / ms / 1e9}
    out["symv_over_yardstick"] = (out["symv_upper_prof"]["tbps_algorithmic"]
                                  / out["yardstick_greedy_colsq"]["tbps_algorithmic"])
    g, fact = rule("variance", diag)
    out["variance_on_factored_buffer"] = {"ms_median": fact["ms_median"],
                                          "picks_equal": fact["picks"] == picks["variance"],
                                          "sum_of_deltas_equal":
                                              fact["sum_of_deltas"] == out["variance"]["sum_of_deltas"]}
    del g
    # what each rule's picks leave: mean of C_yy over all locations
    prior = float(diag.mean())
    out["mean_posterior_variance"] = {"prior": prior}
    for name, A in picks.items():
        c = CriterionPlacement(S, 1, "entropy", placed=A, diag=diag).init()
        nom = c.state()["nom"]
        out["mean_posterior_variance"][name] = float(nom.mean())
        out["mean_posterior_variance"][name + "_max"] = float(nom.max())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "criteria_placement.json"))
    ap.add_argument("--shape", type=int, nargs=3, default=[64, 32, 32])
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
           str(a.reps), "--shape"] + [str(s) for s in a.shape]
    res = {"tool": "tools/criteria_bench.py", "result": None, "stopped": None}
    print(f"[criteria_bench] shape {a.shape}, k = {a.k} ...", flush=True)
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
        print(f"[criteria_bench] stopped: {note}", flush=True)
    else:
        print(f"[criteria_bench] {json.dumps(res['result'])}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[criteria_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
