#!/usr/bin/env python
"""Measure the pass over a generated Sigma and the placements on it (csrc/criteria.hip) on one
MI355X.

Not bench.py: this records the figures behind DESIGN §4h into profiles/site_kernel_criteria.json.
The driver never opens the GPU; each stage is one child process under its own time limit.

  stage "pass"     n = 65,536 (64 x 32 x 32) and n = 262,144 (64^3), d = 3, EQ and Matern 5/2: time
                   per vgposp_kernel_symv launch (device events, two warm-ups, the median of
                   ``--reps`` launches with min and max) against the yardstick
                   vgposp_kernel_gemv_t with Xt = X, the full-square generation of the same
                   product, in the same process: the new pass must be faster with ranges that do
                   not overlap (``faster_than_full_square``).  The ratio is recorded beside the one
                   the main loops' instruction counts predict, (E + rho) / (2 E).  At n = 65,536
                   also vgposp_symv_upper on the assembled 34 GB Sigma, the stored pass over the
                   same triangle.
  stage "place"    50 picks by variance at n = 65,536, matrix-free against dense: picks, time,
                   device memory.
  stage "large"    50 picks by variance at n = 262,144 (64^3), where no dense run exists.  Its
                   time limit is ``--setup`` seconds plus ``--margin`` times 51 n^2 / 2 entries
                   over the rate the first stage measured.
  stage "entropy"  50 picks by entropy at n = 2^21 (128^3): one generated column per round.
  stage "pass2m"   one variance pass at n = 2^21, run only if n^2 / 2 over the measured rate is
                   below ``--pass2m-max`` seconds; limited as the large stage is.
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
# VALU instructions of the main loops at d = 3 (hipcc -S for gfx950).  E: per generated entry,
# kgemv_t_kernel<kind, 3, false> (its body: two targets x one column pair).  The new kernel's loop
# body is two rows x eight columns and the halving exchange of their partials; eight rows share
# the rest of the transpose-reduce and the update of the row sums.  ENTRY_NEW: its instructions per
# entry towards both outputs; RHO: the row-direction share of them (the second fma, the exchanges,
# the butterflies), per entry.
E_FULL = {"eq": 125 / 4, "matern52": 217 / 4}
# ksymv_kernel<kind, 3, false>: 521 (EQ) / 889 (Matern 5/2) VALU instructions in the two-row body,
# 35 more per eight rows
ENTRY_NEW = {"eq": (4 * 521 + 35) / 64, "matern52": (4 * 889 + 35) / 64}
# of which per two-row body 16 fmas, the two swaps, an add and three moves; and the 35
RHO = {"eq": (4 * 22 + 35) / 64, "matern52": (4 * 22 + 35) / 64}
SIZES = {"65536": (64, 32, 32), "262144": (64, 64, 64)}


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


def stage_pass(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    torch.cuda.set_device(0)
    timed = _timing(torch)
    out = {"reps": a.reps, "d": 3, "source_hash": _lib.source_hash("criteria_ksymv"),
           "e_full": E_FULL, "entry_new": ENTRY_NEW, "rho": RHO, "sizes": {}}
    for label, shape in SIZES.items():
        X = torch.as_tensor(grid_points(shape, jitter=0.05, seed=0), device="cuda")
        n, d = X.shape
        ls = 2.0 * grid_spacing(shape)
        amp_t, ls_t = linalg._vec(1.0), linalg._vec(ls)
        diag = torch.full((n,), 1.0 + NOISE + JITTER, dtype=torch.float64, device="cuda")
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        yf = torch.empty(n, dtype=torch.float64, device="cuda")
        ws = linalg.workspace(max(query("vgposp_kernel_symv_workspace_bytes", n),
                                  query("vgposp_kernel_gemv_t_workspace_bytes", n, n)))
        size = {"n": n, "triangle_entries": 0.5 * n * n, "square_entries": float(n) * n,
                "workspace_bytes": query("vgposp_kernel_symv_workspace_bytes", n), "kinds": {}}
        for kind in KINDS:
            kid = KERNEL_KINDS[kind]
            res = {}
            for name in ("vgposp_kernel_symv", "vgposp_kernel_symv_sq"):
                fn = lambda: call(name, kid, _p(X), n, d, _p(amp_t), _p(ls_t), _p(None), _p(diag),
                                  _p(x), _p(y), _p(ws), ws.numel(), _stream())
                r = _launches(timed, fn, a.reps)
                r["triangle_entries_per_s"] = 0.5 * n * n / (r["ms_median"] * 1e-3)
                res[name[7:]] = r
            call("vgposp_kernel_symv", kid, _p(X), n, d, _p(amp_t), _p(ls_t), _p(None), _p(diag),
                 _p(x), _p(y), _p(ws), ws.numel(), _stream())
            fn = lambda: call("vgposp_kernel_gemv_t", kid, _p(X), n, _p(X), n, d, _p(amp_t),
                              _p(ls_t), _p(None), _p(None), _p(x), _p(yf), _p(ws), ws.numel(),
                              _stream())
            res["full_square"] = _launches(timed, fn, a.reps)
            res["full_square"]["entries_per_s"] = float(n) * n / (res["full_square"]["ms_median"]
                                                                  * 1e-3)
            full = yf + (NOISE + JITTER) * x      # its diagonal is amp^2 = 1
            res["max_diff_to_full_square"] = float((y - full).abs().max() / full.abs().max())
            new, old = res["kernel_symv"], res["full_square"]
            res["ratio"] = new["ms_median"] / old["ms_median"]
            if ENTRY_NEW[kind] is not None:
                res["predicted_ratio"] = ENTRY_NEW[kind] / (2 * E_FULL[kind])
            res["faster_than_full_square"] = bool(new["ms_max"] < old["ms_min"])
            size["kinds"][kind] = res
        if label == "65536":    # the stored pass over the same triangle
            wsu = linalg.workspace(query("vgposp_symv_upper_workspace_bytes", n))
            for kind in KINDS:
                S = linalg.kernel_matrix(kind, X, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
                fn = lambda: call("vgposp_symv_upper", _p(S), n, S.stride(0), _p(None), _p(x),
                                  _p(yf), _p(wsu), wsu.numel(), _stream())
                r = _launches(timed, fn, a.reps)
                r["sigma_bytes"] = 8.0 * n * n
                res = size["kinds"][kind]
                call("vgposp_kernel_symv", KERNEL_KINDS[kind], _p(X), n, d, _p(amp_t), _p(ls_t),
                     _p(None), _p(diag), _p(x), _p(y), _p(ws), ws.numel(), _stream())
                res["max_diff_to_stored"] = float((y - yf).abs().max() / yf.abs().max())
                res["symv_upper_stored"] = r
                res["over_stored"] = res["kernel_symv"]["ms_median"] / r["ms_median"]
                del S
                torch.cuda.empty_cache()
            del wsu
        out["sizes"][label] = size
        del ws
        torch.cuda.empty_cache()
    return out


def _place(a, shape, criterion, labels, repeats):
    import torch
    from vgposp_amd import linalg
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_criteria import CriterionPlacement, SiteKernel
    torch.cuda.set_device(0)
    timed = _timing(torch)
    Xh = grid_points(shape, jitter=0.05, seed=0)
    ls = 2.0 * grid_spacing(shape)
    n, k = len(Xh), a.k
    runs = {"n": n, "k": k, "criterion": criterion}
    for label in labels:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        if label == "dense":
            S = linalg.kernel_matrix("eq", Xh, None, 1.0, ls, diag_shift=NOISE + JITTER)[0]
        else:
            S = SiteKernel("eq", Xh, 1.0, ls, noise=NOISE + JITTER)
        g = CriterionPlacement(S, k, criterion)
        g.run(k)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        ms = [timed(lambda: g.run(k)) for _ in range(repeats)]
        picks, deltas = g.result()
        runs[label] = {"first_run_seconds_with_setup": first, "ms": ms,
                       "ms_median": statistics.median(ms) if ms else None,
                       "picks": [int(p) for p in picks],
                       "distinct_picks": len(set(int(p) for p in picks)),
                       "sum_of_deltas": float(deltas.sum()),
                       "held_bytes": torch.cuda.memory_allocated() - base,
                       "peak_bytes": torch.cuda.max_memory_allocated() - base,
                       "workspace_bytes": g.ws.numel()}
        del g, S
    if "dense" in runs and "matrix_free" in runs:
        runs["same_picks"] = runs["dense"]["picks"] == runs["matrix_free"]["picks"]
    return runs


def stage_pass2m(a):
    import torch
    from vgposp_amd import linalg
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    torch.cuda.set_device(0)
    timed = _timing(torch)
    shape = (128, 128, 128)
    X = torch.as_tensor(grid_points(shape, jitter=0.05, seed=0), device="cuda")
    n, d = X.shape
    amp_t, ls_t = linalg._vec(1.0), linalg._vec(2.0 * grid_spacing(shape))
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = linalg.workspace(query("vgposp_kernel_symv_workspace_bytes", n))
    fn = lambda: call("vgposp_kernel_symv", KERNEL_KINDS["eq"], _p(X), n, d, _p(amp_t), _p(ls_t),
                      _p(None), _p(None), _p(x), _p(y), _p(ws), ws.numel(), _stream())
    ms = timed(fn)
    return {"n": n, "ms": ms, "triangle_entries": 0.5 * n * n, "workspace_bytes": ws.numel(),
            "triangle_entries_per_s": 0.5 * n * n / (ms * 1e-3),
            "finite": bool(torch.isfinite(y).all())}


def run_child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--k", str(a.k), "--reps",
           str(a.reps)]
    print(f"[site_kernel_criteria_bench] stage {stage}, limit {limit:.0f} s ...", flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_kernel_criteria.json"))
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed launches (at least 5)")
    ap.add_argument("--limit", type=int, default=300, help="seconds for the pass and place stages")
    ap.add_argument("--setup", type=float, default=90.0,
                    help="seconds allowed to a derived-limit stage besides its passes")
    ap.add_argument("--margin", type=float, default=4.0,
                    help="the passes of such a stage may take this many times their prediction")
    ap.add_argument("--pass2m-max", type=float, default=120.0,
                    help="run the 2^21 pass only if its predicted time is below this")
    ap.add_argument("--child", choices=("pass", "place", "large", "entropy", "pass2m"))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        if a.child == "pass":
            res = stage_pass(a)
        elif a.child == "place":
            res = _place(a, SIZES["65536"], "variance", ("matrix_free", "dense"), 3)
        elif a.child == "large":
            res = _place(a, SIZES["262144"], "variance", ("matrix_free",), 1)
        elif a.child == "entropy":
            res = _place(a, (128, 128, 128), "entropy", ("matrix_free",), 1)
        else:
            res = stage_pass2m(a)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    res = {"tool": "tools/site_kernel_criteria_bench.py", "stopped": None}
    # a stage that stops ends the run: nothing more is started on the device after it
    for stage in ("pass", "place", "large", "entropy", "pass2m"):
        limit = a.limit
        if stage in ("large", "pass2m"):
            rate = res["pass"]["sizes"]["262144"]["kinds"]["eq"]["kernel_symv"][
                "triangle_entries_per_s"]
            n = 262144 if stage == "large" else 1 << 21
            passes = 2 * (a.k + 1) if stage == "large" else 1     # (the run and its one repeat)
            predicted = passes * 0.5 * n * n / rate
            limit = a.setup + a.margin * predicted
            res[stage + "_limit"] = {"triangle_entries_per_s": rate, "passes": passes,
                                     "predicted_pass_seconds": predicted,
                                     "setup_seconds": a.setup, "margin": a.margin,
                                     "seconds": limit}
            if stage == "pass2m" and predicted > a.pass2m_max:
                res[stage] = None
                res["pass2m_not_run"] = f"predicted {predicted:.0f} s > {a.pass2m_max:.0f} s"
                continue
        res[stage], note = run_child(a, stage, limit)
        if res[stage] is None:
            res["stopped"] = f"{stage}: {note}"
            break
    if res["stopped"]:
        print(f"[site_kernel_criteria_bench] stopped: {res['stopped']}", flush=True)
    print(f"[site_kernel_criteria_bench] {json.dumps(res)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[site_kernel_criteria_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
