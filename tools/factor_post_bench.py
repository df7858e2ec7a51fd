#!/usr/bin/env python
"""Measure the field reconstruction on a factored Sigma = F F^T + D (csrc/criteria.hip, the
vgposp_fpost entries) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4m into profiles/factor_post.json.  The
driver never opens the GPU; the stage is one child process under its own time limit.  Nothing is
fixed in advance: the tool records what it measures.  Every time is from device events (torch
events around a whole call, the library's ProfScope pairs for a single kernel family), after two
warm-ups, as the median of ``--reps`` with min and max; the two sides alternate in one process.

  (n, S) = (65,536, 300), (262,144, 96), (262,144, 300), (2^21, 256), k = 50, B = 0, 1, 14, 78:
  64 variance columns and 0, 16, 16, 80 mean columns, i.e. one, two, two and three panels.
  "fused"      one vgposp_fpost_apply (variance, and the mean where B > 0): the small products
               behind alpha and Z, the stream launches and the sensor rows.
  "yardstick"  the same work out of launches the library had before: per chunk of 16,384 rows
               vgposp_gemm of F_c . P into a temporary [16,384][64 + pad16(B)], then
               vgposp_row_sumsq with alpha = -1, beta = 1 over its first 64 columns onto a copy of
               dg (the copy is made outside the timed region; the mean stays in the temporary).
  Also the stream's own scope (criteria_fpost_stream) as a rate over its byte model, 8 n S per
  panel + 8 n (1 + B), beside one vgposp_factor_symv pass (16 n S bytes) at the same shape.
  The fused stream ships if its whole range lies below the yardstick's at B = 0 and 14 on
  (262,144, 300) and (2^21, 256).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = 1e-2
SHAPES = ((65536, 300), (262144, 96), (262144, 300), (1 << 21, 256))
READINGS = (0, 1, 14, 78)
CHUNK = 16384
DECIDING = ((262144, 300), (1 << 21, 256))


def _stats(ms):
    return {"ms": ms, "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def _pad(c):
    return (c + 15) // 16 * 16


def _factor(torch, n, S):
    """A random factor with rows of unit expected norm, filled in row chunks."""
    F = torch.empty((n, S), dtype=torch.float64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(n + S)
    for r0 in range(0, n, 1 << 18):
        F[r0:r0 + (1 << 18)].normal_(0.0, S ** -0.5, generator=g)
    return F


def stage_stream(a):
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd import placement_criteria as PC
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
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

    out = {"reps": a.reps, "k": a.k, "chunk_rows": CHUNK,
           "source_hash": _lib.source_hash("criteria_fpost_stream"), "shapes": []}
    for n, S in SHAPES:
        F = _factor(torch, n, S)
        fac = PC.FactoredCovariance(F, noise=NOISE)
        sensors = torch.randperm(n, generator=torch.Generator().manual_seed(n))[:a.k].numpy()
        rec = PC.FieldReconstruction(fac, sensors, max_readings=max(READINGS))
        rec.check()
        x = torch.randn(n, dtype=torch.float64, device="cuda")
        y = torch.empty(n, dtype=torch.float64, device="cuda")
        sws = linalg.workspace(query("vgposp_factor_symv_workspace_bytes", n, S))
        symv = lambda: call("vgposp_factor_symv", *fac.args(), _p(x), _p(y), _p(sws), sws.numel(),
                            _stream())
        dg = (F * F).sum(1) + NOISE
        var = torch.empty(n, dtype=torch.float64, device="cuda")
        shape = {"n": n, "S": S, "factor_bytes": 8.0 * n * S, "readings": []}
        passes = []
        for B in READINGS:
            kp, bp = _pad(a.k), _pad(B)
            Y = torch.randn((a.k, B), dtype=torch.float64, device="cuda") if B else None
            res = torch.empty((n, max(B, 1)), dtype=torch.float64, device="cuda")
            P = torch.randn((S, kp + bp), dtype=torch.float64, device="cuda")
            tmp = torch.empty((CHUNK, kp + bp), dtype=torch.float64, device="cuda")
            yvar = torch.empty(n, dtype=torch.float64, device="cuda")

            def fused():
                rec._apply(var, Y, None, res if B else None)

            def yardstick():
                for c0 in range(0, n, CHUNK):
                    rows = min(CHUNK, n - c0)
                    call("vgposp_gemm", 0, 0, rows, kp + bp, S, 1.0, F[c0].data_ptr(), S, _p(P),
                         kp + bp, 0.0, _p(tmp), kp + bp, 0, 0, 0, _stream())
                    call("vgposp_row_sumsq", _p(tmp), rows, kp, kp + bp, -1.0, 1.0,
                         yvar[c0].data_ptr(), _stream())

            tf, ty, ts, tp = [], [], [], []
            for i in range(2 + a.reps):          # the sides alternate in one process
                yvar.copy_(dg)
                t0 = timed(fused)
                t1 = timed(yardstick)
                _lib.prof_enable(True)
                try:
                    fused()
                    torch.cuda.synchronize()
                    sc = _lib.prof_query("criteria_fpost_stream")
                finally:
                    _lib.prof_enable(False)
                t2 = timed(symv)
                if i >= 2:
                    tf.append(t0)
                    ty.append(t1)
                    ts.append(sc[0])
                    tp.append(t2)
            panels = -(-(kp + bp) // 64)
            model = 8.0 * n * S * panels + 8.0 * n * (1 + B)
            r = {"B": B, "columns": kp + bp, "panels": panels, "stream_launches": sc[1],
                 "fused": _stats(tf), "yardstick": _stats(ty), "stream_scope": _stats(ts),
                 "stream_bytes": model}
            r["stream_scope"]["bytes_per_s"] = model / (r["stream_scope"]["ms_median"] * 1e-3)
            r["stream_scope"]["flops_per_s"] = (2.0 * n * S * (kp + bp)
                                                / (r["stream_scope"]["ms_median"] * 1e-3))
            r["fused_over_yardstick"] = r["fused"]["ms_median"] / r["yardstick"]["ms_median"]
            r["fused_range_below_yardstick_range"] = r["fused"]["ms_max"] < r["yardstick"]["ms_min"]
            shape["readings"].append(r)
            passes += tp
            del P, tmp, res, yvar
        shape["factor_symv"] = _stats(passes)
        shape["factor_symv"]["bytes_per_s"] = 16.0 * n * S / (shape["factor_symv"]["ms_median"]
                                                              * 1e-3)
        shape["workspace_bytes"] = rec.ws.numel()
        out["shapes"].append(shape)
        del rec, fac, F, sws, dg, var
        torch.cuda.empty_cache()
    out["fused_ships"] = all(r["fused_range_below_yardstick_range"] for s in out["shapes"]
                             if (s["n"], s["S"]) in DECIDING for r in s["readings"]
                             if r["B"] in (0, 14))
    return out


STAGES = {"stream": stage_stream}


def run_child(a, stage, limit):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", stage, "--k", str(a.k), "--reps",
           str(a.reps)]
    print(f"[factor_post_bench] stage {stage}, limit {limit:.0f} s ...", flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "factor_post.json"))
    ap.add_argument("--k", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7, help="timed repetitions (at least 5)")
    ap.add_argument("--limit", type=int, default=300, help="seconds per stage")
    ap.add_argument("--child", choices=tuple(STAGES))
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(STAGES[a.child](a)), flush=True)
        return 0
    res = {"tool": "tools/factor_post_bench.py", "stopped": None}
    for stage in STAGES:
        res[stage], note = run_child(a, stage, a.limit)
        if res[stage] is None:
            res["stopped"] = f"{stage}: {note}"
            break
    if res["stopped"]:
        print(f"[factor_post_bench] stopped: {res['stopped']}", flush=True)
    print(f"[factor_post_bench] {json.dumps(res)}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[factor_post_bench] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
