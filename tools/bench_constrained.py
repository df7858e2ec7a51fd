#!/usr/bin/env python
"""Measure the constrained greedy placement (candidate set + pre-installed sensors) on one MI355X.

Not bench.py: this records the figures behind DESIGN's subsection on constrained placement and the
choice of ``placement_algorithm2.CONDITION_BATCH`` into profiles/constrained_placement.json.

Per order N (default 16,384 and 65,536), in a fresh child process under its own time limit (the
driver never opens the GPU and stops at the first step that fails or runs out of time):

  conditioning  the forced rounds on m = 256 placed sensors (vgposp_greedy_condition) with batch 1
                (one vgposp_greedy_update, i.e. today's mat-vec kernel, per sensor) and with every
                batched width that is built (4 and 8 sensors per pass over L^-1).  Device events,
                one warm-up and ``--reps`` repetitions each, alternating the widths; the median,
                and the achieved HBM rate as the algorithmic bytes of the L^-1 lower triangle per
                pass (8 n (n + 1) / 2) times the passes, over the time.  One further run of each
                width under the library's per-launch timing gives the mat-vec's and the updates'
                shares.
  rounds        k = 50 lazy rounds: the unconstrained problem (the parent's code path, repeated to
                give its run-to-run spread), the same rounds with only the candidate mask, and the
                rounds that follow the conditioning (rounds m .. m + k - 1, whose O(n t) updates
                are longer by construction).

One factorization per N serves every measurement: the workspace right after it is saved and copied
back before each repetition, and the problems share that one workspace buffer.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {1024: (16, 8, 8), 4096: (16, 16, 16), 16384: (32, 32, 16), 65536: (64, 32, 32)}
BATCHES = (1, 4, 8)


def child(a):
    import numpy as np
    import torch
    from vgposp_amd import _lib, linalg
    from vgposp_amd._lib import call
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.linalg import _p, _stream
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    torch.cuda.set_device(0)
    N, m, k = a.n, a.m, a.k
    shape = SHAPES[N]
    X = torch.as_tensor(grid_points(shape, jitter=0.05, seed=3), device="cuda")
    S = linalg.kernel_matrix("eq", X, None, 1.0, 2 * grid_spacing(shape),
                             diag_shift=1e-2 + 1e-6)[0]
    mask = np.arange(N) % 3 != 1
    placed = ((np.arange(m, dtype=np.int64) * (N // m) + 7) % N)
    # one factorization; the three problems share the factored S and the workspace layout
    gU = GreedyPlacement(S, m + k)                                  # unconstrained
    gC = GreedyPlacement(S, k, candidates=mask, placed=placed, condition_batch=max(BATCHES))
    assert gU.ws.numel() == gC.ws.numel() and gC.kmax == m + k
    gC.ws = gU.ws   # one workspace buffer for every problem: where a buffer lies is not under test
    ev = lambda: torch.cuda.Event(enable_timing=True)
    t0, t1 = ev(), ev()
    t0.record()
    call("vgposp_greedy_init_ex", _p(S), gU.n, S.stride(0), gU.kmax, *gU.params, _p(gU.info),
         _p(gU.ws), gU.ws.numel(), _stream())
    t1.record()
    t1.synchronize()
    gU.check()
    factor_ms = t0.elapsed_time(t1)
    ws0 = gU.ws.clone()

    def reset(g):
        g.ws.copy_(ws0)
        g.rounds = 0

    def timed(fn):
        torch.cuda.synchronize()
        s, e = ev(), ev()
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    def condition(batch):
        reset(gC)
        gC.condition_batch = batch
        return timed(gC.constrain)

    def rounds(g, after=None):
        reset(g)
        if after:
            after()
        ms = timed(lambda: [g.step(True) for _ in range(k)])
        return ms

    tri_bytes = 8.0 * N * (N + 1) / 2

    def rows_read_bytes(a0):
        """L^-1 entries in rows >= a0 of the lower triangle: what a pass starting there reads."""
        a0 = float(a0)
        return 8.0 * (a0 * (N - a0) + (N - a0) * (N - a0 + 1) / 2)
    cond = {b: [] for b in BATCHES}
    for b in BATCHES:
        condition(b)                                                # warm-up
    for _ in range(a.reps):                                         # alternate the widths
        for b in BATCHES:
            cond[b].append(condition(b))
    # where the time goes: one more run of each width under the library's per-launch timing
    kernels = {}
    for b in BATCHES:
        _lib.prof_enable(True)
        condition(b)
        kernels[b] = {name: {"ms": ms, "launches": cnt}
                      for name, (ms, cnt, _, _) in sorted(_lib.prof_dump().items())}
        _lib.prof_enable(False)
    # results must not change: the rounds after each width give the same picks
    after = {}
    for b in BATCHES:
        gC.condition_batch = b
        rounds(gC, gC.constrain)
        A, d, _ = gC.result()
        after[b] = ([int(x) for x in A], d)
    same_picks = all(after[b][0] == after[1][0] for b in BATCHES)
    max_rel = max(float(np.max(np.abs(after[b][1] - after[1][1]) / np.abs(after[1][1])))
                  for b in BATCHES)
    conditioning = {}
    for b in BATCHES:
        med = statistics.median(cond[b])
        passes = (m - 1) if b == 1 else -(-(m - 1) // b)
        read = sum(rows_read_bytes(placed[j0:min(j0 + b, m - 1)].min())
                   for j0 in range(0, m - 1, b))
        conditioning[f"batch_{b}"] = {
            "ms": cond[b], "ms_median": med, "spread": (max(cond[b]) - min(cond[b])) / med,
            "passes_over_Linv": passes, "ms_per_sensor": med / m,
            # the whole lower triangle per pass (the algorithmic figure), and only the rows a
            # pass reads: those from its smallest sensor index down
            "hbm_gbps_algorithmic": passes * tri_bytes / med / 1e6,
            "hbm_gbps_rows_read": read / med / 1e6,
            "speedup_over_batch_1": statistics.median(cond[1]) / med,
            "kernels_profiled_run": kernels[b]}
    # rounds: unconstrained (the parent's path) x reps, mask only, after conditioning
    # mask only: a third of the locations blocked, none of them an unconstrained pick, so the
    # rounds make the same picks and stream the same rows; what differs is the mask itself
    rounds(gU)
    picks = [int(x) for x in gU.result()[0]]
    keep = np.ones(N, dtype=bool)
    keep[np.arange(N) % 3 == 1] = False
    keep[picks] = True
    gM = GreedyPlacement(S, m + k, candidates=keep)
    assert gM.ws.numel() == gU.ws.numel()
    gM.ws = gU.ws
    rounds(gM, gM.constrain)                                        # warm-ups
    mask_picks_equal = [int(x) for x in gM.result()[0]] == picks
    free, masked = [], []
    for _ in range(a.reps):
        free.append(rounds(gU))
        masked.append(rounds(gM, gM.constrain))
    gC.condition_batch = max(BATCHES)
    cond_rounds = [rounds(gC, gC.constrain) for _ in range(a.reps)]
    fm, mm = statistics.median(free), statistics.median(masked)
    return {"N": N, "m": m, "k": k, "reps": a.reps, "factor_inverse_ms": factor_ms,
            "tri_bytes_per_pass": tri_bytes, "conditioning": conditioning,
            "picks_equal_across_batches": same_picks, "max_rel_delta_diff_across_batches": max_rel,
            "rounds": {"unconstrained_ms": free, "unconstrained_ms_median": fm,
                       "unconstrained_spread": (max(free) - min(free)) / fm,
                       "mask_only_ms": masked, "mask_only_ms_median": mm,
                       "mask_only_over_unconstrained": mm / fm,
                       "mask_only_picks_equal_unconstrained": mask_picks_equal,
                       "after_conditioning_ms": cond_rounds,
                       "after_conditioning_ms_median": statistics.median(cond_rounds),
                       "note": "after conditioning the rounds are m .. m + k - 1: their O(n t) "
                               "updates run over m more rows than rounds 0 .. k - 1"}}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "constrained_placement.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 65536], choices=sorted(SHAPES))
    ap.add_argument("--m", type=int, default=256, help="placed sensors")
    ap.add_argument("--k", type=int, default=50, help="rounds after conditioning")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=360, help="seconds per GPU step")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int, default=None)
    a = ap.parse_args()
    if a.child:
        sys.path.insert(0, ROOT)
        print("RESULT " + json.dumps(child(a)), flush=True)
        return 0
    res = {"tool": "tools/bench_constrained.py", "sizes": [], "stopped": None}
    for n in a.sizes:
        print(f"[bench_constrained] N = {n} ...", flush=True)
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--m", str(a.m),
               "--k", str(a.k), "--reps", str(a.reps)]
        r = None
        try:
            p = subprocess.run(cmd, cwd=ROOT, timeout=a.limit, capture_output=True, text=True)
            for line in p.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
            note = f"N = {n}: exit status {p.returncode}: {p.stderr.strip()[-800:]}"
        except subprocess.TimeoutExpired:
            note = f"N = {n}: no result within {a.limit} s"
        if r is None:  # nothing more is started on the GPU after a failed step
            res["stopped"] = note
            print(f"[bench_constrained] stopped: {note}", flush=True)
            break
        print(f"[bench_constrained] {json.dumps(r)[:900]}", flush=True)
        res["sizes"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[bench_constrained] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
