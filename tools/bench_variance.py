#!/usr/bin/env python
"""Measure the chunked marginal predictive variance (distributions.variance) on one MI355X.

Not bench.py: this records the figures behind DESIGN §4's ``row_sumsq`` row and the choice of
``distributions.PREDICT_CHUNK_BYTES`` into one JSON file (default profiles/variance_map.json).

Every GPU step is a fresh child process under its own time limit; the driver itself never opens
the GPU, and it stops at the first step that fails or runs out of time.

  rate      vgposp_row_sumsq on [2^20 x 512] and [2^21 x 64] against a device-to-device copy of
            the same matrix timed in the same process (a read-only pass should not be slower than
            a copy, which also writes).
  map       a full-size uncertainty map at P = 128^3: the GPRM on n = 4,096 observations, and the
            VGP at config C3's M = 512; total time, and from the library's per-launch timing the
            share of GEMM, kernel assembly and row_sumsq, and the GEMM's TF/s.  Swept over chunk
            budgets of 32, 64, 128 and 256 MiB.
  parent    GPRM n = 4,096, P = 16,384 (the largest P at which the P x P path is cheap to run):
            ``variance()`` of another source tree (``--parent-tree``, a checkout of the parent
            commit with its library built) against this tree's, results compared.

``--alt-lib NAME=PATH`` repeats ``rate`` and the 256 MiB maps with another build of the library
(e.g. one whose gp.hip was compiled with -DVG_ROWSUMSQ_NT=0, plain instead of non-temporal loads).
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20
RATE_SHAPES = [(1 << 20, 512), (1 << 21, 64)]
BUDGETS_MIB = [32, 64, 128, 256]


# ---- children (each runs in its own process, on the GPU) ------------------------------------------

def _event_ms(torch, fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / reps


def child_rate(a):
    import torch
    from vgposp_amd import linalg
    torch.cuda.set_device(0)
    out = []
    for rows, cols in RATE_SHAPES:
        V = torch.randn((rows, cols), dtype=torch.float64, device="cuda")
        D = torch.empty_like(V)
        o = torch.empty(rows, dtype=torch.float64, device="cuda")
        for _ in range(2):  # warm both
            D.copy_(V)
            linalg.row_sumsq(V, out=o)
        torch.cuda.synchronize()
        # alternate the two, keep the best of three windows of each
        t_copy = min(_event_ms(torch, lambda: D.copy_(V), a.reps) for _ in range(3))
        t_rss = min(_event_ms(torch, lambda: linalg.row_sumsq(V, out=o), a.reps) for _ in range(3))
        ref = (V[:4096] * V[:4096]).sum(1)
        err = float(((o[:4096] - ref).abs() / ref).max())
        nbytes = 8.0 * rows * cols
        out.append({"rows": rows, "cols": cols, "matrix_gib": nbytes / 2 ** 30,
                    "row_sumsq_ms": t_rss, "row_sumsq_gbps": (nbytes + 8.0 * rows) / t_rss / 1e6,
                    "copy_ms": t_copy, "copy_read_plus_write_gbps": 2 * nbytes / t_copy / 1e6,
                    "row_sumsq_over_copy_time": t_rss / t_copy, "max_rel_err_vs_torch": err})
        del V, D, o
    return {"shapes": out, "reps": a.reps}


def _gprm(n_side, Xs):
    import numpy as np
    from vgposp_amd import distributions as tfd, psd_kernels as tfk
    from vgposp_amd.data_generation import grid_points, grid_spacing
    shp = (n_side,) * 3
    X = grid_points(shp, jitter=0.05, seed=1)
    y = np.sin(2 * np.pi * X).sum(1)
    k = tfk.ExponentiatedQuadratic(1.0, 2.0 * grid_spacing(shp))
    return tfd.GaussianProcessRegressionModel(k, index_points=Xs, observation_index_points=X,
                                              observations=y, observation_noise_variance=1e-2,
                                              predictive_noise_variance=0.0)


def _vgp(Xs):
    from vgposp_amd import distributions as tfd, psd_kernels as tfk
    from vgposp_amd.workloads import vgp_c3_data
    X, y, Z = vgp_c3_data(n=32)   # C3's 8^3 inducing grid; a 32^3 sample of its observations
    k = tfk.ExponentiatedQuadratic(1.0, 1.0)
    loc, scale = tfd.VariationalGaussianProcess.optimal_variational_posterior(k, Z, X, y, 0.1)
    # plain copies: the posterior is fixed here, not re-derived on every call
    return tfd.VariationalGaussianProcess(k, Xs, Z, loc.clone(), scale.clone(),
                                          observation_noise_variance=0.1)


def child_map(a):
    import torch
    from vgposp_amd import _lib, distributions as tfd
    from vgposp_amd.data_generation import grid_points
    torch.cuda.set_device(0)
    tfd.PREDICT_CHUNK_BYTES = a.budget_mib * MIB
    side = a.grid
    extent = 4.0 if a.model == "gprm" else 14.0
    Xs = torch.as_tensor(grid_points((side,) * 3, extent=extent), device="cuda")
    P = Xs.shape[0]
    model = _gprm(16, Xs) if a.model == "gprm" else _vgp(Xs)
    n = 4096 if a.model == "gprm" else 512
    chunk = tfd._predict_chunk(P, n, 2 if a.model == "gprm" else 3)
    model.variance(index_points=Xs[:min(P, 2 * chunk + 1)])   # warm every shape but the last chunk
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        v = model.variance()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    _lib.prof_enable(True)
    t0 = time.perf_counter()
    model.variance()
    torch.cuda.synchronize()
    t_prof = time.perf_counter() - t0
    fam = _lib.prof_fold(_lib.prof_dump())
    _lib.prof_enable(False)
    kernels = {name: {"ms": ms, "launches": cnt, "share_of_profiled_run": ms / 1e3 / t_prof,
                      "tflops": fl / ms / 1e9 if ms > 0 and fl > 0 else None,
                      "gbps": by / ms / 1e6 if ms > 0 and by > 0 else None}
               for name, (ms, cnt, fl, by) in sorted(fam.items())}
    return {"model": a.model, "n": n, "P": P, "budget_mib": a.budget_mib, "chunk_rows": chunk,
            "seconds": times, "seconds_best": min(times), "profiled_run_seconds": t_prof,
            "kernels": kernels, "var_min": float(v.min()), "var_mean": float(v.mean()),
            "var_max": float(v.max())}


def child_parent(a):
    import numpy as np
    import torch
    import vgposp_amd
    from vgposp_amd.data_generation import grid_points
    torch.cuda.set_device(0)
    Xs = grid_points((32, 32, 16), jitter=0.05, seed=3)   # P = 16,384
    model = _gprm(16, Xs)
    model.variance()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        v = model.variance()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    np.save(a.save, v.cpu().numpy())
    here = os.path.dirname(os.path.dirname(os.path.abspath(vgposp_amd.__file__))) == ROOT
    return {"tree": "this tree" if here else "parent tree",
            "n": 4096, "P": int(v.shape[-1]), "seconds": times, "seconds_best": min(times),
            "has_row_sumsq": hasattr(vgposp_amd.linalg, "row_sumsq")}


CHILDREN = {"rate": child_rate, "map": child_map, "parent": child_parent}


# ---- driver ---------------------------------------------------------------------------------------

def run_child(step, limit, tree=ROOT, lib=None, **kw):
    """One GPU step in a fresh process under ``limit`` seconds -> (result dict or None, note)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", step, "--tree", tree]
    for k, v in kw.items():
        cmd += ["--" + k.replace("_", "-"), str(v)]
    env = dict(os.environ)
    if lib:
        env["VGPOSP_LIB"] = os.path.abspath(lib)
    try:
        p = subprocess.run(cmd, env=env, cwd=tree, timeout=limit, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        return None, f"{step}: no result within {limit} s"
    for line in p.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:]), None
    return None, f"{step}: exit status {p.returncode}: {p.stderr.strip()[-800:]}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance_map.json"))
    ap.add_argument("--steps", default="rate,map,parent")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--alt-lib", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--grid", type=int, default=128, help="prediction grid side (P = grid^3)")
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    # child-only
    ap.add_argument("--child", choices=sorted(CHILDREN))
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--model", choices=["gprm", "vgp"], default="gprm")
    ap.add_argument("--budget-mib", type=int, default=128)
    ap.add_argument("--save", default=None)
    a = ap.parse_args()

    if a.child:
        sys.path.insert(0, os.path.abspath(a.tree))
        a.reps = a.reps or (20 if a.child == "rate" else 2)
        print("RESULT " + json.dumps(CHILDREN[a.child](a)), flush=True)
        return 0

    import numpy as np
    libs = [("default", None)] + [tuple(s.split("=", 1)) for s in a.alt_lib]
    res = {"tool": "tools/bench_variance.py", "grid": a.grid, "stopped": None}
    steps = a.steps.split(",")
    extra = {"reps": a.reps} if a.reps else {}

    def step(key, *args, **kw):
        if res["stopped"]:
            return None
        print(f"[bench_variance] {key} ...", flush=True)
        r, note = run_child(*args, **kw)
        if r is None:
            res["stopped"] = note   # nothing more is started on the GPU after a failed step
            print(f"[bench_variance] stopped: {note}", flush=True)
        else:
            print(f"[bench_variance] {key}: {json.dumps(r)[:600]}", flush=True)
        return r

    if "rate" in steps:
        res["row_sumsq_rate"] = {name: step(f"rate[{name}]", "rate", a.limit, lib=lib, **extra)
                                 for name, lib in libs}
    if "map" in steps:
        res["maps"] = []
        for model in ("gprm", "vgp"):
            for mib in BUDGETS_MIB:
                for name, lib in (libs if mib == BUDGETS_MIB[-1] else libs[:1]):
                    r = step(f"map[{model},{mib} MiB,{name}]", "map", a.limit, lib=lib, model=model,
                             budget_mib=mib, grid=a.grid, **extra)
                    if r is not None:
                        r["lib"] = name
                        res["maps"].append(r)
    if "parent" in steps:
        if not a.parent_tree:
            res["against_parent"] = "not measured: no --parent-tree given"
        else:
            with tempfile.TemporaryDirectory() as tmp:
                pa = step("parent[parent tree]", "parent", a.limit, tree=os.path.abspath(a.parent_tree),
                          save=os.path.join(tmp, "parent.npy"), **extra)
                nw = step("parent[this tree]", "parent", a.limit, save=os.path.join(tmp, "new.npy"),
                          **extra)
                if pa is not None and nw is not None:
                    d = np.abs(np.load(os.path.join(tmp, "parent.npy"))
                               - np.load(os.path.join(tmp, "new.npy")))
                    res["against_parent"] = {
                        "parent": pa, "new": nw, "max_abs_diff": float(d.max()),
                        "parent_over_new_time": pa["seconds_best"] / nw["seconds_best"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"[bench_variance] wrote {a.out}", flush=True)
    return 1 if res["stopped"] else 0


if __name__ == "__main__":
    sys.exit(main())
