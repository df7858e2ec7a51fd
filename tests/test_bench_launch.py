"""CPU: ``python bench.py --gpus N`` starts its own N ranks (torch.distributed.run as a child
process, 127.0.0.1 rendezvous) and every rank sees WORLD_SIZE = N; inside a launcher a world size
that differs from --gpus is a hard error.  ``--rank-check`` makes each rank report and exit before
any GPU call.  GPU: a plain run's result line and its --dump-outputs files on a small grid."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e,
                          capture_output=True, text=True, timeout=120)


def test_bench_starts_its_own_ranks():
    r = _run(["--gpus", "2", "--rank-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert sorted(x["rank"] for x in lines) == [0, 1]
    assert all(x["n_gpus"] == 2 for x in lines)


def test_single_gpu_default_runs_one_rank_in_process():
    r = _run(["--rank-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip()) == {"rank": 0, "local_rank": 0, "n_gpus": 1}


def test_steps_must_be_positive():
    r = _run(["--steps", "0", "--rank-check"])
    assert r.returncode != 0
    assert "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    """A plain run (8^3 grid, k = 5) prints the headline line alone, times exactly --steps steps,
    and --dump-outputs writes what the step computed: the same arrays as GreedyPlacement.result()
    of the same workload run here."""
    import numpy as np
    import torch

    from vgposp_amd import linalg
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    from vgposp_amd.workloads import placement_split
    shape, k = (8, 8, 8), 5
    d = tmp_path / "dump"
    r = _run(["--shape", *map(str, shape), "--k", str(k), "--steps", "2", "--warmup", "1",
              "--dump-outputs", str(d)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "placements/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: k placements per timed step
    assert np.isclose(line["value"], k / (line["ms_per_step"] * 1e-3), rtol=1e-9)
    # nothing that takes a run of its own in a plain line
    for key in ("roofline", "breakdown", "cholesky_gflops", "c4", "grid_sweep", "vgp_c3", "c2",
                "cpu_baseline"):
        assert key not in line
    got = {p.stem: np.load(p) for p in d.iterdir()}
    assert sorted(got) == ["covariance_factored_sample", "evaluations", "selected", "selected_delta"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["selected"].tolist() == line["selected"]
    # the same workload through the library here
    X, ls = placement_split(shape, 0)
    n = len(X)
    Sigma = torch.empty((n, n), dtype=torch.float64, device="cuda")
    linalg.kernel_matrix("eq", linalg.as_device(X), None, 1.0, ls, diag_shift=1e-2 + 1e-6,
                         out=Sigma[None])
    sel, delta, evals = GreedyPlacement(Sigma, k).run(k).result()
    assert got["selected"].tolist() == [int(s) for s in sel]
    assert got["evaluations"].tolist() == evals.tolist()
    # same kernels on the same inputs; 1e-12 leaves room only for the order of a reduction
    np.testing.assert_allclose(got["selected_delta"], delta, rtol=1e-12)
    assert got["covariance_factored_sample"].shape == (65536,)
    assert np.isfinite(got["covariance_factored_sample"]).all()


def test_world_size_mismatch_is_an_error():
    r = _run(["--gpus", "2", "--rank-check"], env={"WORLD_SIZE": "3", "RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=3" in r.stderr
