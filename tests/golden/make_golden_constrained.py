"""Generate golden vectors of the CONSTRAINED greedy placement (a candidate set and pre-installed
sensors) by driving the REFERENCE's own ``nominator``, ``denominator`` and ``argmax_cache_linear``
through the constrained loop.

Run where a checkout of the reference is at hand (it is absent on the GPU box, so this is never
run there):

    python tests/golden/make_golden_constrained.py /path/to/reference

It imports the reference's ``placement_algorithm2`` module behind the same inert stubs as
``make_golden.py`` and writes ``tests/golden/constrained_golden.json``: picks, selected deltas,
lazy evaluation counts and the per-round relative gap between the best and the second-best delta
among the allowed candidates.  The inputs are the covariances of the committed
``placement_*.npz`` cases; only data is written, no reference source is copied.

Cases: ``candidates = {i : i % 3 != 1}``; ``placed`` = the first two unconstrained algorithm-1
picks (``[1, N // 2]`` for grid8).  Every recorded round must have a relative gap of at least
1e-6, or nothing is written: a pick decided by rounding is not a golden.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import placement as op  # noqa: E402
from tests import numpy_constrained_greedy as ncg  # noqa: E402
from tests.golden_io import placement_cases, placement_cov  # noqa: E402

CASES = ["randcov11", "spd11", "spd40", "grid4", "grid5", "grid654", "grid5m12", "grid5m52",
         "grid8"]
MIN_GAP = 1e-6


def _import_reference(path):
    import make_golden  # the stubs of the unconstrained generator (same directory)
    for name in ["tensorflow", "tensorflow.compat", "tensorflow.compat.v1",
                 "tensorflow_probability", "tensorboard", "tensorboard.plugins",
                 "tensorboard.plugins.projector", "seaborn"]:
        sys.modules[name] = make_golden._Stub(name)
    sys.modules["tensorflow"].__version__ = "1.15.0"
    import matplotlib
    matplotlib.use("Agg")
    sys.path.insert(0, path)
    import placement_algorithm2 as alg2  # the reference module
    return alg2


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    alg2 = _import_reference(sys.argv[1])
    alg2.print = lambda *a, **k: None
    unconstrained = placement_cases()
    golden = {}
    for name in CASES:
        e = unconstrained[name]
        cov = np.asarray(placement_cov(name, e), dtype=np.float64)
        N, k = cov.shape[0], int(e["k"])
        cand = [i for i in range(N) if i % 3 != 1]
        free1 = [int(a) for a in e.get("alg1") or op.placement_lazy_precision(cov, k, lazy=False)]
        placed = [1, N // 2] if name == "grid8" else free1[:2]
        # the reference's functions through the constrained lazy and full loops
        p2, d2, ev2, _ = ncg.constrained_lazy(cov, k, cand, placed, alg2.nominator,
                                              alg2.denominator, alg2.argmax_cache_linear,
                                              gaps=False)
        p1, d1, ev1, _ = ncg.constrained_full(cov, k, cand, placed, alg2.nominator,
                                              alg2.denominator)
        # the gap of every recorded round, along each recorded sequence
        gap2 = [ncg._gap(op.all_deltas(cov, placed + p2[:r])[0][
            [c for c in cand if c not in placed + p2[:r]]]) for r in range(k)]
        gap1 = [ncg._gap(op.all_deltas(cov, placed + p1[:r])[0][
            [c for c in cand if c not in placed + p1[:r]]]) for r in range(k)]
        assert min(gap2 + gap1) >= MIN_GAP, (name, gap2, gap1)
        free2 = [int(a) for a in e["alg2"]]
        assert p2 != free2[:k] and p1 != free1[:k], (name, "the constraints change no pick")
        golden[name] = dict(N=N, k=k, candidates="i % 3 != 1", placed=placed, alg2=p2,
                            alg2_deltas=d2, alg2_evals=ev2, alg2_gap=gap2, alg1=p1,
                            alg1_deltas=d1, alg1_evals=ev1, alg1_gap=gap1)
        print(name, "placed", placed, "alg2", p2, "alg1", p1, "evals", ev2,
              "min gap %.2e" % min(gap2 + gap1), flush=True)
    with open(os.path.join(HERE, "constrained_golden.json"), "w") as f:
        json.dump(golden, f, indent=1)


if __name__ == "__main__":
    main()
