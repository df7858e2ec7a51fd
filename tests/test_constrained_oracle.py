"""CPU: the constrained-greedy oracle (tests/numpy_constrained_greedy.py) against itself, against
the goldens produced with the reference's own functions, and against the unconstrained oracle; and
the validation of the ``candidates`` / ``placed`` arguments."""
import json
import os

import numpy as np
import pytest

from oracle import placement as op
from tests import numpy_constrained_greedy as ncg
from tests.golden_io import GOLDEN, placement_cases, placement_cov
from vgposp_amd.constraints import normalize_constraints, reject_constraints

with open(os.path.join(GOLDEN, "constrained_golden.json")) as f:
    CON = json.load(f)
FREE = placement_cases()
SMALL = [n for n in CON if CON[n]["N"] <= 64]   # one pinv per evaluation: small orders only


def _cand(N):
    return [i for i in range(N) if i % 3 != 1]


def test_golden_holds_the_cases_and_the_gap_rule():
    assert sorted(CON) == sorted(["randcov11", "spd11", "spd40", "grid4", "grid5", "grid654",
                                  "grid5m12", "grid5m52", "grid8"])
    for name, e in CON.items():
        assert min(e["alg2_gap"] + e["alg1_gap"]) >= 1e-6, name
        assert e["alg2"] != FREE[name]["alg2"][: e["k"]], name  # the constraints change the picks
        assert not set(e["alg2"]) & set(e["placed"])
        assert all(a % 3 != 1 for a in e["alg2"] + e["alg1"])
    assert CON["grid8"]["placed"] == [1, 256]


@pytest.mark.parametrize("name", SMALL)
def test_restatements_agree(name):
    e = CON[name]
    cov = placement_cov(name, FREE[name])
    N = e["N"]
    for lazy, slow in ((True, ncg.constrained_lazy), (False, ncg.constrained_full)):
        p, d, ev, gap = slow(cov, e["k"], _cand(N), e["placed"])
        fp, fd, fev, fgap = ncg.constrained_fast(cov, e["k"], _cand(N), e["placed"], lazy=lazy)
        assert p == fp and ev == fev
        np.testing.assert_allclose(d, fd, rtol=1e-9)
        np.testing.assert_allclose(gap, fgap, rtol=1e-6, atol=1e-12)


@pytest.mark.parametrize("name", list(CON))
def test_fast_form_matches_golden(name):
    e = CON[name]
    cov = placement_cov(name, FREE[name])
    for alg, lazy in (("alg2", True), ("alg1", False)):
        p, d, ev, gap = ncg.constrained_fast(cov, e["k"], _cand(e["N"]), e["placed"], lazy=lazy)
        assert p == e[alg] and ev == e[alg + "_evals"]
        np.testing.assert_allclose(d, e[alg + "_deltas"], rtol=1e-9)
        np.testing.assert_allclose(gap, e[alg + "_gap"], rtol=1e-6)


@pytest.mark.parametrize("name", SMALL)
def test_pinv_form_matches_golden(name):
    e = CON[name]
    cov = placement_cov(name, FREE[name])
    p, d, ev, _ = ncg.constrained_lazy(cov, e["k"], _cand(e["N"]), e["placed"], gaps=False)
    assert p == e["alg2"] and ev == e["alg2_evals"]
    np.testing.assert_allclose(d, e["alg2_deltas"], rtol=1e-12)
    p, d, ev, _ = ncg.constrained_full(cov, e["k"], _cand(e["N"]), e["placed"])
    assert p == e["alg1"] and ev == e["alg1_evals"]
    np.testing.assert_allclose(d, e["alg1_deltas"], rtol=1e-12)


@pytest.mark.parametrize("name", ["randcov11", "spd11", "grid4"])
def test_no_constraints_is_the_unconstrained_oracle(name):
    cov = placement_cov(name, FREE[name])
    k = FREE[name]["k"]
    want2 = [int(a) for a in op.placement_algorithm_2(cov, k)]
    want1 = [int(a) for a in op.placement_algorithm_1(cov, k)]
    assert ncg.constrained_lazy(cov, k, gaps=False)[0] == want2 == FREE[name]["alg2"]
    assert ncg.constrained_full(cov, k)[0] == want1 == FREE[name]["alg1"]
    assert ncg.constrained_fast(cov, k, lazy=True)[0] == want2
    assert ncg.constrained_fast(cov, k, lazy=False)[0] == want1


def test_masked_locations_stay_in_a_bar():
    """Deleting the non-candidate rows and columns is a different problem: other deltas."""
    cov = placement_cov("grid5", FREE["grid5"])
    _, d, _, _ = ncg.constrained_fast(cov, 3, _cand(125), lazy=False)
    _, dd = ncg.deleted_rows_picks(cov, 3, _cand(125))
    assert not np.allclose(d, dd, rtol=1e-3)


# ---- normalize_constraints ----
def test_validation_accepts_lists_masks_and_placed_outside_candidates():
    allowed, placed = normalize_constraints(10, 3, [5, 2, 7, 8], [1, 2])
    assert allowed.tolist() == [i in (2, 5, 7, 8) for i in range(10)]
    assert placed.tolist() == [1, 2] and placed.dtype == np.int64
    mask = np.arange(10) % 3 != 1
    allowed, placed = normalize_constraints(10, 6, mask, (4,))      # 4 is not a candidate
    assert allowed.tolist() == mask.tolist() and placed.tolist() == [4]
    assert normalize_constraints(10, 10)[0] is None and len(normalize_constraints(10, 10)[1]) == 0
    assert normalize_constraints(10, 2, None, np.array([9, 0]))[1].tolist() == [9, 0]


def test_validation_rejects_duplicates():
    with pytest.raises(ValueError, match="more than once"):
        normalize_constraints(10, 1, None, [3, 4, 3])
    with pytest.raises(ValueError, match="more than once"):
        normalize_constraints(10, 1, [1, 1, 2], None)


def test_validation_rejects_out_of_range():
    with pytest.raises(ValueError, match="outside"):
        normalize_constraints(10, 1, None, [10])
    with pytest.raises(ValueError, match="outside"):
        normalize_constraints(10, 1, [0, -1], None)
    with pytest.raises(ValueError, match="integer"):
        normalize_constraints(10, 1, None, [0.5])


def test_validation_rejects_k_above_free_candidates():
    normalize_constraints(10, 3, [0, 1, 2, 3], [3, 9])
    with pytest.raises(ValueError, match="exceeds the 3 candidates"):
        normalize_constraints(10, 4, [0, 1, 2, 3], [3, 9])
    with pytest.raises(ValueError, match="exceeds"):
        normalize_constraints(10, 9, None, [0, 1])


def test_validation_rejects_wrong_mask_length():
    with pytest.raises(ValueError, match="length 10"):
        normalize_constraints(10, 1, np.ones(9, dtype=bool))
    with pytest.raises(ValueError, match="length 10"):
        normalize_constraints(10, 1, np.ones((10, 1), dtype=bool))


def test_reject_constraints():
    reject_constraints("x")
    with pytest.raises(ValueError, match="does not support"):
        reject_constraints("x", candidates=[1])
    with pytest.raises(ValueError, match="does not support"):
        reject_constraints("x", placed=[])
