"""GPU: the whole state of the greedy placement kernels (csrc/greedy.hip) against a longdouble
reference, not only their picks.

Every round, for every candidate the kernels write: the fresh delta vector, the pivot buffer
(nom_y, P_yy and the rows W[0..r)[y], V[0..r)[y] of the pick), the extracted column of L^-1, the
lazy cache and the evaluation counts.  The reference state (tests/greedy_state_reference.py) is
taken for A = the device's own picks so far, so a near-tie cannot make the two runs drift apart.

Tolerance: not fixed in advance.  e_cpu is the largest relative error of the fp64 host
restatement (tests/numpy_greedy_backend.NumpyGreedyBackend, the same incremental algorithm on
LAPACK) against the longdouble reference on the same Sigma and the same picks, over all rounds;
the device gets 16 e_cpu (other associations of the same sums: four accumulators per column,
512-row partials, the MFMA-blocked recursive inverse with split-K), and 16 e_cpu <= 1e-11 is
asserted as a condition on the inputs.  The policy (picks, evaluation counts, the cache) and the
slab split are exact: bit for bit, no tolerance.

Inputs (tests/test_greedy_state_reference.py asserts their conditions on the CPU): F1 eq
(13, 10, 8), n = 1040 — two CH = 1024 candidate chunks, three RC = 512 row chunks, three
TRMV_COLS = 512 column tiles — and its leading blocks; F2 matern52 (9, 9, 8); F3 eq (9, 9, 8)
with the TF variant's constants (eps = 1e-6 in the factor).
"""
import numpy as np
import pytest

from tests import greedy_state_reference as R
from tests.greedy_driver import Greedy

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


STATE_KEYS = ("delta", "cache", "piv", "selected", "sel_delta", "evals")


# ---- runs shared by the arithmetic and the policy tests ----
_runs = {}


def _run(name, n=None, lazy=True, cache_init=None, masked=False, placed=(), batch=8, lda=None,
         shift=0, k=None):
    """init (+ mask, + conditioning on `placed`) and k rounds; per round a host copy of the state.
    Returns a dict: recs (one per free round), cond (after the conditioning, or None), cache0
    (the cache before the first round), blocked0, after_init / after_rounds (the Sigma buffer)."""
    key = (name, n, lazy, cache_init, masked, tuple(placed), batch, lda, shift, k)
    if key in _runs:
        return _runs[key]
    K, _, (eps, thr, cinit) = R.fixture(name)
    n = K.shape[0] if n is None else n
    k = R.rounds_at(n) if k is None else k
    m = len(placed)
    g = Greedy(K, n, m + k, (eps, thr, cinit if cache_init is None else cache_init), lda, shift)
    g.init()
    out = {"n": n, "m": m, "k": k, "host0": g.host0, "cond": None, "placed": list(placed)}
    if lda is not None:
        out["after_init"] = g.matrix()
    blocked = R.third_mask(n) if masked else np.zeros(n, dtype=bool)
    if masked:
        g.mask(blocked)
    out["blocked0"] = blocked
    out["cache0"] = g.cache.cpu().numpy().copy()
    if m:
        g.condition(placed, k, batch)
        out["cond"] = g.read()
    out["recs"] = []
    for r in range(m, m + k):
        g.step(r, lazy)
        out["recs"].append(g.read())
    if lda is not None:
        out["after_rounds"] = g.matrix()
    _runs[key] = out
    return out


_cpu = {}


def _e_cpu(name, n, picks, blocked, first):
    """The fp64 host restatement's error on the same Sigma and the same picks (shared by the runs
    that made the same picks)."""
    key = (name, n, tuple(picks), blocked is not None, first)
    if key not in _cpu:
        K, ref, (eps, _, _) = R.fixture(name)
        errs = R.backend_errors(ref, K, n, picks, eps, blocked=blocked, first=first)
        _cpu[key] = max(e["delta"] for e in errs)
    return _cpu[key]


def _check_arithmetic(label, name, run):
    K, ref, (eps, _, _) = R.fixture(name)
    n, m, k = run["n"], run["m"], run["k"]
    recs = run["recs"]
    picks = [int(a) for a in recs[-1]["selected"]]
    assert len(set(picks)) == m + k and min(picks) >= 0
    blocked = run["blocked0"] if run["blocked0"].any() else None
    rounds = list(zip(range(m, m + k), recs, [True] * k))
    if m:  # the state the conditioning leaves: round m - 1; xcol is not part of it (the batched
        rounds.insert(0, (m - 1, run["cond"], False))  # kernels keep their columns in scratch)
        assert picks[:m] == run["placed"]
    e_cpu = _e_cpu(name, n, picks, blocked, rounds[0][0])
    tol = R.tolerance(e_cpu)
    worst = {key: 0.0 for key in R.ERROR_KEYS}
    for r, rec, has_xcol in rounds:
        assert [int(a) for a in rec["selected"][:r + 1]] == picks[:r + 1]
        e = R.round_errors(ref, n, picks, r, rec["delta"], rec["piv"],
                           rec["xcol"] if has_xcol else None, blocked)
        # the threshold distance, on the device's own picks
        assert e["min_nom"] >= R.MIN_DISTANCE and e["min_den"] >= R.MIN_DISTANCE, (label, r, e)
        for key in R.ERROR_KEYS:
            worst[key] = max(worst[key], e[key])
        if has_xcol:  # a free round: sel_delta is the fresh delta of the pick, xcol is zero above a
            assert e["xcol_above"] == 0, (label, r)
            y = picks[r]
            assert _same(rec["sel_delta"][r:r + 1], rec["delta"][y:y + 1]), (label, r)
    dev = max(worst.values())
    print(f"greedy state {label}: n {n} rounds {len(rounds)} e_cpu {e_cpu:.2e} tol {tol:.2e} "
          f"device max {dev:.2e} (" + " ".join(f"{key} {v:.1e}" for key, v in worst.items()) + ")")
    for key, v in worst.items():
        assert v <= tol, (label, key, v, tol)


def _check_policy(label, run, lazy, cache_init):
    n = run["n"]
    cache, blocked = run["cache0"], run["blocked0"].copy()
    assert _same(cache, np.full(n, cache_init))
    total = 0
    for r, rec in enumerate(run["recs"]):
        d = rec["delta"]
        y, ev, after = R.lazy_round(cache, d, blocked, lazy)
        assert int(rec["selected"][r]) == y, (label, r)
        assert int(rec["evals"][r]) == len(ev), (label, r)
        assert _same(rec["cache"], after), (label, r)
        touched = np.zeros(n, dtype=bool)
        if lazy:
            touched[ev] = True
            assert _same(rec["cache"][touched], d[touched]), (label, r)
        assert _same(rec["cache"][~touched], cache[~touched]), (label, r)
        assert not (touched & blocked).any()
        total += len(ev)
        cache = rec["cache"]
        blocked[y] = True
    # masked (and selected) entries are never evaluated: they keep the initial value for good
    assert _same(cache[run["blocked0"]], np.full(int(run["blocked0"].sum()), cache_init))
    return total


# ---- (a) arithmetic and (b) policy, on the same runs ----
MODES = [pytest.param(True, id="lazy"), pytest.param(False, id="full")]
INPUTS = [("F1", n) for n in R.F1_ORDERS] + [("F2", None), ("F3", None)]
INPUT_IDS = [f"{name}-{n}" if n else name for name, n in INPUTS]


@pytest.mark.parametrize("lazy", MODES)
@pytest.mark.parametrize("name,n", INPUTS, ids=INPUT_IDS)
def test_arithmetic(name, n, lazy):
    _check_arithmetic(f"{name}-{n or 'full'} {'lazy' if lazy else 'full'}", name,
                      _run(name, n, lazy))


@pytest.mark.parametrize("lazy", MODES)
@pytest.mark.parametrize("name,n", INPUTS, ids=INPUT_IDS)
def test_policy(name, n, lazy):
    _check_policy(f"{name}-{n}", _run(name, n, lazy), lazy, R.FIXTURES[name][2][2])


def test_policy_finite_cache_init():
    """cache_init = 50.0 lies inside the range of the deltas: a stale 50.0 beats most fresh values
    (it is evaluated), a fresh value above it is selected without evaluating the rest."""
    run = _run("F1", None, True, cache_init=50.0)
    total = _check_policy("F1 cache_init 50", run, True, 50.0)
    d0 = run["recs"][0]["delta"]
    assert d0.max() > 50.0 > d0.min()
    assert 0 < total < run["n"]                   # never a bulk evaluation of everyone
    _check_arithmetic("F1 cache_init 50 lazy", "F1", run)


def test_policy_tied_cache_init():
    """cache_init = the largest round-0 delta, bit for bit: every stale entry ties with the best
    fresh key F* at index fi.  Ties go to the lower index, so exactly the entries 0 .. fi are
    evaluated in round 0 (fi itself last, then selected) and the entries above fi, the second
    candidate chunk included, keep the stale value."""
    d0 = _run("F1", None, True)["recs"][0]["delta"]
    fi = int(np.argmax(d0))
    assert 0 < fi < 1024 and np.count_nonzero(d0 == d0[fi]) == 1
    run = _run("F1", None, True, cache_init=float(d0[fi]))
    _check_policy("F1 cache_init tied", run, True, float(d0[fi]))
    rec = run["recs"][0]
    assert int(rec["selected"][0]) == fi and int(rec["evals"][0]) == fi + 1
    assert _same(rec["cache"][fi + 1:], np.full(run["n"] - fi - 1, d0[fi]))
    _check_arithmetic("F1 cache_init tied lazy", "F1", run)


def test_policy_masked():
    """Every third location blocked: never picked, never evaluated, never counted, cache kept; its
    nom / prec still enter nothing the others read (it stays in A_bar: the reference state is the
    unmasked one)."""
    run = _run("F1", None, True, masked=True)
    _check_policy("F1 masked", run, True, np.inf)
    assert run["recs"][0]["evals"][0] == int((~run["blocked0"]).sum())
    assert not run["blocked0"][run["recs"][-1]["selected"]].any()
    _check_arithmetic("F1 masked lazy", "F1", run)


# ---- (c) slab split == the whole, bit for bit ----
@pytest.mark.parametrize("c", [511, 1024, 1025])
def test_slab_split_is_the_whole_step(c):
    """vgposp_greedy_update_ex over [0, c) and [c, n) + vgposp_greedy_select(0, n) is
    vgposp_greedy_step (include/vgposp.h: "With c0 = 0, c1 = n ... this is exactly
    vgposp_greedy_step"): in greedy_trmv_kernel one thread forms each column's sum, in an order
    that does not depend on the tile origin (cbeg & ~1)."""
    K, _, prm = R.fixture("F1")
    n, k = K.shape[0], R.ROUNDS
    whole = _run("F1", None, True)["recs"]
    split = Greedy(K, n, k, prm).init()
    other = Greedy(K, n, k, prm).init()     # as split; its last select does not own the pick
    for r in range(k):
        for g in (split, other):
            g.update(r, 0, c)
            g.update(r, c, n)
        split.select(r, True, 0, n)
        got = split.read()
        for key in STATE_KEYS + ("xcol",):
            assert _same(got[key], whole[r][key]), (c, r, key)
        if r < k - 1:
            other.select(r, True, 0, n)
        else:
            y = int(whole[r]["selected"][r])
            s0, s1 = (c, n) if y < c else (0, c)
            other.select(r, True, s0, s1)
            rec = other.read()
            assert int(rec["selected"][r]) == y
            assert _same(rec["piv"][:2 + 2 * r], np.zeros(2 + 2 * r))
            for key in ("delta", "cache", "selected", "sel_delta", "evals"):
                assert _same(rec[key], whole[r][key]), (c, r, key)
    # the column of L^-1 by vgposp_greedy_extract: zeros unless the owner range holds the pick
    r = k - 1
    a = int(whole[r]["selected"][r - 1])
    lo, hi = (a + 1, n) if a < c else (0, a)
    split.extract(r, lo, hi)
    assert _same(split.read()["xcol"], np.zeros(n))
    split.extract(r, a, a + 1)
    assert _same(split.read()["xcol"], whole[r]["xcol"])
    split.extract(r, 0, n)
    assert _same(split.read()["xcol"], whole[r]["xcol"])


# ---- (d) conditioning on installed sensors ----
@pytest.mark.parametrize("batch", [1, 4, 8])
def test_conditioning(batch):
    """vgposp_greedy_condition on six sensors (five columns: 4 + 1 with T = 4, one short batch with
    T = 8), then two free rounds: the state the conditioning leaves (A = placed[:5], pivots of
    placed[5]), then A = placed and A = placed + pick.  The batched kernels sum in another order
    (their own row loop: greedy_trmv_batch_kernel), so the batch sizes are each held to the
    reference here, and to each other, to rounding, in test_conditioning_widths."""
    run = _run("F1", None, True, placed=tuple(R.PLACED), batch=batch, k=2)
    _check_arithmetic(f"F1 placed batch {batch}", "F1", run)


# nine conditioned columns (8 + 1 with T = 8, 4 + 4 + 1 with T = 4): a sensor at index 0 and one
# at n - 1, both sides of both row-chunk boundaries, several columns in one chunk
PLACED_EDGES = (0, 1039, 511, 512, 513, 1024, 3, 700, 1023, 64)
WIDTHS_RTOL = 1e-10   # the cross-width tolerance of tests/test_gpu_constrained.py


@pytest.mark.parametrize("placed,lda,batches", [
    pytest.param(tuple(R.PLACED), None, (1, 4, 8), id="placed"),
    pytest.param(PLACED_EDGES, None, (1, 4, 8), id="edges"),
    pytest.param(PLACED_EDGES, 1041, (1, 4), id="edges-lda1041"),   # the scalar-load path
])
def test_conditioning_widths(placed, lda, batches):
    """The batch sizes against each other, after the conditioning and after each of two free
    rounds (workspace and scratch start as 0xFF bytes): picks and evaluation counts are equal,
    the extracted column of a free round is byte-equal, and delta, cache, pivots and pick deltas
    agree to WIDTHS_RTOL (greedy_trmv_batch_kernel sums a column in another order than
    greedy_trmv_kernel).  Every width is also held to the longdouble reference at the tolerance
    of test_arithmetic."""
    runs = {b: _run("F1", None, True, placed=placed, batch=b, lda=lda, k=2) for b in batches}
    one = runs[1]
    m, n = len(placed), one["n"]
    for b in batches:
        _check_arithmetic(f"F1 {m} placed lda {lda or n} batch {b}", "F1", runs[b])
        stages = [("conditioning", m - 1, one["cond"], runs[b]["cond"])]
        stages += [(f"round {i}", m + i, x, y)
                   for i, (x, y) in enumerate(zip(one["recs"], runs[b]["recs"]))]
        for when, r, want, got in stages:
            assert _same(got["selected"], want["selected"]), (b, when)
            assert _same(got["evals"], want["evals"]), (b, when)
            free = np.ones(n, dtype=bool)
            free[want["selected"][:r + 1]] = False
            assert np.isfinite(want["delta"][free]).all(), when
            np.testing.assert_allclose(got["delta"][free], want["delta"][free], rtol=WIDTHS_RTOL)
            stale = np.isinf(want["cache"])            # never evaluated: the initial value
            assert _same(got["cache"][stale], want["cache"][stale]), (b, when)
            np.testing.assert_allclose(got["cache"][~stale], want["cache"][~stale],
                                       rtol=WIDTHS_RTOL)
            # pivots: nom_y, P_yy; the row of W (Sigma alone: no mat-vec in it); the row of V,
            # differences of the q's, so to the row's scale
            np.testing.assert_allclose(got["piv"][:2], want["piv"][:2], rtol=WIDTHS_RTOL)
            assert _same(got["piv"][2:2 + r], want["piv"][2:2 + r]), (b, when)
            v = want["piv"][2 + r:2 + 2 * r]
            np.testing.assert_allclose(got["piv"][2 + r:2 + 2 * r], v, rtol=WIDTHS_RTOL,
                                       atol=WIDTHS_RTOL * np.abs(v).max())
            np.testing.assert_allclose(got["sel_delta"], want["sel_delta"], rtol=WIDTHS_RTOL)
            if r >= m:
                assert _same(got["xcol"], want["xcol"]), (b, when)


# ---- (e) layouts at the ABI ----
@pytest.mark.parametrize("lazy", MODES)
@pytest.mark.parametrize("lda,shift", [(1041, 0), (1042, 0), (1042, 1)])
def test_layouts(lda, shift, lazy):
    """Odd lda (scalar loads), even lda with row padding (16-byte loads), and an even lda on a base
    8 bytes off 16-byte alignment (scalar loads again)."""
    K, _, _ = R.fixture("F1")
    n = K.shape[0]
    run = _run("F1", None, lazy, lda=lda, shift=shift, k=3)
    _check_arithmetic(f"F1 lda {lda} shift {shift} {'lazy' if lazy else 'full'}", "F1", run)
    _check_policy(f"F1 lda {lda} shift {shift}", run, lazy, np.inf)
    iu = np.triu_indices(n, 1)
    for when in ("after_init", "after_rounds"):
        buf, buf0 = run[when], run["host0"]
        assert _same(buf[:shift], buf0[:shift]), when           # ahead of the base
        M, M0 = buf[shift:].reshape(n, lda), buf0[shift:].reshape(n, lda)
        assert _same(M[:, n:], M0[:, n:]), when                  # the padding of every row
        assert _same(M[:, :n][iu], K[iu]), when                  # Sigma is kept above the diagonal
