"""Test oracle: greedy MI placement with a candidate set and pre-installed sensors.

The loops of placement_algorithm2.py:151-219 (lazy) and :128-145 (full) with three changes:
``A`` starts as ``placed`` (A0, in the given order), ``A_bar`` starts as V \\ A0, and the arg-max
loops run over ``candidates \\ A`` instead of V \\ A.  ``nominator`` and ``denominator`` are the
unconstrained ones (``oracle.placement``), so A_bar keeps every non-candidate location.

* ``constrained_lazy`` / ``constrained_full``: restated on ``oracle.placement.nominator``,
  ``denominator`` and ``_delta`` (one pinv per evaluation: small N only).
* ``constrained_fast``: the same decisions from ``oracle.placement.all_deltas`` with the mask
  applied at the arg-max (one inverse per round).
Each returns ``(picks, selected deltas, evaluations per round, relative gap per round)``; the gap is
(best - second best) / |best| of the fresh deltas over the allowed candidates of that round.
"""
from __future__ import annotations

import numpy as np

from oracle import placement as op


def candidate_list(N, candidates=None):
    if candidates is None:
        return list(range(N))
    c = np.asarray(candidates)
    if c.dtype == np.bool_:
        return [int(i) for i in np.flatnonzero(c)]
    return sorted(int(i) for i in c)


def _scalar(x):
    return float(np.asarray(x).reshape(-1)[0])


def _gap(values):
    """Relative gap between the best and the second-best of ``values`` (inf for a single one)."""
    v = np.sort(np.asarray(values, dtype=np.float64))[::-1]
    if len(v) < 2:
        return float("inf")
    return float((v[0] - v[1]) / abs(v[0])) if v[0] != 0 else 0.0


def _fresh(y, A, A_bar, cov, nominator, denominator):
    return _scalar(op._delta(nominator(y, A, cov), denominator(y, A_bar, cov)))


def constrained_lazy(cov_vv, k, candidates=None, placed=(), nominator=op.nominator,
                     denominator=op.denominator, argmax=op.argmax_cache_linear, gaps=True):
    """placement_algorithm2.py:151-219 with A = placed, A_bar = V \\ placed, arg-max over
    candidates \\ A.  The cache starts at +inf for every candidate."""
    cov = np.asarray(cov_vv, dtype=np.float64)
    N = cov.shape[0]
    S = candidate_list(N, candidates)
    A = [int(a) for a in placed]
    A_bar = [v for v in range(N) if v not in set(A)]
    cache = [float("inf")] * N
    picks, deltas, evals, gap = [], [], [], []
    while len(picks) < k:
        uptodate = [False] * N
        cnt = 0
        if gaps:
            gap.append(_gap([_fresh(y, A, A_bar, cov, nominator, denominator)
                             for y in S if y not in A]))
        while True:
            y_st = int(argmax(cache, A, S))
            if uptodate[y_st]:
                break
            cache[y_st] = _fresh(y_st, A, A_bar, cov, nominator, denominator)
            uptodate[y_st] = True
            cnt += 1
        picks.append(y_st)
        deltas.append(cache[y_st])
        evals.append(cnt)
        A.append(y_st)
        A_bar.remove(y_st)
    return picks, deltas, evals, gap


def constrained_full(cov_vv, k, candidates=None, placed=(), nominator=op.nominator,
                     denominator=op.denominator):
    """placement_algorithm2.py:128-145 (argmax_ :105-125) with the same three changes; the
    evaluations of a round are the candidates scored, |candidates \\ A|."""
    cov = np.asarray(cov_vv, dtype=np.float64)
    N = cov.shape[0]
    S = candidate_list(N, candidates)
    A = [int(a) for a in placed]
    A_bar = [v for v in range(N) if v not in set(A)]
    picks, deltas, evals, gap = [], [], [], []
    while len(picks) < k:
        y_st, delta_st, vals = -1, -1, []
        for y in S:
            if y in A:
                continue
            d = _fresh(y, A, A_bar, cov, nominator, denominator)
            vals.append(d)
            if delta_st < d:
                delta_st, y_st = d, y
        picks.append(y_st)
        deltas.append(delta_st)
        evals.append(len(vals))
        gap.append(_gap(vals))
        A.append(y_st)
        A_bar.remove(y_st)
    return picks, deltas, evals, gap


def constrained_fast(cov_vv, k, candidates=None, placed=(), lazy=True, jitter=0.0,
                     thr=op.DELTA_EPS, cache_init=np.inf, pinv=False):
    """The same decisions from all_deltas (one inverse per round), the mask applied at the arg-max.
    ``pinv=True`` takes the deltas of a singular covariance from the pinv restatement instead."""
    cov = np.asarray(cov_vv, dtype=np.float64)
    N = cov.shape[0]
    blocked = np.ones(N, dtype=bool)
    blocked[candidate_list(N, candidates)] = False
    A = [int(a) for a in placed]
    blocked[A] = True
    cache = np.full(N, float(cache_init))
    picks, deltas, evals, gap = [], [], [], []
    for _ in range(k):
        if pinv:
            A_bar = [v for v in range(N) if v not in set(A)]
            delta = np.array([np.nan if v in set(A) else
                              _fresh(v, A, A_bar, cov, op.nominator, op.denominator)
                              for v in range(N)])
        else:
            delta, _, _ = op.all_deltas(cov, A, jitter, thr)
        free = np.flatnonzero(~blocked)
        gap.append(_gap(delta[free]))
        if lazy:
            y, ev = op._lazy_select_np(cache, delta, blocked)
            evals.append(len(ev))
        else:
            y = int(free[np.argmax(delta[free])])
            evals.append(len(free))
        picks.append(int(y))
        deltas.append(float(delta[y]))
        A.append(int(y))
        blocked[y] = True
    return picks, deltas, evals, gap


def deleted_rows_picks(cov_vv, k, candidates):
    """The WRONG way to exclude locations: delete their rows and columns, then run the
    unconstrained full greedy.  Returns (picks in the original numbering, deltas)."""
    keep = np.asarray(candidate_list(np.shape(cov_vv)[0], candidates))
    sub = np.asarray(cov_vv)[np.ix_(keep, keep)]
    p, d, _, _ = constrained_fast(sub, k, lazy=False)
    return [int(keep[i]) for i in p], d
