"""Candidate set and pre-installed sensors of a constrained greedy placement: validation only.

Krause's algorithm splits the locations V into S (where a sensor may go) and U (whose uncertainty
counts but where none can be put) and may start from sensors A0 that are already installed; the
reference assumes U empty and A0 = [] (placement_algorithm2.py:128-160).  This module normalises
the two user arguments; it uses no device and imports only numpy.
"""
from __future__ import annotations

import numpy as np


def _index_array(name, idx, N):
    try:
        a = np.asarray(idx)
    except Exception as e:  # ragged input
        raise ValueError(f"{name} must be a list of indices: {e}") from e
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must hold integer indices, got dtype {a.dtype}")
    a = a.astype(np.int64)
    bad = a[(a < 0) | (a >= N)]
    if bad.size:
        raise ValueError(f"{name} index {int(bad[0])} is outside [0, {N})")
    u, c = np.unique(a, return_counts=True)
    if (c > 1).any():
        raise ValueError(f"{name} holds index {int(u[c > 1][0])} more than once")
    return a


def normalize_constraints(N, k, candidates=None, placed=None):
    """-> ``(allowed, placed)``: ``allowed`` a bool mask [N] (None when ``candidates`` is None:
    every location is a candidate), ``placed`` an int64 array (A0 in the given order, possibly
    empty).

    ``candidates`` is an index list or a boolean mask of length N; ``placed`` is an index list and
    need not lie inside ``candidates``.  Raises ValueError on a mask of the wrong length, an index
    outside [0, N), a duplicate index, or ``k`` larger than the number of free candidates
    ``|candidates \\ placed|``."""
    N, k = int(N), int(k)
    if N < 1:
        raise ValueError(f"N must be positive, got {N}")
    if k < 0:
        raise ValueError(f"k must not be negative, got {k}")
    allowed = None
    if candidates is not None:
        c = np.asarray(candidates)
        if c.dtype == np.bool_:
            if c.shape != (N,):
                raise ValueError(f"a candidates mask must have length {N}, got shape {c.shape}")
            allowed = c.copy()
        else:
            allowed = np.zeros(N, dtype=bool)
            allowed[_index_array("candidates", candidates, N)] = True
    A0 = np.zeros(0, dtype=np.int64) if placed is None else _index_array("placed", placed, N)
    free = np.ones(N, dtype=bool) if allowed is None else allowed.copy()
    free[A0] = False
    nfree = int(free.sum())
    if k > nfree:
        raise ValueError(f"k = {k} exceeds the {nfree} candidates that are not already placed")
    return allowed, A0


def reject_constraints(what, candidates=None, placed=None):
    """For the paths that do not implement constraints: never ignore them silently."""
    if candidates is not None or placed is not None:
        raise ValueError(f"{what} does not support candidates / placed; use "
                         "placement_algorithm2.placement_algorithm_1 / _2 or GreedyPlacement")
