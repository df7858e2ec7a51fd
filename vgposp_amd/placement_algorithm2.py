"""Greedy mutual-information sensor placement on MI355X — drop-in for the reference's
``placement_algorithm2`` module (``/root/reference/placement_algorithm2.py``).

Same names, argument meaning and results:

* ``placement_algorithm_2(cov_vv, k)``  lazy greedy, Krause Alg. 2    (reference :151-219)
* ``placement_algorithm_1(cov_vv, k)``  full greedy                   (reference :128-145)
* ``cov_vv_4x4()``                      the reference's 4x4 fixture    (reference :473-479)
* ``dg_create_random_cov(n)``           U U^T test covariance          (reference :441-444)

``cov_vv`` is an [N, N] float64 covariance (numpy array or device tensor); the result is a Python
list of ``np.int64`` indices in selection order.  The computation runs entirely in libvgposp
(``vgposp_greedy_init`` / ``vgposp_greedy_step``): one in-place Cholesky + inverse of Sigma, then
per selection one HBM-bound triangular mat-vec and a handful of O(N) kernels; the lazy-cache
decisions of the reference are reproduced exactly on device (see csrc/greedy.hip).

``GreedyPlacement`` is the device-resident form used by ``bench.py`` (inputs already in HBM, no
host round trip between selections).
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import linalg
from ._lib import CholeskyError, call, query
from .constraints import normalize_constraints
from .linalg import _p, _stream

# Sensors whose columns q_a = M^T (M e_a) one pass over L^-1 forms while conditioning on ``placed``
# (vgposp_greedy_condition: 1, 4 or 8).
CONDITION_BATCH = 8


class GreedyPlacement:
    """Device-resident greedy placement on an [N, N] covariance held in HBM.

    ``Sigma`` (float64, contiguous, lda = N) is FACTORED IN PLACE by ``init()``: its lower triangle
    becomes L^-1, the strictly upper triangle (Sigma itself) and the saved diagonal are what the
    nominators read.  Pass ``copy=True`` to work on a private copy.

    ``candidates`` (index list or boolean mask of length N) restricts where a sensor may go: the
    other locations are never picked but stay in A_bar, so every denominator still conditions on
    them.  ``placed`` (index list, in order, not necessarily inside ``candidates``) are sensors
    already installed: ``init()`` conditions the state on them (``condition_batch`` of their
    columns per pass over L^-1) and the rounds continue from there.  ``kmax``, ``rounds`` and
    ``result()`` count the new picks only; ``placed`` holds A0.
    """

    def __init__(self, Sigma, kmax, copy=False, jitter=0.0, threshold=1e-8,
                 cache_init=float("inf"), pad_odd=False, candidates=None, placed=None,
                 condition_batch=None):
        S = linalg.as_device(Sigma)
        if S.dim() != 2 or S.shape[0] != S.shape[1]:
            raise ValueError("cov_vv must be a square matrix")
        self.N = int(S.shape[0])                     # candidates
        if not (1 <= kmax <= self.N):
            raise ValueError(f"k must be in [1, {self.N}], got {kmax}")
        self.constrained = candidates is not None or placed is not None
        self.allowed, self.placed = (normalize_constraints(self.N, kmax, candidates, placed)
                                     if self.constrained else (None, np.zeros(0, np.int64)))
        self.m = len(self.placed)                    # |A0|: forced rounds before the first pick
        self.condition_batch = CONDITION_BATCH if condition_batch is None else int(condition_batch)
        if self.condition_batch not in (1, 4, 8):
            raise ValueError(f"condition_batch must be 1, 4 or 8, got {condition_batch}")
        # pad_odd (with copy): an odd order is factored as [Sigma 0; 0 s] at N + 1, so every
        # recursion level runs on the fast (even-leading-dimension) GEMM; the padding candidate is
        # excluded on device after init (vgposp_greedy_exclude) and couples to nothing
        self.padded = bool(pad_odd and copy and self.N % 2 == 1 and self.N > 1)
        if self.padded:
            n = self.N
            P = torch.zeros((n + 1, n + 1), dtype=torch.float64, device=S.device)
            P[:n, :n].copy_(S)
            P[n, n] = torch.diagonal(S).mean()
            self.S = P
        else:
            self.S = S.clone() if copy else S
        self.n = int(self.S.shape[0])                # the library's order
        self.k = int(kmax)                           # new picks
        self.kmax = self.k + self.m                  # the library's rounds: A0, then the picks
        dev = self.S.device
        self.ws = linalg.workspace(query("vgposp_greedy_workspace_bytes", self.n, self.kmax))
        self.info = torch.zeros(1, dtype=torch.int32, device=dev)
        self.selected = torch.full((self.kmax,), -1, dtype=torch.int64, device=dev)
        self.sel_delta = torch.zeros(self.kmax, dtype=torch.float64, device=dev)
        self.evals = torch.zeros(self.kmax, dtype=torch.int64, device=dev)
        self.rounds = 0
        # (jitter, |nom|/|denom| threshold, initial cache): (0, 1e-8, inf) is placement_algorithm2;
        # (1e-6, 1e-7, 1e8) is the TF variant snippets_a2.sparse_placement_algorithm_2
        self.params = (float(jitter), float(threshold), float(cache_init))
        self._lazy = True                            # the mode of the last step()
        # the constraints are uploaded here, so that init() only enqueues work (graph capture)
        self._blocked = self._allowed_dev = self._placed_dev = self._cond_ws = None
        if self.constrained:
            allowed = np.zeros(self.n, dtype=bool)   # the odd-order padding is never allowed
            allowed[: self.N] = True if self.allowed is None else self.allowed
            if self.allowed is not None:
                self._allowed_dev = torch.as_tensor(allowed.astype(np.uint8), device=dev)
            allowed[self.placed] = False
            self.free = int(allowed.sum())           # |candidates \ A0|
            # never an arg-max: not a candidate, or in A0
            self._blocked = torch.as_tensor(~allowed[: self.N], device=dev)
        if self.m:
            self._placed_dev = torch.as_tensor(self.placed, dtype=torch.int64, device=dev)
            self._cond_ws = linalg.workspace(query("vgposp_greedy_condition_workspace_bytes",
                                                   self.n, self.condition_batch))

    def init(self):
        call("vgposp_greedy_init_ex", _p(self.S), self.n, self.S.stride(0), self.kmax,
             *self.params, _p(self.info), _p(self.ws), self.ws.numel(), _stream())
        if self.padded:
            call("vgposp_greedy_exclude", _p(self.ws), self.n, self.kmax, self.N, _stream())
        if self.constrained:
            self.constrain()
        self.rounds = 0
        return self

    def constrain(self):
        """The constrained part of init(), on the state the factorization leaves: mask the
        non-candidates, then the forced rounds on ``placed``."""
        if self._allowed_dev is not None:
            call("vgposp_greedy_mask", _p(self.ws), self.n, self.kmax, _p(self._allowed_dev),
                 _stream())
        if self.m:
            call("vgposp_greedy_condition", _p(self.S), self.n, self.S.stride(0), self.kmax,
                 self.m, self.k, self.condition_batch, _p(self._placed_dev), _p(self.selected),
                 _p(self.ws), self.ws.numel(), _p(self._cond_ws), self._cond_ws.numel(),
                 _stream())

    def cache(self):
        """Device view of the lazy cache (delta_cached) [n] inside the workspace."""
        c = ctypes.c_void_p()
        call("vgposp_greedy_cache", _p(self.ws), self.n, self.kmax, ctypes.byref(c))
        off = c.value - self.ws.data_ptr()
        return self.ws[off:off + 8 * self.N].view(torch.float64)

    def check(self):
        linalg.check_info(self.info)

    def step(self, lazy=True):
        if self.rounds >= self.k:
            raise RuntimeError("all k sensors already placed")
        call("vgposp_greedy_step", _p(self.S), self.n, self.S.stride(0), self.kmax,
             self.m + self.rounds, int(lazy), _p(self.selected), _p(self.sel_delta),
             _p(self.evals), _p(self.ws), self.ws.numel(), _stream())
        self._lazy = bool(lazy)
        self.rounds += 1

    def run(self, k=None, lazy=True):
        k = self.k if k is None else k
        self.init()
        for _ in range(k):
            self.step(lazy)
        return self

    def step_traced(self, trace):
        """A lazy step() that also appends the reference's per-evaluation records to ``trace``: one
        ``(y, delta_y)`` per delta evaluated this round, in the reference's order, then
        ``('select', y*)`` — what placement_algorithm2.py:205 and :188 print.

        The lazy loop (:183-208) evaluates the stale cache entries in descending key order (value,
        then lower index) and stops at the first fresh arg-max, so the evaluated entries are the
        first ``evals[r]`` of the pre-round cache sorted by key, and their deltas are the
        post-round cache values.  The device makes every decision; this only reads back the two
        cache states and the evaluation count."""
        r = self.rounds
        cache = self.cache()
        key = torch.nan_to_num(cache.clone(), nan=-float("inf"))
        if r:
            key[self.selected[self.m:self.m + r]] = -float("inf")
        if self._blocked is not None:  # the reference's loop runs over candidates \ A only
            key[self._blocked] = -float("inf")
        self.step(lazy=True)
        order = torch.sort(key, descending=True, stable=True).indices[: int(self.evals[self.m + r])]
        for c, d in zip(order.cpu().numpy(), cache[order].cpu().numpy()):
            trace.append((int(c), float(d)))
        trace.append(("select", int(self.selected[self.m + r])))

    def result(self):
        """Selections (host list of np.int64), their deltas, and per-round evaluation counts.
        With ``placed``, these are the new picks only (A0 is ``self.placed``)."""
        self.check()
        new = slice(self.m, self.m + self.rounds)
        sel = self.selected[new].cpu().numpy()
        if (sel < 0).any():
            raise RuntimeError("greedy placement found no candidate (all deltas NaN?)")
        evals = self.evals[new].cpu().numpy()
        if self.constrained and not self._lazy:
            # full greedy scores every candidate outside A (argmax_, :105-125): |candidates \ A|
            evals = self.free - np.arange(self.rounds, dtype=np.int64)
        return [np.int64(s) for s in sel], self.sel_delta[new].cpu().numpy(), evals


# A singular (PSD, not PD) cov_vv, e.g. an empirical covariance with fewer samples than locations
# (main.py:125-350): the reference's pinv still defines every delta.  The device path then factors
# Sigma + eps I with a relative eps and takes denom = 1 / P_yy - eps (vgposp_greedy_init_ex's
# jitter), so a candidate in the span of the others gets denom ~ 0 -> delta 0 at the 1e-8
# threshold, as with pinv, and every other delta moves by O(eps).
# A factorization can also "succeed" on a singular cov_vv: a zero pivot that rounds to a tiny
# positive value.  L^-1 then turns rounding noise into large deltas where pinv gives 0, so a pivot
# ratio L_ii^2 / sigma_ii below PIVOT_RTOL * n (rounding level) is treated like a failed pivot.
SINGULAR_EPS = (1e-12, 1e-10, 1e-8)
PIVOT_RTOL = 100 * np.finfo(np.float64).eps


def _check_pivots(g, sdiag):
    """After init(): raise CholeskyError if a pivot of Sigma = L L^T is at rounding level.  The
    factored buffer holds M = L^-1, so L_ii^2 / sigma_ii = 1 / (M_ii^2 sigma_ii)."""
    g.check()
    m = torch.diagonal(g.S)
    ratio = 1.0 / (m * m * sdiag)
    i = int(torch.argmin(ratio))
    if not float(ratio[i]) >= PIVOT_RTOL * g.n:
        raise CholeskyError(i + 1)


def _rounds(g, k, lazy, trace):
    for _ in range(k):
        if trace is not None:
            g.step_traced(trace)
        else:
            g.step(lazy)
    return g.result()[0]


def _place(cov_vv, k, lazy, verbose, trace=None, candidates=None, placed=None):
    con = dict(candidates=candidates, placed=placed)
    if k < 1:
        if candidates is not None or placed is not None:
            normalize_constraints(int(np.shape(cov_vv)[0]), max(k, 0), candidates, placed)
        return []
    if verbose and trace is None:
        trace = []
    tr = None if trace is None else []
    try:
        g = GreedyPlacement(cov_vv, k, copy=True, pad_odd=True, **con)
        sdiag = torch.diagonal(g.S).clone()
        g.init()
        _check_pivots(g, sdiag)
        A = _rounds(g, k, lazy, tr)
    except CholeskyError as err:
        S = linalg.as_device(cov_vv)
        scale = float(torch.mean(torch.diagonal(S)).abs()) or 1.0
        for rel in SINGULAR_EPS:
            try:
                tr = None if trace is None else []
                g = GreedyPlacement(S, k, copy=True, jitter=rel * scale, pad_odd=True,
                                    **con).init()
                A = _rounds(g, k, lazy, tr)
                break
            except CholeskyError:
                continue
        else:
            raise err
    if trace is not None:
        trace.extend(tr)
    if verbose:  # the reference's lines, placement_algorithm2.py:205 and :188
        for t in trace:
            if t[0] == "select":
                print("y*=", t[1])
            else:
                print("delta_y=", t[1], "y_st=", t[0])
    return A


def placement_algorithm_2(cov_vv, k, verbose=False, trace=None, candidates=None, placed=None):
    """Lazy greedy MI placement (placement_algorithm2.py:151-219).  Returns k indices.

    ``candidates`` (index list or boolean mask of length N): the locations where a sensor may go;
    the others are never picked but still count in every denominator.  ``placed`` (index list):
    sensors already installed; the k new picks are returned, ``placed`` is not part of them.

    ``verbose=True`` prints the reference's per-evaluation lines (``delta_y= … y_st= …`` for every
    delta evaluated, ``y*= …`` per selection, :205 / :188); ``trace`` (a list) receives the same
    records as ``(y, delta)`` / ``('select', y)`` tuples without printing."""
    return _place(cov_vv, k, True, verbose, trace, candidates, placed)


def placement_algorithm_1(cov_vv, k, verbose=False, candidates=None, placed=None):
    """Full greedy MI placement (placement_algorithm2.py:128-145).  Returns k indices;
    ``candidates`` / ``placed`` as in ``placement_algorithm_2``."""
    return _place(cov_vv, k, False, verbose, None, candidates, placed)


def cov_vv_4x4():
    """The reference's fixture (placement_algorithm2.py:473-479)."""
    return np.array([[1.10, 0.31, 0.33, 0.27],
                     [0.31, 1.01, 0.30, 0.27],
                     [0.33, 0.30, 0.97, 0.33],
                     [0.27, 0.27, 0.33, 1.2]])


def dg_create_random_cov(n, rng=None):
    """placement_algorithm2.py:441-444."""
    r = np.random if rng is None else rng
    m = r.uniform(0, 1, n ** 2).reshape(-1, n)
    return np.dot(m, m.T)


def placement_from_points(X, k, kind="eq", amp=1.0, ls=1.0, noise=1e-2, jitter=1e-6, lazy=True,
                          candidates=None, placed=None, criterion="mi", targets=None,
                          target_points=None, target_weights=None, cross=None, cov="dense"):
    """Assemble Sigma = K(X, X) + (noise + jitter) I on device and place k sensors.

    ``criterion``: ``"mi"`` (mutual information, the default), or ``"variance"`` / ``"entropy"``
    (placement_criteria.CriterionPlacement on the same assembled matrix).  ``targets``, the
    locations whose posterior variance counts, belongs to ``"variance"`` alone.

    ``target_points`` Xt [P, d] (``"variance"`` alone, instead of ``targets``): the posterior
    variance of the latent field counts at these points, which need not be rows of X; the cross-
    covariance K(Xt, X) is assembled without noise.  ``target_weights`` [P] >= 0 weigh them.
    ``cross``: ``"dense"`` (the default) assembles K(Xt, X) [P, N] once; ``"matrix_free"`` never
    does and generates its entries from the points in every round (placement_criteria.CrossKernel),
    for a mesh whose cross-covariance does not fit the device.

    ``cov``: ``"dense"`` (the default) assembles Sigma [N, N]; ``"matrix_free"`` never does and
    generates it from the points in every round (placement_criteria.SiteKernel with the diagonal
    amp^2 + noise + jitter the assembly has), for site sets whose covariance does not fit the
    device.  It is for ``"variance"`` and ``"entropy"`` (the mutual-information placement factors
    Sigma) and, with ``target_points``, implies ``cross="matrix_free"``."""
    if cov not in ("dense", "matrix_free"):
        raise ValueError(f"unknown cov {cov!r}; expected 'dense' or 'matrix_free'")
    if cov == "matrix_free":
        if criterion == "mi":
            raise ValueError("cov='matrix_free' applies to criterion='variance' and 'entropy': "
                             "the mutual-information placement factors Sigma")
        if cross == "dense":
            raise ValueError("cov='matrix_free' and cross='dense' exclude each other: a stored "
                             "cross-covariance with a generated Sigma is not supported")
        if target_points is not None and cross is None:
            cross = "matrix_free"
    if cross is not None:
        if target_points is None:
            raise ValueError("cross needs target_points")
        if cross not in ("dense", "matrix_free"):
            raise ValueError(f"unknown cross {cross!r}; expected 'dense' or 'matrix_free'")
    if target_points is not None:
        if criterion != "variance":
            raise ValueError("target_points apply to criterion='variance' only")
        if targets is not None:
            raise ValueError("target_points and targets exclude each other")
        Xt = np.asarray(target_points, dtype=np.float64) if not isinstance(
            target_points, torch.Tensor) else target_points
        Xt = Xt[:, None] if Xt.ndim == 1 else Xt
        d = 1 if np.ndim(X) == 1 else np.shape(X)[1]
        if Xt.ndim != 2 or Xt.shape[1] != d:
            raise ValueError(f"target_points must be [P, {d}], got shape {tuple(Xt.shape)}")
    elif target_weights is not None:
        raise ValueError("target_weights need target_points")
    if criterion == "mi":
        if targets is not None:
            raise ValueError("targets apply to criterion='variance'; the mutual-information "
                             "placement has no target set")
    else:
        from .placement_criteria import CRITERIA
        if criterion not in CRITERIA:
            raise ValueError(f"unknown criterion {criterion!r}; expected 'mi' or one of "
                             f"{list(CRITERIA)}")
    if cov == "matrix_free":
        from .placement_criteria import CriterionPlacement, CrossKernel, SiteKernel
        site = SiteKernel(kind, X, amp, ls, noise=noise + jitter)
        gen = CrossKernel.from_site(site, Xt) if target_points is not None else None
        g = CriterionPlacement(site, k, criterion, candidates=candidates, placed=placed,
                               targets=targets, target_weights=target_weights,
                               cross_kernel=gen).run(k)
        return g.result()[0]
    K = linalg.kernel_matrix(kind, X, None, amp, ls, diag_shift=noise + jitter)[0]
    if criterion != "mi":
        from .placement_criteria import CriterionPlacement, CrossKernel
        R = gen = None
        if cross == "matrix_free":
            gen = CrossKernel(kind, X, Xt, amp, ls)
        elif target_points is not None:
            R = linalg.kernel_matrix(kind, Xt, X, amp, ls)[0]
        g = CriterionPlacement(K, k, criterion, candidates=candidates, placed=placed,
                               targets=targets, cross_cov=R, target_weights=target_weights,
                               cross_kernel=gen).run(k)
        return g.result()[0]
    g = GreedyPlacement(K, k, candidates=candidates, placed=placed).run(k, lazy=lazy)
    return g.result()[0]


def placement_from_samples(samples, k, criterion="variance", noise=0.0, tr_stdev=1.0,
                           candidates=None, placed=None, targets=None, cov="factored"):
    """Place k sensors on the empirical covariance of ``samples`` [N locations, S samples] plus
    diag(``noise``): the reference's placement covariance (tfp.stats.covariance of the tracer
    samples for every pair of locations, main.py:190-199).

    ``cov``: ``"factored"`` (the default) never forms the N x N matrix and runs the rounds on the
    centred samples themselves (placement_criteria.FactoredCovariance.from_samples): N S doubles
    on the device instead of N^2.  ``"variance"`` and ``"entropy"`` take any noise >= 0.  ``"mi"``
    (placement_criteria.FactoredMIPlacement) inverts Sigma through Woodbury's identity, so it needs
    noise > 0 at every location (ValueError otherwise, before any device work), and it is the
    full greedy on fresh deltas: every delta is fresh after the one stream over the samples a
    round needs anyway, so the lazy cache of ``placement_algorithm_2`` is not emulated.
    ``"dense"`` assembles ``covariance.empirical_cov(samples) + diag(noise)`` and runs the existing
    paths; its ``"mi"`` is the lazy ``placement_algorithm_2`` and takes noise = 0 (a singular Sigma
    is retried with jitter).  ``noise`` is a scalar or [N], ``targets`` belongs to ``"variance"``."""
    if cov not in ("dense", "factored"):
        raise ValueError(f"unknown cov {cov!r}; expected 'dense' or 'factored'")
    if criterion == "mi":
        if targets is not None:
            raise ValueError("targets apply to criterion='variance'; the mutual-information "
                             "placement has no target set")
        if cov == "factored":
            from .placement_criteria import (FactoredCovariance, placement_mutual_information,
                                             require_positive_noise)
            shape = tuple(np.shape(samples))
            if len(shape) == 2 and shape[0] >= 1:   # (from_samples reports any other shape)
                require_positive_noise(FactoredCovariance._noise_vector(noise, shape[0]))
            fac = FactoredCovariance.from_samples(samples, noise=noise, tr_stdev=tr_stdev)
            return placement_mutual_information(fac, k, candidates=candidates, placed=placed)
    else:
        from .placement_criteria import CRITERIA
        if criterion not in CRITERIA:
            raise ValueError(f"unknown criterion {criterion!r}; expected 'mi' or one of "
                             f"{list(CRITERIA)}")
    from .placement_criteria import CriterionPlacement, FactoredCovariance
    if cov == "factored":
        fac = FactoredCovariance.from_samples(samples, noise=noise, tr_stdev=tr_stdev)
        if k < 1:
            normalize_constraints(fac.N, max(int(k), 0), candidates, placed)
            return []
        g = CriterionPlacement(fac, k, criterion, candidates=candidates, placed=placed,
                               targets=targets).run(k)
        return g.result()[0]
    from .covariance import empirical_cov
    N = int(np.shape(samples)[0])
    nv = FactoredCovariance._noise_vector(noise, N)
    Sigma = empirical_cov(samples, tr_stdev=tr_stdev)
    if nv is not None:
        torch.diagonal(Sigma).add_(linalg.as_device(nv))
    if criterion == "mi":
        return _place(Sigma, k, True, False, None, candidates, placed)
    if k < 1:
        normalize_constraints(N, max(int(k), 0), candidates, placed)
        return []
    g = CriterionPlacement(Sigma, k, criterion, candidates=candidates, placed=placed,
                           targets=targets).run(k)
    return g.result()[0]


def reconstruct_from_samples(samples, sensors, readings, noise=0.0, obs_noise=0.0, tr_stdev=1.0):
    """What follows ``placement_from_samples``: ``(mean, variance)`` of the field at all N
    locations given ``readings`` [k] or [k, B] at ``sensors``, under the same covariance (the
    empirical covariance of ``samples`` plus diag(``noise``), main.py:190-199) with the samples'
    mean per location as the prior mean, never forming an N x N or N x k array
    (placement_criteria.FieldReconstruction).  ``obs_noise`` >= 0 is a scalar measurement-error
    variance on the sensors' own covariance."""
    from .placement_criteria import reconstruct_from_samples as run
    return run(samples, sensors, readings, noise=noise, obs_noise=obs_noise, tr_stdev=tr_stdev)
