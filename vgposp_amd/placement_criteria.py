"""Greedy sensor placement by variance reduction (A-optimal) and by entropy on MI355X: the two
baselines Krause, Singh & Guestrin judge the mutual-information placement against, and the rule
to use when the posterior variance of the field is what matters.

With Sigma = ``cov_vv``, A the sensors chosen so far (``placed`` included) and
C = Sigma - Sigma_{:,A} Sigma_AA^-1 Sigma_{A,:} the conditional covariance:

* ``criterion="variance"``: delta_y = sum_{v in T} C_vy^2 / C_yy — the drop of the targets' total
  posterior variance when y is added, so the deltas of a run sum to the total reduction;
* ``criterion="entropy"``:  delta_y = C_yy — the largest conditional variance.

C_yy < ``threshold`` gives delta_y = 0; the arg-max runs over ``candidates`` minus A, ties to the
lowest index; every round scores every free candidate.  ``candidates`` and ``placed`` mean what
they mean in ``placement_algorithm_2``; ``targets`` (index list or boolean mask, default every
location) are the locations whose uncertainty counts and need not intersect the candidates.

Nothing is factored (csrc/criteria.hip keeps nom = diag C, s_y = sum_T C_vy^2 and the pivoted
Cholesky rows W; the variance rule passes once per round over the upper triangle of Sigma with
``vgposp_symv_upper``), so a singular PSD covariance needs no jitter, and Sigma is only read.

Targets outside V: with ``cross_cov`` = R [P, N], the covariance between P targets that are no
rows of ``cov_vv`` (a finer mesh, the latent field without sensor noise) and the N locations, and
``target_weights`` = omega [P] >= 0 (default ones; cell volumes of an uneven mesh), the variance
rule is delta_y = sum_v omega_v D_vy^2 / C_yy with D = R - R_{:,A} Sigma_AA^-1 Sigma_{A,:}: the drop
of the weighted total posterior variance of the targets.  One pass per round over R
(``vgposp_gemv_t``) replaces the pass over Sigma; the state gains the target-side rows U.

A mesh too fine to store R: ``cross_kernel`` = ``CrossKernel(kind, points, target_points, amp,
ls, ...)`` instead of ``cross_cov`` runs the same rounds with every entry of R generated from the
2 d coordinates of its target and its location (``vgposp_kernel_gemv_t``), so the device holds
(P + N) d doubles instead of P N.

Sites too many to store Sigma: a ``SiteKernel(kind, points, amp, ls, scale=None, noise=0.0)`` in
the place of ``cov_vv`` is Sigma = diag(a) K(X, X) diag(a) + diag(noise), generated from the points
in every pass (``vgposp_kernel_symv``) and in the one column a round reads, so the device holds
N (d + 2) doubles instead of N^2.  With ``CrossKernel.from_site`` beside it nothing of size N^2 or
P N is held at all.

A covariance estimated from samples: a ``FactoredCovariance(F, noise=0.0)`` in the place of
``cov_vv`` is Sigma = F F^T + diag(noise); ``FactoredCovariance.from_samples(samples)`` is the
reference's empirical covariance of S samples per location (``covariance.empirical_cov``) without
the N x N matrix.  A pass is two streams over F (``vgposp_factor_symv``), the column of a round one,
so the device holds N S doubles instead of N^2.

Mutual information on that factor: where its noise is positive at every location,
``FactoredMIPlacement`` / ``placement_mutual_information`` run the reference's own criterion
(placement_algorithm2.py:371-413) through Woodbury's identity on an S x S matrix, O(N S) per round
and one stream over F (``vgposp_fmi_*``), as the full greedy on fresh deltas.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import linalg
from ._lib import call, query
from .constraints import _index_array, normalize_constraints
from .linalg import _p, _stream

CRITERIA = {"variance": 0, "entropy": 1}   # VGPOSP_CRIT_VARIANCE / VGPOSP_CRIT_ENTROPY


def normalize_targets(N, targets):
    """-> bool mask [N], or None when ``targets`` is None (every location counts).  ``targets`` is
    an index list or a boolean mask of length N; raises ValueError as
    ``constraints.normalize_constraints`` does for ``candidates``."""
    if targets is None:
        return None
    t = np.asarray(targets)
    if t.dtype == np.bool_:
        if t.shape != (N,):
            raise ValueError(f"a targets mask must have length {N}, got shape {t.shape}")
        return t.copy()
    mask = np.zeros(N, dtype=bool)
    mask[_index_array("targets", targets, N)] = True
    return mask


def _criterion_id(criterion):
    try:
        return CRITERIA[criterion]
    except (KeyError, TypeError):
        raise ValueError(f"unknown criterion {criterion!r}; expected one of {list(CRITERIA)}")


def _points(name, X):
    X = linalg.as_device(X)
    X = X[:, None] if X.dim() == 1 else X
    if X.dim() != 2 or X.shape[0] < 1:
        raise ValueError(f"{name} must be [count, d] with count >= 1, got {tuple(X.shape)}")
    return X.contiguous()


def _positive_scalars(amp, ls):
    for name, v in (("amp", amp), ("ls", ls)):
        if not (np.ndim(v) == 0 and np.isfinite(float(v)) and float(v) > 0.0):
            raise ValueError(f"{name} must be a finite, positive scalar, got {v!r}")
    return float(amp), float(ls)


def _host_vector(name, a, count):
    a = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a))
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (count,):
        raise ValueError(f"{name} must have length {count}, got shape {a.shape}")
    return a


def _scale(name, a, count):
    if a is None:
        return None
    a = _host_vector(name, a, count)
    if not np.isfinite(a).all() or (a <= 0.0).any():
        raise ValueError(f"{name} must be finite and positive")
    return linalg.as_device(a)


def _nonnegative(name, a, count):
    """-> host float64 [count], finite and not negative (a noise vector, the targets' weights)."""
    a = _host_vector(name, a, count)
    if not np.isfinite(a).all() or (a < 0.0).any():
        raise ValueError(f"{name} must be finite and not negative")
    return a


def _noise(noise, N):
    """-> host float64 [N] from a scalar or a vector."""
    return _nonnegative("noise", np.full(N, float(noise)) if np.ndim(noise) == 0 else noise, N)


def _field(kind, points, amp, ls, scale_name, scale):
    """What a SiteKernel and a CrossKernel hold of the sites, validated and on the device:
    (kind, X, N, d, amp_value, ls_value, amp, ls, scale)."""
    kind = linalg.kind_id(kind)
    X = _points("points", points)
    N, d = int(X.shape[0]), int(X.shape[1])
    if not 1 <= d <= 8:
        raise ValueError(f"points must have 1 <= d <= 8 coordinates, got {d}")
    amp_value, ls_value = _positive_scalars(amp, ls)
    return (kind, X, N, d, amp_value, ls_value, linalg._vec(amp_value), linalg._vec(ls_value),
            _scale(scale_name, scale, N))


class SiteKernel:
    """A covariance of the candidate sites that is never stored: Sigma = diag(scale) K(points,
    points) diag(scale) + diag(noise) for one stationary kernel ``kind`` (``amp``, ``ls`` scalars)
    under a per-point amplitude field.  ``points`` [N, d], d <= 8; ``scale`` [N] (default ones) is
    finite and positive; ``noise`` (a scalar or [N]) is finite and not negative.  It goes where
    ``cov_vv`` goes in ``CriterionPlacement`` and the placement functions.  The device holds the
    points, the scale and the diagonal scale^2 amp^2 + noise: N (d + 2) doubles instead of N^2."""

    def __init__(self, kind, points, amp, ls, scale=None, noise=0.0):
        (self.kind, self.X, self.N, self.d, self.amp_value, self.ls_value, self.amp, self.ls,
         self.scale) = _field(kind, points, amp, ls, "scale", scale)
        noise = _noise(noise, self.N)
        a = np.ones(self.N) if self.scale is None else self.scale.cpu().numpy()
        self.diag = linalg.as_device(a * a * (self.amp_value * self.amp_value) + noise)

    def field(self):
        """The site side as ``CrossKernel.from_site`` shares it (the noise is no part of it)."""
        return (self.kind, self.X, self.N, self.d, self.amp_value, self.ls_value, self.amp,
                self.ls, self.scale)

    def args(self):
        """(kind, X, N, d, amp, ls, site_scale, diag) as the vgposp_critg_* entries take them."""
        return (self.kind, _p(self.X), self.N, self.d, _p(self.amp), _p(self.ls), _p(self.scale),
                _p(self.diag))


class FactoredCovariance:
    """A covariance given by a factor and never stored: Sigma = F F^T + diag(noise), F [N, S] with
    1 <= S <= 4096.  A device float64 ``F`` with unit column stride (a view with a row pitch
    included) is used where it lies and only read; anything else is copied to the device.
    ``noise`` (a scalar or [N]) is finite and not negative.  It goes where ``cov_vv`` goes in
    ``CriterionPlacement`` and the placement functions.  The device holds N S doubles instead of
    N^2."""

    S_MAX = 4096

    def __init__(self, F, noise=0.0):
        on_device = isinstance(F, torch.Tensor) and F.device.type == "cuda"
        self._F = F if on_device else np.asarray(
            F.detach().cpu().numpy() if isinstance(F, torch.Tensor) else F, dtype=np.float64)
        shape = tuple(self._F.shape)
        if len(shape) != 2 or shape[0] < 1:
            raise ValueError(f"F must be [N, S] with N >= 1, got {shape}")
        self.N, self.S = int(shape[0]), int(shape[1])
        if not 1 <= self.S <= self.S_MAX:
            raise ValueError(f"F must have 1 <= S <= {self.S_MAX} columns, got {self.S}")
        self._noise = self._noise_vector(noise, self.N)
        self._uploaded = False

    @staticmethod
    def _noise_vector(noise, N):
        """-> host float64 [N], or None when it is zero everywhere."""
        noise = _noise(noise, N)
        return noise if noise.any() else None

    def _upload(self):
        # on first use, so that the arguments are validated without a device
        if not self._uploaded:
            self._F = _device_matrix(self._F)
            self._noise = None if self._noise is None else linalg.as_device(self._noise)
            self._uploaded = True

    @property
    def F(self):
        """The factor on the device, [N, S] float64 with unit column stride."""
        self._upload()
        return self._F

    @property
    def noise(self):
        """The noise on the device, [N] float64, or None when it is zero everywhere."""
        self._upload()
        return self._noise

    def noise_is_positive(self):
        """Whether the noise is positive at every location (D = diag(noise) invertible).  Before
        the first use of F or noise this looks at host data only."""
        if self._noise is None:
            return False
        return bool((self._noise > 0.0).all())

    @classmethod
    def from_samples(cls, samples, noise=0.0, tr_stdev=1.0):
        """The empirical covariance of ``samples`` [N locations, S samples] (+ diag(noise)):
        F = (samples - their mean per location) / (tr_stdev sqrt(S)), so that F F^T equals
        ``covariance.empirical_cov(samples, tr_stdev=tr_stdev)`` (biased, centred on the sample
        mean).  The samples are copied, then centred in place."""
        from .covariance import center_rows_
        shape = tuple(np.shape(samples))
        if len(shape) != 2 or shape[0] < 1 or not 1 <= shape[1] <= cls.S_MAX:
            raise ValueError(f"samples must be [N, S] with N >= 1 and 1 <= S <= {cls.S_MAX}, got "
                             f"{shape}")
        if not (np.ndim(tr_stdev) == 0 and np.isfinite(float(tr_stdev)) and float(tr_stdev) > 0.0):
            raise ValueError(f"tr_stdev must be a finite, positive scalar, got {tr_stdev!r}")
        cls._noise_vector(noise, shape[0])
        T = linalg.as_device(samples).clone()
        center_rows_(T, 1.0 / (float(tr_stdev) * float(np.sqrt(shape[1]))))
        return cls(T, noise)

    def args(self):
        """(F, N, S, ldf, noise) as the vgposp_critf_* entries take them."""
        return _p(self.F), self.N, self.S, self.F.stride(0), _p(self.noise)


class CrossKernel:
    """A cross-covariance that is never stored: R = diag(target_scale) K(target_points, points)
    diag(site_scale) for one stationary kernel ``kind`` (``amp``, ``ls`` scalars) under a per-point
    amplitude field.  ``points`` [N, d] are the locations of ``cov_vv``, ``target_points`` [P, d]
    the targets, d <= 8; the scales (default ones) are finite and positive.  Everything is held
    on the device: (P + N) (d + 1) doubles instead of P N."""

    def __init__(self, kind, points, target_points, amp, ls, site_scale=None, target_scale=None,
                 *, _site=None):
        # the site side: validated here, or a SiteKernel's own device tensors (from_site)
        (self.kind, self.X, self.N, self.d, self.amp_value, self.ls_value, self.amp, self.ls,
         self.site_scale) = (_field(kind, points, amp, ls, "site_scale", site_scale)
                             if _site is None else _site.field())
        self.Xt = _points("target_points", target_points)
        self.P = int(self.Xt.shape[0])
        if self.Xt.shape[1] != self.d:
            raise ValueError(f"target_points must be [P, {self.d}], got {tuple(self.Xt.shape)}")
        self.target_scale = _scale("target_scale", target_scale, self.P)

    @classmethod
    def from_site(cls, site, target_points, target_scale=None):
        """The cross-covariance between ``target_points`` and the sites of a ``SiteKernel``: its
        kind, amp, ls, points and scale (the sensor noise is no part of it)."""
        if not isinstance(site, SiteKernel):
            raise ValueError("from_site needs a placement_criteria.SiteKernel")
        return cls(None, None, target_points, None, None, target_scale=target_scale, _site=site)

    def agrees_with(self, site):
        """Whether this cross-covariance and the ``SiteKernel`` describe one field: the same kind,
        amp, ls, points and site scale."""
        def same(a, b):
            return (a is None and b is None) or (a is not None and b is not None
                                                 and a.shape == b.shape and bool(torch.equal(a, b)))
        return (self.kind == site.kind and self.amp_value == site.amp_value
                and self.ls_value == site.ls_value and same(self.X, site.X)
                and same(self.site_scale, site.scale))

    def args(self):
        """(kind, Xt, P, X, d, amp, ls, target_scale, site_scale) as the vgposp_critk_* entries
        take them."""
        return (self.kind, _p(self.Xt), self.P, _p(self.X), self.d, _p(self.amp), _p(self.ls),
                _p(self.target_scale), _p(self.site_scale))


def check_cross_arguments(criterion, targets, cross_cov, target_weights, cross_kernel=None):
    """The combinations ``cross_cov`` / ``cross_kernel`` / ``target_weights`` do not allow
    (ValueError)."""
    if cross_kernel is not None:
        if cross_cov is not None:
            raise ValueError("cross_kernel and cross_cov exclude each other: the one generates "
                             "what the other stores")
        if not isinstance(cross_kernel, CrossKernel):
            raise ValueError("cross_kernel must be a placement_criteria.CrossKernel")
    elif cross_cov is None:
        if target_weights is not None:
            raise ValueError("target_weights need cross_cov: targets inside V are not weighted")
        return
    name, rows = (("cross_cov", "the rows of cross_cov") if cross_kernel is None
                  else ("cross_kernel", "target_points"))
    if criterion != "variance":
        raise ValueError(f"{name} and target_weights apply to criterion='variance' only")
    if targets is not None:
        raise ValueError(f"{name} and targets exclude each other: {rows} are the targets")


def normalize_weights(P, target_weights):
    """-> device float64 [P], or None (all ones).  Weights are finite and not negative."""
    if target_weights is None:
        return None
    return linalg.as_device(_nonnegative("target_weights", target_weights, P))


def _device_matrix(M):
    """A device float64 matrix with unit column stride (a view with a row pitch included) is used
    where it lies; anything else is copied to the device."""
    if (isinstance(M, torch.Tensor) and M.device.type == "cuda" and M.dim() == 2
            and M.dtype == torch.float64 and M.stride(1) == 1 and M.stride(0) >= M.shape[1]):
        return M
    return linalg.as_device(M)


class _Stored:
    """A Sigma or an R held as a matrix, where a generated source would stand: ``args()`` is
    (pointer, rows, pitch) and what the entry takes after them (the diagonal of a Sigma)."""

    def __init__(self, M, *tail):
        self.M, self.tail = M, tail

    def args(self):
        return (_p(self.M), int(self.M.shape[0]), self.M.stride(0), *self.tail)


# (where Sigma comes from, where the targets outside V come from) -> the family of its entries
_FAMILIES = {(_Stored, type(None)): "crit", (_Stored, _Stored): "critx",
             (_Stored, CrossKernel): "critk", (SiteKernel, type(None)): "critg",
             (SiteKernel, CrossKernel): "critgk", (FactoredCovariance, type(None)): "critf"}


class CriterionPlacement:
    """Device-resident greedy placement by ``criterion`` on an [N, N] covariance held in HBM.

    ``Sigma`` (float64, unit column stride, row stride >= N) is only read, never copied, and only
    its entries j >= i: a buffer that ``GreedyPlacement.init()`` factored in place serves as well
    when ``diag`` is the diagonal of Sigma saved before.  ``placed`` runs as forced rounds in
    ``init()``; ``kmax``, ``rounds`` and ``result()`` count the new picks only.

    ``cross_cov`` [P, N] (variance rule only, instead of ``targets``) judges the placement at P
    targets outside V, weighted by ``target_weights`` [P] >= 0; like ``Sigma`` it is used where it
    lies when it is a device float64 tensor with unit column stride, and only read.

    ``cross_kernel`` (a ``CrossKernel``, instead of ``cross_cov``) runs the same rounds on a
    cross-covariance generated from the points in every pass and never stored.

    ``Sigma`` may be a ``SiteKernel`` instead of a matrix: the same rounds on a covariance
    generated from the points.  ``diag`` and ``cross_cov`` do not combine with it, and a
    ``cross_kernel`` must describe the same field (``CrossKernel.from_site``).

    ``Sigma`` may be a ``FactoredCovariance``: the same rounds on Sigma = F F^T + diag(noise).
    ``diag``, ``cross_cov`` and ``cross_kernel`` do not combine with it.
    """

    def __init__(self, Sigma, kmax, criterion="variance", candidates=None, placed=None,
                 targets=None, threshold=1e-8, diag=None, cross_cov=None, target_weights=None,
                 cross_kernel=None):
        self.criterion = criterion
        self.crit = _criterion_id(criterion)
        self.site = Sigma if isinstance(Sigma, SiteKernel) else None
        self.fac = Sigma if isinstance(Sigma, FactoredCovariance) else None
        if self.fac is not None:
            for name, arg in (("diag", diag), ("cross_cov", cross_cov),
                              ("cross_kernel", cross_kernel)):
                if arg is not None:
                    raise ValueError(f"{name} and a FactoredCovariance exclude each other: the "
                                     "factor is the whole covariance, and targets outside V "
                                     "from samples are not supported")
            S = None
            self.N = self.n = self.fac.N
            dev = self.fac.F.device
        elif self.site is not None:
            if diag is not None:
                raise ValueError("diag and a SiteKernel exclude each other: the SiteKernel holds "
                                 "the diagonal")
            if cross_cov is not None:
                raise ValueError("cross_cov and a SiteKernel exclude each other: use "
                                 "CrossKernel.from_site")
            S = None
            self.N = self.n = self.site.N
            dev = self.site.X.device
        else:
            S = _device_matrix(Sigma)
            if S.dim() != 2 or S.shape[0] != S.shape[1]:
                raise ValueError("cov_vv must be a square matrix")
            self.N = self.n = int(S.shape[0])
            dev = S.device
        self.S = S
        if not (1 <= kmax <= self.N):
            raise ValueError(f"k must be in [1, {self.N}], got {kmax}")
        self.allowed, self.placed = normalize_constraints(self.N, kmax, candidates, placed)
        self.targets = normalize_targets(self.N, targets)
        if self.targets is not None and self.crit != CRITERIA["variance"]:
            raise ValueError("targets apply to criterion='variance' only")
        check_cross_arguments(criterion, targets, cross_cov, target_weights, cross_kernel)
        self.R = self.omega = None
        self.gen = cross_kernel
        self.P = 0
        if self.gen is not None:
            if self.gen.N != self.N:
                raise ValueError(f"cross_kernel has {self.gen.N} points, cov_vv {self.N} locations")
            if self.site is not None and not self.gen.agrees_with(self.site):
                raise ValueError("cross_kernel and the SiteKernel must agree in kind, amp, ls, "
                                 "points and site scale (CrossKernel.from_site builds one that "
                                 "does)")
            self.P = self.gen.P
            self.omega = normalize_weights(self.P, target_weights)
        if cross_cov is not None:
            self.R = _device_matrix(cross_cov)
            if self.R.dim() != 2 or self.R.shape[1] != self.N or self.R.shape[0] < 1:
                raise ValueError(f"cross_cov must be [P, {self.N}] with P >= 1, got "
                                 f"{tuple(self.R.shape)}")
            self.P = int(self.R.shape[0])
            self.omega = normalize_weights(self.P, target_weights)
        if not threshold >= 0.0:
            raise ValueError(f"threshold must not be negative, got {threshold}")
        self.threshold = float(threshold)
        self.m = len(self.placed)
        self.k = int(kmax)
        self.kmax = self.k + self.m
        self.diag = None
        if diag is not None:
            self.diag = linalg.as_device(diag).reshape(-1)
            if self.diag.numel() != self.N:
                raise ValueError(f"diag must have length {self.N}, got {self.diag.numel()}")

        def mask(b):
            return None if b is None else torch.as_tensor(b.astype(np.uint8), device=dev)
        self._allowed_dev, self._targets_dev = mask(self.allowed), mask(self.targets)
        self._placed_dev = (torch.as_tensor(self.placed, dtype=torch.int64, device=dev)
                            if self.m else None)
        # The entry family, resolved once from where Sigma and the targets come from: its name, the
        # leading arguments of every call and the sizes its workspace is laid out by.  With both
        # sides generated (n, diag) stand for Sigma: the CrossKernel carries the rest.
        sigma = self.site or self.fac or _Stored(S, _p(self.diag))
        cross = self.gen if self.R is None else _Stored(self.R)
        self._family = "vgposp_" + _FAMILIES[type(sigma), type(cross)]
        self._cross = cross is not None
        self._lead = ((self.n, _p(self.site.diag)) if self.site is not None and self._cross
                      else sigma.args()) + (cross.args() if self._cross else ())
        self._sizes = ((self.n,) + ((self.fac.S,) if self.fac is not None else ())
                       + ((self.P,) if self._cross else ()) + (self.kmax,))
        self.ws = linalg.workspace(query(self._family + "_workspace_bytes", *self._sizes))
        self.selected = torch.full((self.kmax,), -1, dtype=torch.int64, device=dev)
        self.sel_delta = torch.zeros(self.kmax, dtype=torch.float64, device=dev)
        self.rounds = 0

    def _step(self, r, forced=None, j=0):
        call(self._family + "_step", *self._lead, self.kmax, r, _p(forced), j, _p(self.selected),
             _p(self.sel_delta), _p(self.ws), self.ws.numel(), _stream())

    def init(self):
        # targets in V: the rule and its mask; targets outside V: their weights, the variance rule
        rule = ((_p(self.omega), self.kmax, self.threshold) if self._cross
                else (self.kmax, self.crit, self.threshold, _p(self._targets_dev)))
        call(self._family + "_init", *self._lead, *rule, _p(self._allowed_dev), _p(self.ws),
             self.ws.numel(), _stream())
        for j in range(self.m):
            self._step(j, self._placed_dev, j)
        self.rounds = 0
        return self

    def step(self):
        if self.rounds >= self.k:
            raise RuntimeError("all k sensors already placed")
        self._step(self.m + self.rounds)
        self.rounds += 1

    def run(self, k=None):
        k = self.k if k is None else k
        self.init()
        for _ in range(k):
            self.step()
        return self

    def state(self):
        """Device views into the workspace: ``nom`` [N] (C_yy), ``s`` [N] (sum_T C_vy^2, or
        sum_v omega_v D_vy^2), ``delta`` [N] (as scored by the last round, before its pick),
        ``W`` [placed + rounds, N] and, with ``cross_cov`` or ``cross_kernel``, ``U``
        [placed + rounds, P]."""
        ptr = [ctypes.c_void_p() for _ in range(5 if self._cross else 4)]
        call(self._family + "_buffers", _p(self.ws), *self._sizes, *map(ctypes.byref, ptr))

        def view(p, count):
            off = p.value - self.ws.data_ptr()
            return self.ws[off:off + 8 * count].view(torch.float64)
        rows = self.m + self.rounds
        st = {"nom": view(ptr[0], self.N), "s": view(ptr[1], self.N),
              "delta": view(ptr[2], self.N), "W": view(ptr[3], rows * self.N).view(rows, self.N)}
        if self._cross:
            st["U"] = view(ptr[4], rows * self.P).view(rows, self.P)
        return st

    def variance_removed(self):
        """[P] device tensor: sum_r U_r[v]^2, what the sensors so far (``placed`` included) took
        off the prior variance of target v.  Needs ``cross_cov`` or ``cross_kernel``."""
        if self.R is None and self.gen is None:
            raise ValueError("variance_removed() needs cross_cov")
        U = self.state()["U"]
        return (U * U).sum(dim=0)

    def result(self):
        """``(picks, deltas)``: the new picks (host list of np.int64; ``placed`` is not part of
        them) and the delta each had when it was picked."""
        new = slice(self.m, self.m + self.rounds)
        sel = self.selected[new].cpu().numpy()
        if (sel < 0).any():
            raise RuntimeError("greedy placement found no candidate (all deltas NaN?)")
        return [np.int64(s) for s in sel], self.sel_delta[new].cpu().numpy()


def require_positive_noise(fac):
    """ValueError unless the noise of the ``FactoredCovariance`` (or a host noise vector; None:
    zero everywhere) is positive at every location: Woodbury needs an invertible D."""
    ok = (fac.noise_is_positive() if isinstance(fac, FactoredCovariance)
          else fac is not None and bool((np.asarray(fac) > 0.0).all()))
    if not ok:
        raise ValueError("the noise must be positive at every location: the mutual-information "
                         "placement factors Sigma, and on a factor that is Woodbury's identity, "
                         "for which D = diag(noise) must be invertible; with noise = 0 anywhere "
                         "use cov='dense'")


class FactoredMIPlacement:
    """Device-resident greedy mutual-information placement on a ``FactoredCovariance``
    Sigma = F F^T + diag(noise) whose noise is positive at every location (``vgposp_fmi_*``,
    csrc/criteria.hip): the reference's criterion (placement_algorithm2.py:371-413) on the
    reference's covariance (main.py:190-199) without Sigma or its inverse, O(N S) per round.

    Selection is the full greedy (``placement_algorithm_1``, ``GreedyPlacement.step(lazy=False)``):
    the arg-max over the fresh delta of every free candidate, ties to the lowest index.  The dense
    path's default is the lazy policy, whose cache exists to save evaluations; here every delta is
    fresh after the one stream over F a round needs anyway, so the cache is not emulated and there
    are no ``evals``.  ``candidates`` / ``placed`` as in ``GreedyPlacement``: blocked locations
    stay in every denominator, ``placed`` runs as forced rounds in ``init()``; ``kmax``,
    ``rounds`` and ``result()`` count the new picks only.  Jitter is 0."""

    def __init__(self, fac, kmax, candidates=None, placed=None, threshold=1e-8):
        if not isinstance(fac, FactoredCovariance):
            raise ValueError("FactoredMIPlacement needs a placement_criteria.FactoredCovariance")
        self.fac = fac
        self.N = self.n = fac.N
        require_positive_noise(fac)                 # before any device work
        if not (1 <= kmax <= self.N):
            raise ValueError(f"k must be in [1, {self.N}], got {kmax}")
        self.allowed, self.placed = normalize_constraints(self.N, kmax, candidates, placed)
        if not threshold >= 0.0:
            raise ValueError(f"threshold must not be negative, got {threshold}")
        self.threshold = float(threshold)
        self.m = len(self.placed)
        self.k = int(kmax)
        self.kmax = self.k + self.m
        dev = fac.F.device
        self._allowed_dev = (None if self.allowed is None
                             else torch.as_tensor(self.allowed.astype(np.uint8), device=dev))
        self._placed_dev = (torch.as_tensor(self.placed, dtype=torch.int64, device=dev)
                            if self.m else None)
        self._sizes = (self.n, fac.S, self.kmax)
        self.ws = linalg.workspace(query("vgposp_fmi_workspace_bytes", *self._sizes))
        self.info = torch.zeros(1, dtype=torch.int32, device=dev)
        self.selected = torch.full((self.kmax,), -1, dtype=torch.int64, device=dev)
        self.sel_delta = torch.zeros(self.kmax, dtype=torch.float64, device=dev)
        self.rounds = 0

    def _step(self, r, forced=None, j=0):
        call("vgposp_fmi_step", *self.fac.args(), self.kmax, r, _p(forced), j, _p(self.selected),
             _p(self.sel_delta), _p(self.ws), self.ws.numel(), _stream())

    def init(self):
        call("vgposp_fmi_init", *self.fac.args(), self.kmax, self.threshold,
             _p(self._allowed_dev), _p(self.info), _p(self.ws), self.ws.numel(), _stream())
        for j in range(self.m):
            self._step(j, self._placed_dev, j)
        self.rounds = 0
        return self

    def check(self):
        """Synchronise on the status of the S x S factorization; raise CholeskyError if C was not
        positive definite (it is whenever the noise is positive and F is finite)."""
        linalg.check_info(self.info)

    def step(self):
        if self.rounds >= self.k:
            raise RuntimeError("all k sensors already placed")
        self._step(self.m + self.rounds)
        self.rounds += 1

    def run(self, k=None):
        k = self.k if k is None else k
        self.init()
        for _ in range(k):
            self.step()
        return self

    def state(self):
        """Device views into the workspace: ``nom`` [N] and ``prec`` [N] (conditioned on every
        pick so far), ``delta`` [N] (as scored by the last round, before its pick), ``W`` and
        ``V`` [placed + rounds, N]."""
        ptr = [ctypes.c_void_p() for _ in range(5)]
        call("vgposp_fmi_buffers", _p(self.ws), *self._sizes, *map(ctypes.byref, ptr))

        def view(p, count):
            off = p.value - self.ws.data_ptr()
            return self.ws[off:off + 8 * count].view(torch.float64)
        rows = self.m + self.rounds
        st = {name: view(p, self.N) for name, p in zip(("nom", "prec", "delta"), ptr)}
        st["W"] = view(ptr[3], rows * self.N).view(rows, self.N)
        st["V"] = view(ptr[4], rows * self.N).view(rows, self.N)
        return st

    def result(self):
        """``(picks, deltas)``: the new picks (host list of np.int64; ``placed`` is not part of
        them) and the delta each had when it was picked.  Raises CholeskyError from ``info``."""
        self.check()
        new = slice(self.m, self.m + self.rounds)
        sel = self.selected[new].cpu().numpy()
        if (sel < 0).any():
            raise RuntimeError("greedy placement found no candidate (all deltas NaN?)")
        return [np.int64(s) for s in sel], self.sel_delta[new].cpu().numpy()


def placement_mutual_information(fac, k, candidates=None, placed=None):
    """k sensors by greedy mutual information on a ``FactoredCovariance`` whose noise is positive
    everywhere (``FactoredMIPlacement``: the full greedy on fresh deltas, where the dense
    ``placement_algorithm_2`` is lazy).  Returns a list of ``np.int64``."""
    if not isinstance(fac, FactoredCovariance):
        raise ValueError("placement_mutual_information needs a placement_criteria."
                         "FactoredCovariance")
    if k < 1:
        require_positive_noise(fac)
        normalize_constraints(fac.N, max(int(k), 0), candidates, placed)
        return []
    return FactoredMIPlacement(fac, k, candidates=candidates, placed=placed).run(k).result()[0]


def _place(cov_vv, k, criterion, candidates, placed, targets, cross_cov=None,
           target_weights=None, cross_kernel=None):
    if k < 1:
        N = (cov_vv.N if isinstance(cov_vv, (SiteKernel, FactoredCovariance))
             else int(np.shape(cov_vv)[0]))
        if isinstance(cov_vv, FactoredCovariance) and (cross_cov is not None
                                                       or cross_kernel is not None):
            raise ValueError("cross_cov / cross_kernel and a FactoredCovariance exclude each "
                             "other: targets outside V from samples are not supported")
        normalize_constraints(N, max(int(k), 0), candidates, placed)
        normalize_targets(N, targets)
        check_cross_arguments(criterion, targets, cross_cov, target_weights, cross_kernel)
        return []
    g = CriterionPlacement(cov_vv, k, criterion, candidates=candidates, placed=placed,
                           targets=targets, cross_cov=cross_cov, target_weights=target_weights,
                           cross_kernel=cross_kernel)
    return g.run(k).result()[0]


def placement_variance_reduction(cov_vv, k, candidates=None, placed=None, targets=None,
                                 cross_cov=None, target_weights=None, cross_kernel=None):
    """k sensors by greedy variance reduction: each pick minimises the total posterior variance of
    ``targets`` (default: every location).  Returns a list of ``np.int64`` like
    ``placement_algorithm_2``; ``candidates`` / ``placed`` as there.  A singular PSD ``cov_vv``
    needs no retry: nothing is factored.

    ``cross_cov`` [P, N] instead of ``targets``: the posterior variance counts at P targets outside
    V whose covariance with the N locations it holds, weighted by ``target_weights`` [P] >= 0.
    ``cross_kernel`` (a ``CrossKernel``) instead of ``cross_cov``: the same rule with that
    covariance generated from the points in every round and never stored."""
    return _place(cov_vv, k, "variance", candidates, placed, targets, cross_cov, target_weights,
                  cross_kernel)


def placement_entropy(cov_vv, k, candidates=None, placed=None):
    """k sensors by the entropy rule: each pick has the largest conditional variance given the
    sensors so far (the pivots of a diagonal-pivoted Cholesky of ``cov_vv``)."""
    return _place(cov_vv, k, "entropy", candidates, placed, None)


class FieldReconstruction:
    """What the sensors say about the whole field, on a ``FactoredCovariance``
    Sigma = F F^T + diag(noise) (``vgposp_fpost_*``, csrc/criteria.hip): the posterior mean at all
    N sites from the readings at ``sensors`` and the variance that is left, without Sigma, Sigma_VA
    or any N x k array.  ``obs_noise`` >= 0 is a scalar measurement-error variance added to the
    sensors' own covariance only.  With A = ``sensors`` and G = Sigma_AA + obs_noise I:

        var_i  = Sigma_ii - Sigma_iA G^-1 Sigma_Ai
        mean_i = mu_i + Sigma_iA G^-1 (y - mu_A)

    One k x k factorization in ``__init__``, then one stream over F per 64 columns of work
    (k variance columns, one mean column per reading).  Everything is validated on the host before
    any device work: distinct in-range sensors, 1 <= k <= 1,024, ``obs_noise`` finite and >= 0, and,
    where both noises are zero, k <= S (G = F_A F_A^T is singular beyond that).  ``info`` is the
    device status of the factorization; nothing synchronises the host until ``check()``."""

    K_MAX = 1024
    B_MAX = 1024

    def __init__(self, fac, sensors, obs_noise=0.0, max_readings=64):
        if not isinstance(fac, FactoredCovariance):
            raise ValueError("FieldReconstruction needs a placement_criteria.FactoredCovariance")
        self.fac = fac
        self.N = self.n = fac.N
        self.sensors = _index_array("sensors", sensors, self.N)
        self.k = int(self.sensors.size)
        if not 1 <= self.k <= self.K_MAX:
            raise ValueError(f"the number of sensors must be in [1, {self.K_MAX}], got {self.k}")
        if not (np.ndim(obs_noise) == 0 and np.isfinite(float(obs_noise))
                and float(obs_noise) >= 0.0):
            raise ValueError(f"obs_noise must be a finite scalar >= 0, got {obs_noise!r}")
        self.obs_noise = float(obs_noise)
        if fac._noise is None and self.obs_noise == 0.0 and self.k > fac.S:
            raise ValueError(f"{self.k} sensors on a factor of {fac.S} columns with zero noise "
                             "and obs_noise = 0: the sensors' covariance F_A F_A^T is singular; "
                             "give a noise or an obs_noise > 0")
        if not (isinstance(max_readings, (int, np.integer)) and 1 <= max_readings <= self.B_MAX):
            raise ValueError(f"max_readings must be an integer in [1, {self.B_MAX}], got "
                             f"{max_readings!r}")
        self.max_readings = int(max_readings)
        self._ready = False

    def _init(self):
        # on first use, so that the arguments are validated without a device
        if self._ready:
            return
        dev = self.fac.F.device
        self._sensors_dev = torch.as_tensor(self.sensors, dtype=torch.int64, device=dev)
        self.ws = linalg.workspace(query("vgposp_fpost_workspace_bytes", self.n, self.fac.S,
                                         self.k, self.max_readings))
        self._info = torch.zeros(1, dtype=torch.int32, device=dev)
        call("vgposp_fpost_init", *self.fac.args(), _p(self._sensors_dev), self.k, self.obs_noise,
             _p(self._info), _p(self.ws), self.ws.numel(), _stream())
        self._ready = True

    @property
    def info(self):
        """The device status of the k x k factorization ([1] int32; 0: positive definite)."""
        self._init()
        return self._info

    def check(self):
        """Synchronise on the status of the factorization; raise CholeskyError if the sensors'
        covariance was not positive definite (then no output was written)."""
        linalg.check_info(self.info)

    def _apply(self, var, Y, mu, out):
        nrhs = 0 if Y is None else int(Y.shape[1])
        call("vgposp_fpost_apply", *self.fac.args(), self.k, _p(var), _p(Y),
             0 if Y is None else Y.stride(0), nrhs, _p(mu), _p(out),
             0 if out is None else out.stride(0), _p(self.ws), self.ws.numel(), _stream())

    def variance(self, out=None):
        """[N] device tensor: the posterior variance of every site as computed (a sensor's own is
        0 up to rounding when both noises are zero there; tiny negatives are not clamped)."""
        self._init()
        var = (torch.empty(self.N, dtype=torch.float64, device=self.fac.F.device)
               if out is None else out)
        self._apply(var, None, None, None)
        return var

    def stddev(self):
        """[N] device tensor: the square root of the variance clamped at 0."""
        return self.variance().clamp_(min=0.0).sqrt_()

    def _mean(self, readings, mean, out, var):
        """``mean()``; ``var`` [N] (or None) is filled in the first slice's pass over F."""
        Y = readings.detach() if isinstance(readings, torch.Tensor) else np.asarray(readings)
        shape = tuple(Y.shape)
        if len(shape) not in (1, 2) or shape[0] != self.k:
            raise ValueError(f"readings must be [{self.k}] or [{self.k}, B], got {shape}")
        if mean is not None and tuple(np.shape(mean)) != (self.N,):
            raise ValueError(f"mean must have length {self.N}, got shape "
                             f"{tuple(np.shape(mean))}")
        self._init()
        mu = None if mean is None else linalg.as_device(mean).reshape(-1).contiguous()
        Y = linalg.as_device(Y).reshape(self.k, -1).contiguous()
        B = int(Y.shape[1])
        res = (torch.empty((self.N, B), dtype=torch.float64, device=Y.device)
               if out is None else out)
        if var is not None and B == 0:
            self._apply(var, None, None, None)
        for b0 in range(0, B, self.max_readings):
            b1 = min(B, b0 + self.max_readings)
            self._apply(var if b0 == 0 else None, Y[:, b0:b1], mu, res[:, b0:b1])
        return res.reshape(self.N) if len(shape) == 1 else res

    def mean(self, readings, mean=None, out=None):
        """The posterior mean of the field given ``readings`` at the sensors, in their order: [k]
        -> [N], or [k, B] (B sets of readings) -> [N, B].  ``mean`` [N] is the prior mean (default
        zeros).  Works in slices of ``max_readings`` columns."""
        return self._mean(readings, mean, out, None)

    def mean_and_variance(self, readings, mean=None):
        """``(mean(readings, mean), variance())`` with the variance taken in the first slice's
        pass over F: the two share every 64-column panel that has room for both."""
        var = torch.empty(self.N, dtype=torch.float64, device=linalg.device())
        return self._mean(readings, mean, None, var), var


def reconstruct_from_samples(samples, sensors, readings, noise=0.0, obs_noise=0.0, tr_stdev=1.0):
    """``(mean, variance)`` of the field given ``readings`` at ``sensors``, under the empirical
    covariance of ``samples`` [N locations, S samples] plus diag(``noise``) (the reference's
    placement covariance, main.py:190-199) with the samples' mean per location as the prior mean.
    ``readings`` [k] or [k, B]; ``mean`` is [N] or [N, B], ``variance`` [N]."""
    shape = tuple(np.shape(samples))
    if len(shape) != 2 or shape[0] < 1:
        raise ValueError(f"samples must be [N, S] with N >= 1, got {shape}")
    _index_array("sensors", sensors, shape[0])
    T = linalg.as_device(samples)
    mu = T.mean(1)                      # before from_samples centres its copy
    fac = FactoredCovariance.from_samples(T, noise=noise, tr_stdev=tr_stdev)
    rec = FieldReconstruction(fac, sensors, obs_noise=obs_noise)
    mean, var = rec.mean_and_variance(readings, mean=mu)
    rec.check()
    return mean, var
