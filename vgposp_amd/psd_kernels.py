"""PSD kernels with the ``tfp.positive_semidefinite_kernels`` surface the reference uses
(``from tensorflow_probability import positive_semidefinite_kernels as tfkern``):

* ``ExponentiatedQuadratic(amplitude, length_scale, feature_ndims=1)``
  (3D_sin_wave.py:158-159, main_tests.py:617-619, variational_Gaussian_process_example.py:55-57)
* ``MaternOneHalf`` (gp_functions.py:160-163, main.py:94)
* ``MaternThreeHalves``
* ``MaternFiveHalves`` (main_architecture_2_sampledistribution.py:211)

``amplitude`` / ``length_scale`` are floats, arrays (a shape-[B] value gives a batch of B kernels,
NOT ARD — as with the reference's shape-[2] AMPLITUDE_INIT, main_GP_fit.py:117-118), device
tensors, or trainable ``variables.Softplus`` views.  ``matrix(x1, x2)`` assembles K on the GPU
(libvgposp ``vgposp_kernel_matrix``) and returns a float64 device tensor [B, n, m]
(or [n, m] when the kernel is not batched).
"""
from __future__ import annotations

import numpy as np
import torch

from . import linalg
from .variables import batch_size, resolve


class PositiveSemidefiniteKernel:
    kind = None

    def __init__(self, amplitude=None, length_scale=None, feature_ndims=1, validate_args=False,
                 name=None):
        if feature_ndims != 1:
            raise NotImplementedError("only feature_ndims=1 (the reference's setting) is supported")
        self.amplitude = amplitude
        self.length_scale = length_scale
        self.feature_ndims = feature_ndims
        self.validate_args = validate_args
        self.name = name or type(self).__name__

    # -- parameters ---------------------------------------------------------------------------
    @property
    def batch_size(self):
        return batch_size(self.amplitude, self.length_scale)

    @property
    def batch_shape(self):
        B = self.batch_size
        shaped = any(hasattr(p, "shape") and tuple(getattr(p, "shape")) != ()
                     for p in (self.amplitude, self.length_scale) if p is not None)
        return (B,) if shaped else ()

    def params(self):
        B = self.batch_size
        amp = resolve(self.amplitude, B)
        ls = resolve(self.length_scale, B)
        if self.validate_args:
            if not bool((amp > 0).all()) or not bool((ls > 0).all()):
                raise ValueError("amplitude and length_scale must be positive")
        return amp, ls

    # -- evaluation ---------------------------------------------------------------------------
    def matrix(self, x1, x2, diag_shift=None, lower=False, keep_batch=None):
        amp, ls = self.params()
        K = linalg.kernel_matrix(self.kind, _pts(x1), _pts(x2), amp, ls, diag_shift=diag_shift,
                                 lower=lower)
        if keep_batch is None:
            keep_batch = self.batch_shape != ()
        return K if keep_batch else K[0]

    def apply(self, x1, x2):
        """k(x1_i, x2_i) for paired rows: the diagonal of matrix(x1, x2) (device tensor)."""
        K = self.matrix(x1, x2, keep_batch=True)
        out = torch.diagonal(K, dim1=-2, dim2=-1)
        return out if self.batch_shape != () else out[0]

    def __repr__(self):
        return f"{self.name}(amplitude={self.amplitude!r}, length_scale={self.length_scale!r})"


def _pts(x):
    if hasattr(x, "shape") and len(x.shape) == 1:
        return x.reshape(-1, 1) if hasattr(x, "reshape") else np.asarray(x).reshape(-1, 1)
    if hasattr(x, "shape") and len(x.shape) == 3:  # [batch=1, n, d] index points
        if x.shape[0] != 1:
            raise NotImplementedError("batched index points must have batch size 1")
        return x[0]
    return x


class ExponentiatedQuadratic(PositiveSemidefiniteKernel):
    kind = "eq"


class MaternOneHalf(PositiveSemidefiniteKernel):
    kind = "matern12"


class MaternThreeHalves(PositiveSemidefiniteKernel):
    kind = "matern32"


class MaternFiveHalves(PositiveSemidefiniteKernel):
    kind = "matern52"


MAX_FEATURES = 8  # the d <= 8 of every libvgposp assembly kernel


class FeatureScaled(PositiveSemidefiniteKernel):
    """``tfkern.FeatureScaled(kernel, scale_diag)``: per-feature (ARD) length scales,

        k(x1, x2) = kernel(x1 / scale_diag, x2 / scale_diag).

    The base kernel keeps its own amplitude and length_scale.  ``scale_diag`` [d] is an array, a
    device tensor or a trainable ``variables.Softplus``.  The points are divided once
    (``scaled``, libvgposp ``vgposp_scale_points``) and every assembly kernel of the base then
    evaluates the scaled kernel.  One (non-batched) base kernel and one scale vector only."""

    def __init__(self, kernel, scale_diag, validate_args=False, name=None):
        if isinstance(kernel, FeatureScaled):
            raise NotImplementedError("a FeatureScaled inside a FeatureScaled is not supported: "
                                      "multiply the two scale_diag vectors instead")
        if kernel.batch_shape != () or kernel.batch_size != 1:
            raise NotImplementedError("FeatureScaled needs one (non-batched) base kernel")
        shape = tuple(scale_diag.shape) if hasattr(scale_diag, "shape") else np.shape(scale_diag)
        if len(shape) != 1:
            raise ValueError(f"scale_diag must have shape [d] (batched scales are not supported), "
                             f"got {shape}")
        if not 1 <= shape[0] <= MAX_FEATURES:
            raise ValueError(f"scale_diag has {shape[0]} entries; 1 to {MAX_FEATURES} features are "
                             "supported")
        self.kernel = kernel
        self.scale_diag = scale_diag
        self.num_features = int(shape[0])
        self.feature_ndims = kernel.feature_ndims
        self.validate_args = validate_args
        self.name = name or type(self).__name__
        if validate_args and not hasattr(scale_diag, "value"):
            host = scale_diag.detach().cpu().numpy() if isinstance(scale_diag, torch.Tensor) \
                else np.asarray(scale_diag, dtype=np.float64)
            if not (host > 0).all():
                raise ValueError("scale_diag must be positive")

    # -- the base kernel's parameters -----------------------------------------------------------
    @property
    def kind(self):
        return self.kernel.kind

    @property
    def amplitude(self):
        return self.kernel.amplitude

    @property
    def length_scale(self):
        return self.kernel.length_scale

    def params(self):
        return self.kernel.params()

    def scale(self):
        """Current scale_diag as a [d] float64 device tensor."""
        s = resolve(self.scale_diag)
        if self.validate_args and not bool((s > 0).all()):
            raise ValueError("scale_diag must be positive")
        return s

    # -- evaluation -----------------------------------------------------------------------------
    def scaled(self, x):
        """x / scale_diag as a [n, d] device tensor."""
        x = _pts(x if hasattr(x, "shape") else np.asarray(x, dtype=np.float64))
        d = 1 if len(x.shape) == 1 else int(x.shape[-1])
        if d != self.num_features:
            raise ValueError(f"scale_diag has {self.num_features} entries, the index points have "
                             f"{d} features")
        return linalg.scale_points(x, self.scale())

    def matrix(self, x1, x2, diag_shift=None, lower=False, keep_batch=None):
        z1 = self.scaled(x1)
        z2 = z1 if x2 is x1 else self.scaled(x2)
        return self.kernel.matrix(z1, z2, diag_shift=diag_shift, lower=lower,
                                  keep_batch=keep_batch)

    def __repr__(self):
        return f"{self.name}({self.kernel!r}, scale_diag={self.scale_diag!r})"


def scaled_points(kernel, x):
    """The points a kernel's assembly sees: ``x / scale_diag`` for a FeatureScaled kernel, ``x``
    itself otherwise.  For call sites that assemble through ``linalg`` with ``kernel.kind``."""
    return kernel.scaled(x) if isinstance(kernel, FeatureScaled) else x
