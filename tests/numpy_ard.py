"""References for FeatureScaled (per-feature length scale) kernels, built from the unchanged
``oracle/gp.py`` applied to pre-scaled points z = x / s.

Forward values and the amp / ls gradients come from the oracle directly.  The scale gradient follows
from the chain rule through z = x / s, dz_k/ds_k = -z_k / s_k, applied to BOTH arguments:

    d/ds_k sum_ij Kbar_ij K(z1_i, z2_j) = -(sum_i X1bar_z[i, k] z1[i, k]
                                            + sum_j X2bar_z[j, k] z2[j, k]) / s_k

where X1bar_z is the oracle's ``kernel_vjp`` and X2bar_z the same on the transposed problem
(K(z2, z1) with Kbar^T).  The adjoint with respect to the unscaled X1 is X1bar_z / s.
"""
import numpy as np

from oracle import gp as ogp


def _pts(X):
    X = np.asarray(X, dtype=np.float64)
    return X[:, None] if X.ndim == 1 else X


def kernel_vjp_scaled(kind, X1, X2, amp, ls, scale, Kbar):
    """(grad [2 + d] = d/d(amp, ls, scale), X1bar [n1, d] w.r.t. the unscaled X1) of
    sum(Kbar * K(X1 / scale, X2 / scale))."""
    scale = np.asarray(scale, dtype=np.float64)
    Z1, Z2 = _pts(X1) / scale, _pts(X2) / scale
    ga, gl, X1bar_z = ogp.kernel_vjp(kind, Z1, Z2, amp, ls, Kbar)
    _, _, X2bar_z = ogp.kernel_vjp(kind, Z2, Z1, amp, ls, np.ascontiguousarray(Kbar.T))
    gs = -(np.sum(X1bar_z * Z1, axis=0) + np.sum(X2bar_z * Z2, axis=0)) / scale
    return np.concatenate([[ga, gl], gs]), X1bar_z / scale


def lml_and_grads_scaled(kind, X, y, amp, ls, noise, scale, jitter=1e-6):
    """(LML, grad [3 + d] = dLML/d(amp, ls, noise, scale)) of a GP with the FeatureScaled kernel:
    the scale part is half the VJP's with Kbar = alpha alpha^T - C^-1."""
    scale = np.asarray(scale, dtype=np.float64)
    Z = _pts(X) / scale
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    lml, ga, gl, gn = ogp.gp_log_prob_and_grads(kind, Z, y, amp, ls, noise, jitter)
    C = ogp.kernel_matrix(kind, Z, Z, amp, ls)[0] + (noise + jitter) * np.eye(len(Z))
    Q = np.linalg.inv(C)
    alpha = Q @ y
    g, _ = kernel_vjp_scaled(kind, X, X, amp, ls, scale, np.outer(alpha, alpha) - Q)
    return lml[0], np.concatenate([[ga[0], gl[0], gn[0]], 0.5 * g[2:]])


def vgp_loss_scaled(kind, Z, X, y, Xb, yb, amp, ls, noise, scale, kl_weight):
    """oracle.vgp_training_loss of the FeatureScaled kernel (every point set divided by scale)."""
    scale = np.asarray(scale, dtype=np.float64)
    return ogp.vgp_training_loss(kind, _pts(Z) / scale, _pts(X) / scale, y, _pts(Xb) / scale, yb,
                                 amp, ls, noise, kl_weight)


def vgp_loss_grads_scaled(kind, Z, X, y, Xb, yb, amp, ls, noise, scale, kl_weight, h=1e-6):
    """(loss, d/damp, d/dls, d/dnoise, d/dZ [M, d] in unscaled coordinates, d/dscale [d]).
    The first four and d/dZ (divided by scale) are the oracle's analytic gradient on scaled inputs;
    d/dscale is by central differences of the oracle's loss with step ``h``."""
    scale = np.asarray(scale, dtype=np.float64)
    L, ga, gl, gs, gZ = ogp.vgp_training_loss_grads(kind, _pts(Z) / scale, _pts(X) / scale, y,
                                                    _pts(Xb) / scale, yb, amp, ls, noise,
                                                    kl_weight)
    gsc = np.zeros_like(scale)
    for k in range(scale.size):
        e = np.zeros_like(scale)
        e[k] = h
        gsc[k] = (vgp_loss_scaled(kind, Z, X, y, Xb, yb, amp, ls, noise, scale + e, kl_weight)
                  - vgp_loss_scaled(kind, Z, X, y, Xb, yb, amp, ls, noise, scale - e, kl_weight)
                  ) / (2 * h)
    return L, ga, gl, gs, gZ / scale, gsc
