"""C-ABI boundary and host-side rejections of the FeatureScaled (per-feature length scale) path
without a GPU: the five symbols are exported, declared and typed, the workspace queries answer, bad
arguments are reported by position before any device work, and the kernel class refuses what it
does not support.  The numpy reference the GPU tests use is pinned to central differences here."""
import ctypes

import numpy as np
import pytest

from oracle import gp as ogp
from tests import numpy_ard
from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)  # a non-NULL pointer that is never dereferenced
BIG = 1 << 40
NEW = {"vgposp_scale_points": (ctypes.c_int, 6),
       "vgposp_kernel_vjp_scaled_workspace_bytes": (ctypes.c_size_t, 3),
       "vgposp_kernel_vjp_scaled": (ctypes.c_int, 18),
       "vgposp_lml_grad_scaled_workspace_bytes": (ctypes.c_size_t, 1),
       "vgposp_lml_grad_scaled": (ctypes.c_int, 14)}


def test_symbols_exported_declared_and_typed():
    lib = _lib.load()
    for name, (res, nargs) in NEW.items():
        assert hasattr(lib, name)
        assert name in _lib.header_symbols()
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res and len(got_args) == nargs, name
    assert lib.vgposp_abi_version() == 2


def test_scale_points_arguments():
    lib = _lib.load()
    assert lib.vgposp_scale_points(None, 0, 3, None, None, None) == 0   # n = 0: no device work
    assert lib.vgposp_scale_points(P8, -1, 3, P8, P8, None) == -2
    assert lib.vgposp_scale_points(P8, 5, 0, P8, P8, None) == -3
    assert lib.vgposp_scale_points(P8, 5, 9, P8, P8, None) == -3
    assert lib.vgposp_scale_points(None, 5, 3, P8, P8, None) == -1
    assert lib.vgposp_scale_points(P8, 5, 3, None, P8, None) == -4      # NULL scale
    assert lib.vgposp_scale_points(P8, 5, 3, P8, None, None) == -5


def _vjp(kind=0, Z1=P8, n1=10, Z2=P8, n2=20, d=3, amp=P8, ls=P8, scale=P8, Kbar=P8, ldk=20,
         u=None, w=None, grad=P8, X1bar=None, ws=P8, ws_bytes=BIG):
    return _lib.load().vgposp_kernel_vjp_scaled(kind, Z1, n1, Z2, n2, d, amp, ls, scale, Kbar, ldk,
                                                u, w, grad, X1bar, ws, ws_bytes, None)


def test_kernel_vjp_scaled_arguments():
    assert _vjp(kind=4) == -1
    assert _vjp(Z1=None) == -2
    assert _vjp(n1=0) == -3
    assert _vjp(Z2=None) == -4
    assert _vjp(n2=0) == -5
    assert _vjp(d=0) == -6 and _vjp(d=9) == -6
    assert _vjp(amp=None) == -7
    assert _vjp(ls=None) == -8
    assert _vjp(scale=None) == -9
    assert "bad argument 9" in _lib.last_error()
    assert _vjp(Kbar=None) == -10
    assert _vjp(ldk=19) == -11
    assert _vjp(u=P8) == -12 and _vjp(w=P8) == -12     # both set or both NULL
    assert _vjp(grad=None) == -14
    assert _vjp(ws=None) == -16
    assert _vjp(ws_bytes=16) == _lib.E_WS
    assert "workspace 16 <" in _lib.last_error()


def _lml(kind=0, Z=P8, n=10, d=3, amp=P8, ls=P8, scale=P8, Cinv=P8, ldc=10, alpha=P8, grad=P8,
         ws=P8, ws_bytes=BIG):
    return _lib.load().vgposp_lml_grad_scaled(kind, Z, n, d, amp, ls, scale, Cinv, ldc, alpha,
                                              grad, ws, ws_bytes, None)


def test_lml_grad_scaled_arguments():
    assert _lml(kind=-1) == -1
    assert _lml(Z=None) == -2
    assert _lml(n=0) == -3
    assert _lml(d=0) == -4 and _lml(d=9) == -4
    assert _lml(amp=None) == -5
    assert _lml(ls=None) == -6
    assert _lml(scale=None) == -7
    assert _lml(Cinv=None) == -8
    assert _lml(ldc=9) == -9
    assert _lml(alpha=None) == -10
    assert _lml(grad=None) == -11
    assert _lml(ws=None) == -12
    assert _lml(ws_bytes=16) == _lib.E_WS


def test_workspace_queries():
    q = lambda n1, n2, d: _lib.query("vgposp_kernel_vjp_scaled_workspace_bytes", n1, n2, d)
    assert q(0, 10, 3) == 0 and q(10, 0, 3) == 0 and q(10, 10, 0) == 0 and q(-1, 10, 3) == 0
    # [col-blocks][n1][d] X1bar partials and [blocks][2 + d] scalars
    assert q(37, 1100, 3) >= 8 * (2 * 37 * 3 + 2 * 3 * 5)
    assert q(37, 1100, 3) > _lib.query("vgposp_kernel_vjp_workspace_bytes", 37, 1100, 3)
    assert q(38, 1100, 3) > q(37, 1100, 3)          # grows with n1
    assert q(37, 2100, 3) > q(37, 1100, 3)          # with n2 (a third column block)
    assert q(37, 1100, 4) > q(37, 1100, 3)          # and with d
    g = lambda n: _lib.query("vgposp_lml_grad_scaled_workspace_bytes", n)
    assert g(0) == 0 and g(-5) == 0
    assert g(1) >= 8 * 11 and g(17) >= 2 * 8 * 11 and g(300) > g(17) > g(1)


def test_feature_scaled_rejections():
    from vgposp_amd import psd_kernels as psd
    base = psd.MaternFiveHalves(0.9, 1.1)
    k = psd.FeatureScaled(base, np.array([0.5, 2.0, 1.0]))
    assert k.kind == "matern52" and k.batch_shape == () and k.batch_size == 1
    assert k.amplitude == 0.9 and k.length_scale == 1.1
    with pytest.raises(ValueError, match="3 entries.*2 features"):
        k.scaled(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="3 entries.*2 features"):
        k.matrix(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match="positive"):
        psd.FeatureScaled(base, [1.0, 0.0], validate_args=True)
    with pytest.raises(ValueError, match="positive"):
        psd.FeatureScaled(base, [1.0, -2.0], validate_args=True)
    with pytest.raises(NotImplementedError, match="non-batched"):
        psd.FeatureScaled(psd.ExponentiatedQuadratic(np.array([1.0, 2.0]), 1.0), [1.0])
    with pytest.raises(NotImplementedError, match="inside"):
        psd.FeatureScaled(k, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        psd.FeatureScaled(base, np.ones(9))            # d <= 8
    with pytest.raises(ValueError):
        psd.FeatureScaled(base, np.ones((2, 3)))       # batched scale_diag


@pytest.mark.parametrize("kind", ogp.KERNELS)
def test_reference_scale_gradient_is_the_finite_difference(kind):
    """The helper's scale gradient against central differences of the oracle's kernel matrix, and
    the identity sum_k s_k d/ds_k = ls d/dls (scaling every feature is scaling ls)."""
    rng = np.random.default_rng(3)
    X1, X2 = rng.uniform(-2, 2, (7, 3)), rng.uniform(-2, 2, (9, 3))
    Kb = rng.normal(size=(7, 9))
    s = np.array([0.7, 1.3, 2.1])
    f = lambda sc: np.sum(Kb * ogp.kernel_matrix(kind, X1 / sc, X2 / sc, 0.8, 0.9)[0])
    g, _ = numpy_ard.kernel_vjp_scaled(kind, X1, X2, 0.8, 0.9, s, Kb)
    h = 1e-6
    fd = [(f(s + h * e) - f(s - h * e)) / (2 * h) for e in np.eye(3)]
    np.testing.assert_allclose(g[2:], fd, rtol=1e-6, atol=1e-8 * np.abs(fd).max())
    assert np.dot(s, g[2:]) == pytest.approx(0.9 * g[1], rel=1e-12)
    y = rng.normal(size=7)
    _, gl = numpy_ard.lml_and_grads_scaled(kind, X1, y, 0.8, 0.9, 0.1, s)
    fl = lambda sc: ogp.gp_log_prob(kind, X1 / sc, y, [0.8], [0.9], 0.1)[0]
    fd = [(fl(s + h * e) - fl(s - h * e)) / (2 * h) for e in np.eye(3)]
    np.testing.assert_allclose(gl[3:], fd, rtol=1e-6, atol=1e-8 * np.abs(fd).max())
