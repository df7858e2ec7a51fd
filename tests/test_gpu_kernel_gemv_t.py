"""GPU: vgposp_kernel_gemv_t / vgposp_kernel_gemv_t_sq (csrc/criteria.hip) against the longdouble
product of the longdouble-generated matrix (tests/numpy_kernel_cross.py).

y = R^T x for R = diag(a_t) K(Xt, X) diag(a_s), never stored.  Points uniform in [0, 1]^d, ls in
[0.3, 1], amp 1.3; x holds zeros (the zero weights of a target mesh); the first targets coincide
with the first sites (r = 0).  Bound: |err_j| <= (4 P eps + tau) (|R|^T |x|)_j with tau = 1e-13
(2e-13 for the squared form): the summation term of tests/test_gpu_gemv_t.py plus the project's
per-entry assembly tolerance (measured: at most 0.006 of the bound).  Two launches are
bit-identical (fixed-order reduction)."""
import ctypes

import numpy as np
import pytest

from tests import numpy_kernel_cross as K
from vgposp_amd._lib import KGEMV_ROWS as H

pytestmark = pytest.mark.gpu

AMP = 1.3
# P: one chunk, its edges, and four chunks with a ragged end; n: one column tile, its edge (even and
# odd: the last lane's pair is whole or half), two tiles, and three with a single last column
PAIRS = [(1, 1), (1, 513), (2, 2), (2, 1025), (63, 511), (63, 2), (H - 1, 512), (H, 1),
         (H, 513), (H + 1, 511), (H + 1, 1025), (3 * H + 1, 512)]
DIMS = [1, 3, 5, 8, 2]       # 1 .. 3 are compiled in, 4 .. 8 share the run-time form
COMBOS = [(d, kind) for d in DIMS for kind in K.KINDS]
# two (d, kind) per pair: every kind meets every d over the 24 slots
CASES = [(P, n, *COMBOS[(2 * i + j) % len(COMBOS)]) for i, (P, n) in enumerate(PAIRS)
         for j in range(2)]
CASES += [(3 * H + 1, 1025, d, kind) for d, kind in
          ((1, "matern32"), (3, "eq"), (5, "matern12"), (8, "matern52"), (8, "eq"), (5, "eq"),
           (1, "matern52"), (3, "matern12"))]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _inputs(P, n, d, seed):
    rng = np.random.default_rng(seed)
    Xt, Xs = rng.random((P, d)), rng.random((n, d))
    c = min(3, P, n)
    Xt[:c] = Xs[:c]
    x = rng.standard_normal(P)
    x[rng.random(P) < 0.3] = 0.0
    w = rng.uniform(0.5, 2.0, P)
    w[rng.random(P) < 0.3] = 0.0
    return Xt, Xs, float(rng.uniform(0.3, 1.0)), x, w, rng.uniform(0.5, 2.0, P), \
        rng.uniform(0.5, 2.0, n)


def _launch(name, kind, Xt, Xs, ls, at, a_s, x):
    """One launch on a NaN-filled workspace and output: a partial read before it is written, or a
    column that is not written, shows."""
    import torch
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.linalg import _p, _stream
    P, n = Xt.shape[0], Xs.shape[0]
    ws = torch.empty(max(query("vgposp_kernel_gemv_t_workspace_bytes", P, n), 1),
                     dtype=torch.uint8, device="cuda")
    ws.fill_(0xFF)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()
    t = [dev(a) for a in (Xt, Xs, np.array([AMP]), np.array([ls]), at, a_s, x)]
    call(name, KERNEL_KINDS[kind], _p(t[0]), P, _p(t[1]), n, Xt.shape[1], _p(t[2]), _p(t[3]),
         _p(t[4]), _p(t[5]), _p(t[6]), _p(y), _p(ws), ws.numel(), _stream())
    return y.cpu().numpy()


@pytest.mark.parametrize("P,n,d,kind", CASES)
def test_kernel_gemv_t(P, n, d, kind):
    Xt, Xs, ls, x, w, at, a_s = _inputs(P, n, d, 1000 * P + n + d)
    K0 = K.kernel_ld(kind, Xt, Xs, AMP, ls)
    for scaled in (False, True):
        sc = (at, a_s) if scaled else (None, None)
        R = at.astype(K.LD)[:, None] * K0 * a_s.astype(K.LD)[None, :] if scaled else K0
        for name, vec, sq in (("vgposp_kernel_gemv_t", x, False),
                              ("vgposp_kernel_gemv_t_sq", w, True)):
            got = _launch(name, kind, Xt, Xs, ls, *sc, vec)
            want, weight = K.gemv_t_ld(R, vec, sq)
            bound = K.gemv_t_bound(P, weight, sq)
            err = np.abs(got.astype(K.LD) - want)
            assert np.isfinite(got).all(), (name, scaled)
            worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
            print(f"{name} {kind} P {P} n {n} d {d} scaled {scaled}: worst err / bound "
                  f"{worst:.3f}")
            assert (err <= bound).all(), (name, scaled, worst)
            again = _launch(name, kind, Xt, Xs, ls, *sc, vec)
            assert got.tobytes() == again.tobytes(), (name, scaled)


@pytest.mark.parametrize("P,n,d,kind", [(3 * H + 1, 1025, 3, "matern52"), (H + 1, 511, 5, "eq")])
def test_equals_the_stored_pass_on_the_assembled_matrix(P, n, d, kind):
    """vgposp_gemv_t on the device-assembled kernel_matrix(Xt, X): within the sum of both bounds
    (the assembled entries carry the same per-entry tolerance)."""
    import torch
    from vgposp_amd import linalg
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    Xt, Xs, ls, x, w, _, _ = _inputs(P, n, d, 7 * P + n)
    Rd = linalg.kernel_matrix(kind, Xt, Xs, AMP, ls)[0]
    R = K.cross_ld(kind, Xt, Xs, AMP, ls)
    for stored, name, vec, sq in (("vgposp_gemv_t", "vgposp_kernel_gemv_t", x, False),
                                  ("vgposp_gemv_t_sq", "vgposp_kernel_gemv_t_sq", w, True)):
        ws = torch.empty(query("vgposp_gemv_t_workspace_bytes", P, n), dtype=torch.uint8,
                         device="cuda")
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        xv = torch.as_tensor(vec).cuda()
        call(stored, _p(Rd), P, n, Rd.stride(0), _p(xv), _p(y), _p(ws), ws.numel(), _stream())
        got = _launch(name, kind, Xt, Xs, ls, None, None, vec)
        bound = 2 * K.gemv_t_bound(P, K.gemv_t_ld(R, vec, sq)[1], sq)
        diff = np.abs(got.astype(K.LD) - y.cpu().numpy().astype(K.LD))
        print(f"{name} against {stored}: worst difference / bound {float(np.max(diff / bound)):.3f}")
        assert (diff <= bound).all()


def test_host_wrapper():
    from vgposp_amd.covariance import kernel_gemv_t
    Xt, Xs, ls, x, w, at, a_s = _inputs(700, 300, 3, 11)
    R = K.cross_ld("matern32", Xt, Xs, AMP, ls, at, a_s)
    for vec, sq in ((x, False), (w, True)):
        got = kernel_gemv_t("matern32", Xt, Xs, AMP, ls, vec, squared=sq, target_scale=at,
                            site_scale=a_s).cpu().numpy()
        want, weight = K.gemv_t_ld(R, vec, sq)
        assert (np.abs(got.astype(K.LD) - want) <= K.gemv_t_bound(700, weight, sq)).all()
    with pytest.raises(ValueError, match="shapes do not match"):
        kernel_gemv_t("eq", Xt, Xs, AMP, ls, x[:-1])
    with pytest.raises(ValueError, match="shapes do not match"):
        kernel_gemv_t("eq", Xt, Xs[:, :2], AMP, ls, x)


def test_kernel_gemv_t_is_capturable():
    """No host synchronisation: the launch records into a graph, and the replay gives the bits of
    the eager launch."""
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    P, n, d = 700, 600, 3
    Xt, Xs, ls, x, _, at, a_s = _inputs(P, n, d, 4)
    t = [torch.as_tensor(a).cuda() for a in (Xt, Xs, np.array([AMP]), np.array([ls]), at, a_s, x)]
    ws = torch.empty(query("vgposp_kernel_gemv_t_workspace_bytes", P, n), dtype=torch.uint8,
                     device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    args = lambda: (3, _p(t[0]), P, _p(t[1]), n, d, _p(t[2]), _p(t[3]), _p(t[4]), _p(t[5]),
                    _p(t[6]), _p(y), _p(ws), ws.numel(), _stream())
    call("vgposp_kernel_gemv_t", *args())
    torch.cuda.synchronize()
    eager = y.cpu().numpy().copy()
    y.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("vgposp_kernel_gemv_t", *args())   # (the capture stream is the current stream here)
    g.replay()
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == eager.tobytes()
    assert np.isfinite(eager).all() and np.any(eager != 0.0)


def test_empty_dimensions_do_no_device_work():
    from vgposp_amd._lib import call
    null = ctypes.c_void_p(0)
    for name in ("vgposp_kernel_gemv_t", "vgposp_kernel_gemv_t_sq"):
        assert call(name, 0, null, 0, null, 7, 3, null, null, null, null, null, null, null, 0,
                    null) == 0
        assert call(name, 0, null, 7, null, 0, 3, null, null, null, null, null, null, null, 0,
                    null) == 0
