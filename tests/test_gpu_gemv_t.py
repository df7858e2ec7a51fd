"""GPU: vgposp_gemv_t / vgposp_gemv_t_sq (csrc/criteria.hip) against a longdouble product.

y = R^T x for a P x n row-major R with row pitch ldr >= n: the row padding holds NaN and must never
be read; x holds zeros (the zero weights of a target mesh).  Bound, from the summation bound of a
P-term sum in any order with one rounding per product (the form of tests/test_gpu_symv.py):
|err_j| <= 4 P eps (|R|^T |x|)_j.  Two launches are bit-identical (fixed-order reduction)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
# P: one row tile, its edge, two, and four with a ragged end; n: one column tile, its edge (even
# and odd: the last lane's pair is whole or half), two, and three with a single last column
SHAPES = [(1, 1), (1, 513), (2, 2), (2, 1025), (63, 511), (63, 2), (511, 512), (512, 1),
          (512, 513), (513, 511), (513, 1025), (1537, 2), (1537, 512), (1537, 1025)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _launch(name, view, P, n, ldr, x):
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    ws = torch.empty(max(query("vgposp_gemv_t_workspace_bytes", P, n), 1), dtype=torch.uint8,
                     device="cuda")
    ws.fill_(0xFF)   # NaN bytes: a partial read before it is written shows
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    call(name, _p(view), P, n, ldr, _p(x), _p(y), _p(ws), ws.numel(), _stream())
    return y.cpu().numpy()


def _check(P, n, ldr, shift):
    """Both forms on an R that lies ``shift`` doubles into a NaN-filled buffer."""
    import torch
    rng = np.random.default_rng(1000 * P + n + ldr + shift)
    R = rng.standard_normal((P, n))
    x = rng.standard_normal(P)
    x[rng.random(P) < 0.3] = 0.0
    w = rng.uniform(0.5, 2.0, P)
    w[rng.random(P) < 0.3] = 0.0
    host = np.full(shift + P * ldr, np.nan)
    host[shift:].reshape(P, ldr)[:, :n] = R
    buf = torch.as_tensor(host).cuda()
    view = buf[shift:].view(P, ldr)
    assert view.data_ptr() % 16 == 8 * (shift % 2)
    for name, vec, M in (("vgposp_gemv_t", x, R.astype(LD)),
                         ("vgposp_gemv_t_sq", w, R.astype(LD) ** 2)):
        xv = torch.as_tensor(vec).cuda()
        got = _launch(name, view, P, n, ldr, xv)
        want = M.T @ vec.astype(LD)
        bound = 4 * P * EPS * (np.abs(M).T @ np.abs(vec).astype(LD))
        err = np.abs(got.astype(LD) - want)
        assert np.isfinite(got).all(), (name, P, n, ldr, shift)
        worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
        print(f"{name} P {P} n {n} ldr {ldr} shift {shift}: worst err / bound {worst:.3f}")
        assert (err <= bound).all(), (name, P, n, ldr, shift, worst)
        again = _launch(name, view, P, n, ldr, xv)
        assert got.tobytes() == again.tobytes(), (name, P, n, ldr, shift)
    assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)   # R is only read


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("P,n", SHAPES)
def test_gemv_t(P, n, pad):
    _check(P, n, n + pad, 0)


@pytest.mark.parametrize("P,n,ldr", [(513, 511, 512), (700, 1025, 1026), (63, 2, 5)])
def test_gemv_t_at_an_odd_aligned_base(P, n, ldr):
    """A base 8 bytes off 16-byte alignment (a view offset by one double), on an even and on an odd
    pitch: the 8-byte load path."""
    _check(P, n, ldr, 1)


def test_gemv_t_is_capturable():
    """No host synchronisation: the launch records into a graph, and the replay gives the bits of
    the eager launch."""
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    P, n = 700, 600
    rng = np.random.default_rng(4)
    R = torch.as_tensor(rng.standard_normal((P, n))).cuda()
    x = torch.as_tensor(rng.standard_normal(P)).cuda()
    ws = torch.empty(query("vgposp_gemv_t_workspace_bytes", P, n), dtype=torch.uint8,
                     device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    args = lambda: (_p(R), P, n, n, _p(x), _p(y), _p(ws), ws.numel(), _stream())
    call("vgposp_gemv_t", *args())
    torch.cuda.synchronize()
    eager = y.cpu().numpy().copy()
    y.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("vgposp_gemv_t", *args())   # (the capture stream is the current stream here)
    g.replay()
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == eager.tobytes()


def test_empty_dimensions_do_no_device_work():
    from vgposp_amd._lib import call
    null = ctypes.c_void_p(0)
    for name in ("vgposp_gemv_t", "vgposp_gemv_t_sq"):
        assert call(name, null, 0, 7, 7, null, null, null, 0, null) == 0
        assert call(name, null, 7, 0, 0, null, null, null, 0, null) == 0
