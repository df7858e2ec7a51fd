"""GPU: vgposp_symv_upper / vgposp_symv_upper_sq (csrc/criteria.hip) against a longdouble product.

y = A x for a symmetric row-major A of which only the entries j >= i may be read: the strictly
lower triangle and the row padding hold NaN, and so does the diagonal when ``diag`` replaces it.
Bound, from the summation bound of an n-term sum in any order with one rounding per product:
|err_i| <= 4 n eps (|A| |x|)_i.  Two launches are bit-identical (fixed-order reduction)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
SIZES = [1, 2, 63, 511, 512, 513, 1537]   # one tile, its edge, two, and four with a ragged end


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _symmetric(n, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((n, n))
    return (B + B.T) / 2


def _launch(name, buf, n, lda, diag, x):
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    ws = torch.empty(max(query("vgposp_symv_upper_workspace_bytes", n), 1), dtype=torch.uint8,
                     device="cuda")
    ws.fill_(0xFF)   # NaN bytes: a partial read before it is written shows
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    call(name, _p(buf), n, lda, _p(diag), _p(x), _p(y), _p(ws), ws.numel(), _stream())
    return y.cpu().numpy()


@pytest.mark.parametrize("pad", [0, 1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_symv_upper(n, pad):
    import torch
    lda = n + pad
    A = _symmetric(n, 100 + n)
    rng = np.random.default_rng(n + pad)
    x = rng.standard_normal(n)
    x[rng.random(n) < 0.4] = 0.0             # a target mask zeroes entries of w.t
    t = (rng.random(n) < 0.5).astype(np.float64)
    d = rng.uniform(1.0, 2.0, n)
    for use_diag in (False, True):
        host = np.full((n, lda), np.nan)
        iu = np.triu_indices(n, 0 if not use_diag else 1)
        host[:, :n][iu] = A[iu]
        Aref = A.copy()
        if use_diag:
            Aref[np.diag_indices(n)] = d
        buf = torch.as_tensor(host).cuda()
        assert buf.data_ptr() % 16 == 0
        dd = torch.as_tensor(d).cuda() if use_diag else None
        for name, vec, M in (("vgposp_symv_upper", x, Aref.astype(LD)),
                             ("vgposp_symv_upper_sq", t, Aref.astype(LD) ** 2)):
            xv = torch.as_tensor(vec).cuda()
            got = _launch(name, buf, n, lda, dd, xv)
            want = M @ vec.astype(LD)
            bound = 4 * n * EPS * (np.abs(M) @ np.abs(vec).astype(LD))
            err = np.abs(got.astype(LD) - want)
            assert np.isfinite(got).all(), (name, n, lda, use_diag)
            worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
            print(f"{name} n {n} lda {lda} diag {use_diag}: worst err / bound {worst:.3f}")
            assert (err <= bound).all(), (name, n, lda, use_diag, worst)
            again = _launch(name, buf, n, lda, dd, xv)
            assert got.tobytes() == again.tobytes(), (name, n, lda, use_diag)
        assert np.array_equal(buf.cpu().numpy(), host, equal_nan=True)   # A is only read


def test_symv_in_a_wider_buffer_at_an_offset():
    """A sub-block of a wider matrix whose base is 8 bytes off 16-byte alignment (even lda): the
    8-byte load path on an even pitch; everything around the block is NaN."""
    import torch
    n, lda, shift = 700, 704, 1
    A = _symmetric(n, 9)
    x = np.random.default_rng(3).standard_normal(n)
    host = np.full(shift + n * lda, np.nan)
    host[shift:].reshape(n, lda)[:, :n][np.triu_indices(n)] = A[np.triu_indices(n)]
    buf = torch.as_tensor(host).cuda()
    view = buf[shift:].view(n, lda)
    assert view.data_ptr() % 16 == 8
    got = _launch("vgposp_symv_upper", view, n, lda, None, torch.as_tensor(x).cuda())
    want = A.astype(LD) @ x.astype(LD)
    bound = 4 * n * EPS * (np.abs(A).astype(LD) @ np.abs(x).astype(LD))
    assert (np.abs(got.astype(LD) - want) <= bound).all()


def test_symv_is_capturable():
    """No host synchronisation: the launch records into a graph, and the replay gives the bits of
    the eager launch."""
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    n = 600
    A = torch.as_tensor(_symmetric(n, 4)).cuda()
    x = torch.as_tensor(np.random.default_rng(5).standard_normal(n)).cuda()
    ws = torch.empty(query("vgposp_symv_upper_workspace_bytes", n), dtype=torch.uint8,
                     device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    args = lambda: (_p(A), n, n, ctypes.c_void_p(0), _p(x), _p(y), _p(ws), ws.numel(), _stream())
    call("vgposp_symv_upper", *args())
    torch.cuda.synchronize()
    eager = y.cpu().numpy().copy()
    y.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("vgposp_symv_upper", *args())   # (the capture stream is the current stream here)
    g.replay()
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == eager.tobytes()
