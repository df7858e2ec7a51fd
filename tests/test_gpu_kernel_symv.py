"""GPU: vgposp_kernel_symv / vgposp_kernel_symv_sq (csrc/criteria.hip) against the longdouble
product of the longdouble-generated matrix (tests/numpy_site_kernel.py).

y = Sigma x for Sigma = diag(a) K(X, X) diag(a) off the diagonal and a vector on it, never stored.
Points uniform in [0, 1]^d, ls in [0.3, 1], amp 1.3; a third of x is zero; two pairs of sites
coincide (one pair inside a tile, one across the first and the last tile), whose entry is
a_i a_j amp^2 and not the diagonal.  Bound: |err_i| <= (4 n eps + tau) (|Sigma| |x|)_i with
tau = 1e-13 (2e-13 for the squared form), the constants of numpy_kernel_cross.gemv_t_bound.  Two
launches are bit-identical (fixed-order reduction).

The workgroup's tile block is G x G 512-tiles with G = 1 below n = 32,769, 2 from there and 8 from
n = 229,377: n = 4,097 spans nine groups in both directions at G = 1; 32,769 and 229,377 are the
smallest sizes at which the blocks hold 2 x 2 and 8 x 8 tiles (with a ragged last block).  Their
longdouble matrices do not fit, so they are checked against the full-square pass and, for a few
rows, against the longdouble row."""
import ctypes

import numpy as np
import pytest

from tests import numpy_kernel_cross as K
from tests import numpy_site_kernel as SK

pytestmark = pytest.mark.gpu

AMP = 1.3
NS = [1, 2, 63, 511, 512, 513, 1025, 1537]
DIMS = [1, 3, 5, 8]          # 1 .. 3 are compiled in, 4 .. 8 share the run-time form
COMBOS = [(d, kind) for d in DIMS for kind in K.KINDS]
# two (d, kind) per n: every kind meets d = 1, 3, 5, 8 over the 16 slots; d = 2 and the three tiles
# with a single last column for every kind follow
CASES = [(n, *COMBOS[(2 * i + j) % len(COMBOS)]) for i, n in enumerate(NS) for j in range(2)]
CASES += [(1537, d, kind) for d, kind in
          ((2, "eq"), (2, "matern12"), (2, "matern32"), (2, "matern52"), (3, "eq"), (5, "matern12"),
           (1, "matern32"), (8, "matern52"))]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


def _inputs(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    if n >= 2:
        X[n - 1] = X[0]
    if n >= 4:
        X[2] = X[1]
    x = rng.standard_normal(n)
    x[rng.random(n) < 0.33] = 0.0
    w = rng.uniform(0.5, 2.0, n)
    w[rng.random(n) < 0.33] = 0.0
    return X, float(rng.uniform(0.3, 1.0)), x, w, rng.uniform(0.5, 2.0, n), \
        rng.uniform(0.5, 3.0, n)


def _dev(a):
    import torch
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _launch(name, kind, X, ls, scale, diag, x):
    """One launch on a NaN-filled workspace and output: a partial read before it is written, or an
    output that is not written, shows."""
    import torch
    from vgposp_amd._lib import KERNEL_KINDS, call, query
    from vgposp_amd.linalg import _p, _stream
    n = X.shape[0]
    ws = torch.empty(max(query("vgposp_kernel_symv_workspace_bytes", n), 1), dtype=torch.uint8,
                     device="cuda")
    ws.fill_(0xFF)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    t = [_dev(a) for a in (X, np.array([AMP]), np.array([ls]), scale, diag, x)]
    call(name, KERNEL_KINDS[kind], _p(t[0]), n, X.shape[1], _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]),
         _p(t[5]), _p(y), _p(ws), ws.numel(), _stream())
    return y.cpu().numpy()


FORMS = (("vgposp_kernel_symv", False), ("vgposp_kernel_symv_sq", True))


@pytest.mark.parametrize("n,d,kind", CASES)
def test_kernel_symv(n, d, kind):
    X, ls, x, w, a, dg = _inputs(n, d, 1000 * n + d)
    for scale in (None, a):
        for diag in (None, dg):
            S = SK.site_cov_ld(kind, X, AMP, ls, scale, diag)
            if n >= 2:      # the coincident pair is an off-diagonal entry
                sa = np.ones(n) if scale is None else scale
                assert abs(float(S[0, n - 1]) - sa[0] * sa[n - 1] * AMP * AMP) < 1e-14 * 16
            for (name, sq), vec in zip(FORMS, (x, w)):
                got = _launch(name, kind, X, ls, scale, diag, vec)
                want, weight = SK.symv_ld(S, vec, sq)
                bound = SK.symv_bound(n, weight, sq)
                err = np.abs(got.astype(K.LD) - want)
                assert np.isfinite(got).all(), (name, scale is not None, diag is not None)
                worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
                print(f"{name} {kind} n {n} d {d} scale {scale is not None} diag "
                      f"{diag is not None}: worst err / bound {worst:.3f}")
                assert (err <= bound).all(), (name, worst)
                again = _launch(name, kind, X, ls, scale, diag, vec)
                assert got.tobytes() == again.tobytes(), name


def _full_square(kind, X, ls, scale, diag, vec, sq):
    """vgposp_kernel_gemv_t(Xt = X) with its diagonal term a_i^2p amp^2p x_i replaced by
    diag_i^p x_i, on the device."""
    import torch
    from vgposp_amd.covariance import kernel_gemv_t
    full = kernel_gemv_t(kind, X, X, AMP, ls, vec, squared=sq, target_scale=scale,
                         site_scale=scale)
    n = X.shape[0]
    a2 = torch.ones(n, dtype=torch.float64, device="cuda") if scale is None else _dev(scale) ** 2
    own = a2 * AMP * AMP
    dg = own if diag is None else _dev(diag)
    v = _dev(vec)
    return (full + ((dg * dg - own * own) if sq else (dg - own)) * v).cpu().numpy()


@pytest.mark.parametrize("n,d,kind", [(1537, 3, "matern52"), (1025, 5, "eq"), (513, 2, "matern12")])
def test_equals_the_full_square_pass_and_the_stored_pass(n, d, kind):
    """vgposp_kernel_gemv_t with Xt = X plus the diagonal correction, and vgposp_symv_upper on the
    device-assembled matrix with the same diag: each within the sum of both bounds."""
    import torch
    from vgposp_amd import linalg
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    X, ls, x, w, _, dg = _inputs(n, d, 7 * n + d)
    S = SK.site_cov_ld(kind, X, AMP, ls, None, dg)
    Sd = linalg.kernel_matrix(kind, X, None, AMP, ls)[0]
    for (name, sq), vec in zip(FORMS, (x, w)):
        got = _launch(name, kind, X, ls, None, dg, vec).astype(K.LD)
        bound = 2 * SK.symv_bound(n, SK.symv_ld(S, vec, sq)[1], sq)
        full = _full_square(kind, X, ls, None, dg, vec, sq).astype(K.LD)
        print(f"{name} against the full square: worst difference / bound "
              f"{float(np.max(np.abs(got - full) / bound)):.3f}")
        assert (np.abs(got - full) <= bound).all()
        ws = torch.empty(query("vgposp_symv_upper_workspace_bytes", n), dtype=torch.uint8,
                         device="cuda")
        y = torch.zeros(n, dtype=torch.float64, device="cuda")
        xv, dv = _dev(vec), _dev(dg)
        call("vgposp_symv_upper_sq" if sq else "vgposp_symv_upper", _p(Sd), n, Sd.stride(0),
             _p(dv), _p(xv), _p(y), _p(ws), ws.numel(), _stream())
        stored = y.cpu().numpy().astype(K.LD)
        print(f"{name} against vgposp_symv_upper: worst difference / bound "
              f"{float(np.max(np.abs(got - stored) / bound)):.3f}")
        assert (np.abs(got - stored) <= bound).all()


def test_nine_groups_in_both_directions():
    """n = 512 * 8 + 1, EQ, d = 3, against the longdouble product."""
    n, d, kind = 4097, 3, "eq"
    X, ls, x, w, a, dg = _inputs(n, d, 4097)
    S = SK.site_cov_ld(kind, X, AMP, ls, a, dg)
    for (name, sq), vec in zip(FORMS, (x, w)):
        got = _launch(name, kind, X, ls, a, dg, vec)
        want, weight = SK.symv_ld(S, vec, sq)
        bound = SK.symv_bound(n, weight, sq)
        err = np.abs(got.astype(K.LD) - want)
        print(f"{name} n {n}: worst err / bound {float(np.max(err / bound)):.3f}")
        assert np.isfinite(got).all() and (err <= bound).all()
        assert got.tobytes() == _launch(name, kind, X, ls, a, dg, vec).tobytes()


@pytest.mark.parametrize("n", [32769, 229377], ids=["2x2-tile blocks", "8x8-tile blocks"])
def test_tile_blocks(n):
    """The smallest n at which a workgroup's block is 2 x 2 and 8 x 8 tiles, the last block ragged
    (a single row and column).  Against the full-square pass within the sum of both bounds, whose
    weight |Sigma| |x| the full-square pass gives too (every entry is positive), and for rows at
    the blocks' corners against the longdouble row."""
    d, kind = 3, "eq"
    X, ls, x, w, a, dg = _inputs(n, d, n)
    G = 2 if n == 32769 else 8
    rows = sorted({0, 1, 511, 512, 512 * G - 1, 512 * G, 512 * G + 1, n // 2, n - 513, n - 2,
                   n - 1})
    for (name, sq), vec in zip(FORMS, (x, w)):
        got = _launch(name, kind, X, ls, a, dg, vec)
        assert np.isfinite(got).all()
        assert got.tobytes() == _launch(name, kind, X, ls, a, dg, vec).tobytes()
        full = _full_square(kind, X, ls, a, dg, vec, sq)
        weight = _full_square(kind, X, ls, a, dg, np.abs(vec), sq).astype(K.LD)
        bound = 2 * SK.symv_bound(n, weight, sq)
        diff = np.abs(got.astype(K.LD) - full.astype(K.LD))
        print(f"{name} n {n} against the full square: worst difference / bound "
              f"{float(np.max(diff / bound)):.3f}")
        assert (diff <= bound).all()
        worst = 0.0
        for i in rows:
            r = K.kernel_ld(kind, X[i:i + 1], X, AMP, ls)[0] * K.LD(a[i]) * a.astype(K.LD)
            r[i] = dg[i]
            r = r * r if sq else r
            want, wt = r @ vec.astype(K.LD), np.abs(r) @ np.abs(vec).astype(K.LD)
            e = abs(K.LD(got[i]) - want) / SK.symv_bound(n, wt, sq)
            worst = max(worst, float(e))
        print(f"{name} n {n} against {len(rows)} longdouble rows: worst err / bound {worst:.3f}")
        assert worst <= 1.0


def test_host_wrapper():
    from vgposp_amd.covariance import kernel_symv
    X, ls, x, w, a, dg = _inputs(700, 3, 11)
    for scale, diag in ((None, None), (a, dg)):
        S = SK.site_cov_ld("matern32", X, AMP, ls, scale, diag)
        for vec, sq in ((x, False), (w, True)):
            got = kernel_symv("matern32", X, AMP, ls, vec, squared=sq, site_scale=scale,
                              diag=diag).cpu().numpy()
            want, weight = SK.symv_ld(S, vec, sq)
            assert (np.abs(got.astype(K.LD) - want) <= SK.symv_bound(700, weight, sq)).all()
    with pytest.raises(ValueError, match="shapes do not match"):
        kernel_symv("eq", X, AMP, ls, x[:-1])
    with pytest.raises(ValueError, match="shapes do not match"):
        kernel_symv("eq", X, AMP, ls, x, site_scale=a[:-1])
    with pytest.raises(ValueError, match="shapes do not match"):
        kernel_symv("eq", X, AMP, ls, x, diag=dg[:-1])


def test_kernel_symv_is_capturable():
    """No host synchronisation: the launch records into a graph, and the replay gives the bits of
    the eager launch."""
    import torch
    from vgposp_amd._lib import call, query
    from vgposp_amd.linalg import _p, _stream
    n, d = 1300, 3
    X, ls, x, _, a, dg = _inputs(n, d, 4)
    t = [_dev(v) for v in (X, np.array([AMP]), np.array([ls]), a, dg, x)]
    ws = torch.empty(query("vgposp_kernel_symv_workspace_bytes", n), dtype=torch.uint8,
                     device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    args = lambda: (3, _p(t[0]), n, d, _p(t[1]), _p(t[2]), _p(t[3]), _p(t[4]), _p(t[5]), _p(y),
                    _p(ws), ws.numel(), _stream())
    call("vgposp_kernel_symv", *args())
    torch.cuda.synchronize()
    eager = y.cpu().numpy().copy()
    y.zero_()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call("vgposp_kernel_symv", *args())   # (the capture stream is the current stream here)
    g.replay()
    torch.cuda.synchronize()
    assert y.cpu().numpy().tobytes() == eager.tobytes()
    assert np.isfinite(eager).all() and np.any(eager != 0.0)


def test_empty_dimension_does_no_device_work():
    from vgposp_amd._lib import call
    null = ctypes.c_void_p(0)
    for name in ("vgposp_kernel_symv", "vgposp_kernel_symv_sq"):
        assert call(name, 9, null, 0, 0, null, null, null, null, null, null, null, 0, null) == 0
