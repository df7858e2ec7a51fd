"""GPU: the marginal predictive variance without the P x P covariance.

* ``linalg.row_sumsq`` (vgposp_row_sumsq) against numpy in ``longdouble``.  Tolerance: relative
  cols * 2^-52, the worst-case bound of ANY summation order of cols squared terms, so it does not
  prescribe the kernel's order.  With ``beta != 0`` the accumulated ``beta * out`` is one more
  term of the same sum, so the bound is taken relative to sum_j V_ij^2 + |beta out_i| (for
  beta = 0 exactly the relative bound on the row sum).
* ``variance`` / ``stddev`` / ``mean_and_variance`` of the three GP surfaces against the diagonal
  of the oracle's full covariance (oracle/gp.py), against the reference-executed fixture
  tests/golden/gprm_confidence.npz (s2 = diag(K_ss) - sum(Lk^2), plot_confidence_interval.py:51),
  and against their own ``covariance()``; tolerances are those of the existing covariance tests
  (test_gpu_gp.py, test_gpu_gprm_golden.py).
* Peak device memory of a P = 16,384 map, and the properties of an uncertainty map on a placement.
"""
import os

import numpy as np
import pytest

from oracle import gp as ogp

pytestmark = pytest.mark.gpu

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gprm_confidence.npz")
MIB = 1 << 20


@pytest.fixture(scope="module")
def mods():
    import torch
    torch.cuda.set_device(0)
    from vgposp_amd import distributions, linalg, psd_kernels
    return torch, distributions, psd_kernels, linalg


# ---- row_sumsq ----------------------------------------------------------------------------------

# the first eight are the shapes every path switch needs (1 column, short rows in sub-groups,
# 63 / 64 / 65 around one wave per row, several blocks of four loads, more rows than one
# workgroup); the last two put 16-byte loads on the short-row path
SHAPES = [(1, 1), (3, 1), (5, 63), (4, 64), (7, 65), (129, 257), (2, 4099), (1000, 50),
          (9, 24), (6, 31)]


def _strip(torch, rows, cols, pad, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-3, 4, (rows, cols))
    buf = torch.full((rows, cols + pad), float("nan"), dtype=torch.float64, device="cuda")
    buf[:, :cols] = torch.as_tensor(V, device="cuda")
    S = (V.astype(np.longdouble) ** 2).sum(axis=1)
    return V, buf[:, :cols], S, rng


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_row_sumsq_matches_longdouble(mods, rows, cols, pad):
    torch, _, _, linalg = mods
    V, Vd, S, rng = _strip(torch, rows, cols, pad, seed=1000 * rows + cols)
    if rows > 1:
        assert Vd.stride(0) == cols + pad
    tol = cols * 2.0 ** -52
    # alpha = 1, beta = 0 onto NaN: out must not be read
    out = torch.full((rows,), float("nan"), dtype=torch.float64, device="cuda")
    r = linalg.row_sumsq(Vd, out=out, alpha=1.0, beta=0.0)
    assert r is out
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.longdouble) - S)
    print(f"row_sumsq {rows}x{cols} pad {pad}: max rel err {float((err / S).max()):.3e} (tol {tol:.3e})")
    assert np.isfinite(got).all()
    assert (err <= tol * S).all()
    again = linalg.row_sumsq(Vd).cpu().numpy()
    assert np.array_equal(again, got), "a second run is not bit-identical"
    # alpha = -1, beta = 1 onto a random out
    o0 = rng.standard_normal(rows) * 10.0 ** rng.integers(-3, 4, rows)
    out2 = torch.as_tensor(o0, device="cuda").clone()
    linalg.row_sumsq(Vd, out=out2, alpha=-1.0, beta=1.0)
    got2 = out2.cpu().numpy()
    exp2 = o0.astype(np.longdouble) - S
    err2 = np.abs(got2.astype(np.longdouble) - exp2)
    assert (err2 <= tol * (S + np.abs(o0))).all(), float((err2 / (S + np.abs(o0))).max())
    out3 = torch.as_tensor(o0, device="cuda").clone()
    linalg.row_sumsq(Vd, out=out3, alpha=-1.0, beta=1.0)
    assert np.array_equal(out3.cpu().numpy(), got2)


def test_row_sumsq_zero_columns_scales_out(mods):
    torch, _, _, linalg = mods
    V = torch.empty((6, 0), dtype=torch.float64, device="cuda")
    out = torch.arange(6, dtype=torch.float64, device="cuda")
    linalg.row_sumsq(V, out=out, alpha=1.0, beta=-2.0)
    np.testing.assert_array_equal(out.cpu().numpy(), -2.0 * np.arange(6))
    assert linalg.row_sumsq(V).cpu().numpy().tolist() == [0.0] * 6


# ---- GPRM ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gprm_case(mods):
    _, dist, psd, _ = mods
    rng = np.random.default_rng(11)
    n, P = 151, 1037
    X = rng.uniform(-2, 2, (n, 2))
    y = np.sin(2 * np.pi * X).sum(1) + rng.normal(0, 0.03, n)
    Xs = rng.uniform(-2, 2, (P, 2))
    amp, ls = np.array([0.9, 1.2]), np.array([0.5, 0.7])
    gprm = dist.GaussianProcessRegressionModel(
        psd.ExponentiatedQuadratic(amp, ls), index_points=Xs, observation_index_points=X,
        observations=y, observation_noise_variance=0.05, predictive_noise_variance=0.0)
    rm, rc = ogp.gprm_mean_cov("eq", Xs, X, y, amp, ls, 0.05, 0.0)
    return gprm, Xs, rm, np.diagonal(rc, axis1=-2, axis2=-1).copy()


def test_gprm_variance_matches_oracle_diagonal(gprm_case):
    gprm, Xs, _, rvar = gprm_case
    v = gprm.variance(chunk_points=256).cpu().numpy()   # four full chunks and one of 13
    assert v.shape == (2, 1037)
    print("gprm var vs oracle: max abs err", np.abs(v - rvar).max())
    np.testing.assert_allclose(v, rvar, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gprm.variance().cpu().numpy(), rvar, rtol=1e-7, atol=1e-9)
    sd = gprm.stddev(chunk_points=256).cpu().numpy()
    np.testing.assert_allclose(sd, np.sqrt(v), rtol=1e-15)
    # a one-row chunk, on call-time index points
    v1 = gprm.variance(index_points=Xs[:5], chunk_points=1).cpu().numpy()
    assert v1.shape == (2, 5)
    np.testing.assert_allclose(v1, rvar[:, :5], rtol=1e-7, atol=1e-9)


def test_gprm_variance_matches_own_covariance(gprm_case):
    gprm, _, _, _ = gprm_case
    v = gprm.variance(chunk_points=256).cpu().numpy()
    c = gprm.covariance().cpu().numpy()
    np.testing.assert_allclose(v, np.diagonal(c, axis1=-2, axis2=-1), rtol=0, atol=1e-11)


def test_gprm_mean_and_variance_one_pass(gprm_case):
    gprm, _, rm, rvar = gprm_case
    m, v = gprm.mean_and_variance(chunk_points=256)
    assert tuple(m.shape) == (2, 1037) and tuple(v.shape) == (2, 1037)
    np.testing.assert_allclose(m.cpu().numpy(), gprm.mean().cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(m.cpu().numpy(), rm, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(v.cpu().numpy(), rvar, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize("chunk", [97, 1, None])
def test_gprm_variance_matches_reference_fixture(mods, chunk):
    _, dist, psd, _ = mods
    z = np.load(FIX)
    k = psd.ExponentiatedQuadratic(1.0, np.sqrt(float(z["param"])))
    gprm = dist.GaussianProcessRegressionModel(
        k, index_points=z["Xtest"], observation_index_points=z["Xtrain"],
        observations=z["ytrain"].reshape(-1), observation_noise_variance=float(z["diag_shift"]),
        predictive_noise_variance=0.0, jitter=0.0)
    m, v = gprm.mean_and_variance(chunk_points=chunk)       # 700 = 7 * 97 + 21
    assert tuple(v.shape) == (700,)
    print("gprm var vs fixture: max abs err", np.abs(v.cpu().numpy() - z["s2"]).max())
    np.testing.assert_allclose(v.cpu().numpy(), z["s2"], rtol=0, atol=1e-13)
    np.testing.assert_allclose(m.cpu().numpy(), z["mu"], rtol=0, atol=1e-13)


# ---- VGP ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,M", [("eq", 40), ("matern52", 40), ("eq", 1)])
def test_vgp_variance_matches_oracle_diagonal(mods, kind, M):
    _, dist, psd, _ = mods
    rng = np.random.default_rng(7)
    N, P = 600, 517
    X = rng.uniform(-2, 2, (N, 2))
    y = np.sin(2 * X).sum(1) + rng.normal(0, 0.1, N)
    Z = rng.uniform(-2, 2, (M, 2))
    Xs = rng.uniform(-2, 2, (P, 2))
    cls = {"eq": psd.ExponentiatedQuadratic, "matern52": psd.MaternFiveHalves}[kind]
    k = cls(0.9, 0.7)
    loc, scale = dist.VariationalGaussianProcess.optimal_variational_posterior(k, Z, X, y, 0.05)
    rloc, rscale = ogp.vgp_optimal_posterior(kind, Z, X, y, 0.9, 0.7, 0.05)
    vgp = dist.VariationalGaussianProcess(k, Xs, Z, loc, scale, observation_noise_variance=0.05)
    rm, rc = ogp.vgp_predictive(kind, Xs, Z, rloc, rscale, 0.9, 0.7, 0.05)
    m, v = vgp.mean_and_variance(chunk_points=128)           # four full chunks and one of 5
    assert tuple(v.shape) == (517,)
    print("vgp var vs oracle: max abs err", np.abs(v.cpu().numpy() - np.diag(rc[0])).max())
    np.testing.assert_allclose(v.cpu().numpy(), np.diag(rc[0]), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(m.cpu().numpy(), rm[0], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(m.cpu().numpy(), vgp.mean().cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(vgp.variance().cpu().numpy(), np.diag(rc[0]), rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(vgp.stddev(chunk_points=128).cpu().numpy(),
                               np.sqrt(v.cpu().numpy()), rtol=1e-15)


# ---- GP prior -----------------------------------------------------------------------------------

def test_gp_prior_variance(mods):
    _, dist, psd, _ = mods
    amp, ls = np.array([0.9, 1.2]), np.array([0.5, 0.7])
    X = np.random.default_rng(3).uniform(-2, 2, (333, 3))
    gp = dist.GaussianProcess(psd.MaternThreeHalves(amp, ls), X, observation_noise_variance=0.3)
    v = gp.variance(chunk_points=64).cpu().numpy()
    assert v.shape == (2, 333)
    np.testing.assert_allclose(v, np.broadcast_to((amp ** 2 + 0.3)[:, None], (2, 333)), rtol=1e-15)
    np.testing.assert_allclose(gp.stddev().cpu().numpy(), np.sqrt(v), rtol=1e-15)
    assert tuple(gp.variance(index_points=X[:7]).shape) == (2, 7)


# ---- memory -------------------------------------------------------------------------------------

def _peak_mib(torch, fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / MIB
    assert bool(torch.isfinite(out).all())
    return peak


@pytest.fixture(scope="module")
def big_gprm(mods):
    """n = 256, P = 16,384: the full posterior covariance alone is 2 GiB."""
    torch, dist, psd, _ = mods
    rng = np.random.default_rng(5)
    X = rng.uniform(-2, 2, (256, 2))
    y = np.sin(2 * X).sum(1)
    Xs = torch.as_tensor(rng.uniform(-2, 2, (16384, 2)), device="cuda")
    return dist.GaussianProcessRegressionModel(
        psd.ExponentiatedQuadratic(0.9, 0.5), index_points=Xs, observation_index_points=X,
        observations=y, observation_noise_variance=0.05)


@pytest.fixture(scope="module")
def big_vgp(mods):
    torch, dist, psd, _ = mods
    rng = np.random.default_rng(6)
    M = 128
    Z = rng.uniform(-2, 2, (M, 2))
    loc = rng.standard_normal(M)
    scale = 0.1 * np.tril(rng.standard_normal((M, M))) + 0.5 * np.eye(M)
    Xs = torch.as_tensor(rng.uniform(-2, 2, (16384, 2)), device="cuda")
    return dist.VariationalGaussianProcess(psd.ExponentiatedQuadratic(0.9, 0.5), Xs, Z, loc, scale,
                                           observation_noise_variance=0.05)


def test_gprm_variance_memory_default_chunk(mods, big_gprm):
    p = _peak_mib(mods[0], lambda: big_gprm.variance())
    print(f"gprm variance peak, default chunk: {p:.1f} MiB")
    assert p < 512


def test_gprm_variance_memory_chunk_1024(mods, big_gprm):
    """The two [1024, 256] strips are 4 MiB.  The factorization of the 256 x 256 observation
    covariance runs in the compact Cholesky workspace (4.4 MiB; the full one, with its fixed
    64 MiB of split-K partials, would alone exceed the bound)."""
    p = _peak_mib(mods[0], lambda: big_gprm.variance(chunk_points=1024))
    print(f"gprm variance peak, chunk 1024: {p:.1f} MiB")
    assert p < 64


def test_vgp_variance_memory_default_chunk(mods, big_vgp):
    p = _peak_mib(mods[0], lambda: big_vgp.variance())
    print(f"vgp variance peak, default chunk: {p:.1f} MiB")
    assert p < 512


def test_vgp_variance_memory_chunk_1024(mods, big_vgp):
    p = _peak_mib(mods[0], lambda: big_vgp.variance(chunk_points=1024))
    print(f"vgp variance peak, chunk 1024: {p:.1f} MiB")
    assert p < 64


def test_predict_chunk_budget(mods):
    _, dist, _, _ = mods
    assert dist.PREDICT_CHUNK_BYTES <= 256 * MIB
    for n, strips in [(1, 2), (50, 2), (4096, 2), (512, 3), (10 ** 6, 3)]:
        c = dist._predict_chunk(10 ** 9, n, strips)
        assert c >= 256 and c % 256 == 0
        assert c == 256 or 8 * c * n * strips <= dist.PREDICT_CHUNK_BYTES
        assert 8 * (c + 256) * n * strips > dist.PREDICT_CHUNK_BYTES
    assert dist._predict_chunk(13, 50, 2) == 13
    assert dist._predict_chunk(1000, 50, 2, chunk_points=97) == 97


# ---- an uncertainty map on a placement ----------------------------------------------------------

def test_variance_map_on_placement(mods):
    _, dist, psd, _ = mods
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_algorithm2 import placement_from_points
    shp, k, amp, noise, jitter = (6, 6, 6), 8, 1.0, 1e-2, 1e-6
    X = grid_points(shp, jitter=0.05, seed=0)
    ls = 2.0 * grid_spacing(shp)
    picks = [int(a) for a in placement_from_points(X, k, "eq", amp, ls, noise, jitter)]
    assert len(set(picks)) == k
    kern = psd.ExponentiatedQuadratic(amp, ls)
    means = [amp ** 2]   # the prior map
    for t in range(1, k + 1):
        A = picks[:t]
        gprm = dist.GaussianProcessRegressionModel(
            kern, index_points=X, observation_index_points=X[A], observations=np.zeros(t),
            observation_noise_variance=noise, predictive_noise_variance=0.0, jitter=jitter)
        v = gprm.variance(chunk_points=100).cpu().numpy()    # 216 = 2 * 100 + 16; n = 1 ... 8
        assert v.shape == (216,)
        assert v.min() >= -1e-12 and v.max() <= amp ** 2 + 0.0 + 1e-12
        assert (v[A] < noise).all(), v[A]
        means.append(float(v.mean()))
    assert all(b < a for a, b in zip(means, means[1:])), means
