"""GPU parity of the FeatureScaled (per-feature length scale) path: vgposp_scale_points, the forward
assembly through scaled points, the one-pass scaled kernel VJP and LML gradient, the GP and VGP
fits that train scale_diag, and the predictive surfaces.  References: the unchanged oracle/gp.py
applied to pre-scaled points (tests/numpy_ard.py)."""
import numpy as np
import pytest

from oracle import gp as ogp
from tests import numpy_ard

pytestmark = pytest.mark.gpu

CLS = {"eq": "ExponentiatedQuadratic", "matern12": "MaternOneHalf",
       "matern32": "MaternThreeHalves", "matern52": "MaternFiveHalves"}
AMP, LS = 0.8, 0.9


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    torch.cuda.set_device(0)
    return torch


def _scales(d, seed=0):
    return np.random.default_rng(100 + d + seed).uniform(0.5, 2.0, d)


def _dev(torch, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device="cuda")


# ---- 1. scale_points ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("inplace", [False, True])
def test_scale_points(torch_dev, d, n, inplace):
    from vgposp_amd import linalg
    torch = torch_dev
    rng = np.random.default_rng(n + d)
    X, s = rng.normal(size=(n, d)), _scales(d)
    Xd = _dev(torch, X)
    out = linalg.scale_points(Xd, _dev(torch, s), out=Xd if inplace else None)
    assert (out.data_ptr() == Xd.data_ptr()) == inplace
    np.testing.assert_allclose(out.cpu().numpy(), X / s, rtol=1e-15, atol=0)
    if not inplace:
        assert np.array_equal(Xd.cpu().numpy(), X)


# ---- 2. FeatureScaled.matrix -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ogp.KERNELS)
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_matrix_matches_oracle_on_scaled_points(torch_dev, kind, d):
    from vgposp_amd import psd_kernels as psd
    torch = torch_dev
    rng = np.random.default_rng(d)
    n1, n2 = 37, 53
    X1, X2, s = rng.uniform(-2, 2, (n1, d)), rng.uniform(-2, 2, (n2, d)), _scales(d)
    base = getattr(psd, CLS[kind])(AMP, LS)
    k = psd.FeatureScaled(base, s)
    got = k.matrix(X1, X2).cpu().numpy()
    np.testing.assert_allclose(got, ogp.kernel_matrix(kind, X1 / s, X2 / s, AMP, LS)[0],
                               rtol=1e-13)
    # lower=True with a diagonal shift (the GP's C = K + shift I): lower triangle only
    gl = k.matrix(X1, X1, diag_shift=0.3, lower=True).cpu().numpy()
    ref = ogp.kernel_matrix(kind, X1 / s, X1 / s, AMP, LS)[0] + 0.3 * np.eye(n1)
    il = np.tril_indices(n1)
    np.testing.assert_allclose(gl[il], ref[il], rtol=1e-13)
    # paired rows
    np.testing.assert_allclose(k.apply(X1, X2[:n1]).cpu().numpy(),
                               np.diagonal(ogp.kernel_matrix(kind, X1 / s, X2[:n1] / s, AMP, LS)[0]),
                               rtol=1e-13)
    # unit scales: bit-identical to the base kernel
    ones = psd.FeatureScaled(base, _dev(torch, np.ones(d)))
    assert torch.equal(ones.matrix(X1, X2), base.matrix(X1, X2))
    # (a lower assembly leaves the strictly upper triangle unwritten)
    assert torch.equal(torch.tril(ones.matrix(X1, X1, diag_shift=0.3, lower=True)),
                       torch.tril(base.matrix(X1, X1, diag_shift=0.3, lower=True)))


# ---- 3. vgposp_kernel_vjp_scaled ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ogp.KERNELS)
@pytest.mark.parametrize("n1,n2", [(1, 1), (16, 1024), (37, 1100)])
@pytest.mark.parametrize("d", [1, 3, 5, 8])
def test_kernel_vjp_scaled(torch_dev, kind, n1, n2, d):
    from vgposp_amd import linalg
    from vgposp_amd.vgp_training import kernel_vjp
    torch = torch_dev
    rng = np.random.default_rng(n1 + n2 + d)
    X1, X2, s = rng.uniform(-2, 2, (n1, d)), rng.uniform(-2, 2, (n2, d)), _scales(d)
    Kb = rng.normal(size=(n1, n2))
    u, w = rng.normal(size=n1), rng.normal(size=n2)
    sd = _dev(torch, s)
    Z1, Z2 = linalg.scale_points(_dev(torch, X1), sd), linalg.scale_points(_dev(torch, X2), sd)
    ones = _dev(torch, np.ones(d))
    for rank1 in (False, True):
        ud, wd = (_dev(torch, u), _dev(torch, w)) if rank1 else (None, None)
        rg, rX = numpy_ard.kernel_vjp_scaled(kind, X1, X2, AMP, LS, s,
                                             Kb + (np.outer(u, w) if rank1 else 0.0))
        tolx = dict(rtol=1e-9, atol=1e-11 * np.abs(rX).max())
        g, Xb = kernel_vjp(kind, Z1, Z2, AMP, LS, _dev(torch, Kb), ud, wd, scale=sd)
        gn = g.cpu().numpy()
        assert gn.shape == (2 + d,)
        np.testing.assert_allclose(gn[:2], rg[:2], rtol=1e-10)
        np.testing.assert_allclose(Xb.cpu().numpy(), rX, **tolx)
        np.testing.assert_allclose(gn[2:], rg[2:], rtol=1e-9, atol=1e-11 * np.abs(rg[2:]).max())
        # scaling every feature is scaling the length scale
        assert np.dot(s, gn[2:]) == pytest.approx(LS * gn[1], rel=1e-9)
        # no atomics: a second call gives the same bits
        g2, Xb2 = kernel_vjp(kind, Z1, Z2, AMP, LS, _dev(torch, Kb), ud, wd, scale=sd)
        assert torch.equal(g, g2) and torch.equal(Xb, Xb2)
        # without X1bar: the same scalars
        g3, none = kernel_vjp(kind, Z1, Z2, AMP, LS, _dev(torch, Kb), ud, wd, want_x1bar=False,
                              scale=sd)
        assert none is None and torch.equal(g, g3)
        # unit scales: the isotropic entry
        gi, Xi = kernel_vjp(kind, X1, X2, AMP, LS, _dev(torch, Kb), ud, wd)
        go, Xo = kernel_vjp(kind, X1, X2, AMP, LS, _dev(torch, Kb), ud, wd, scale=ones)
        np.testing.assert_allclose(go[:2].cpu().numpy(), gi.cpu().numpy(), rtol=1e-13)
        np.testing.assert_allclose(Xo.cpu().numpy(), Xi.cpu().numpy(), rtol=1e-13)


@pytest.mark.parametrize("d", [1, 3])
def test_kernel_vjp_scaled_matern12_symmetric(torch_dev, d):
    """Z1 = Z2: r = 0 on the diagonal, where Matern 1/2 has no direction (sub-gradient 0)."""
    from vgposp_amd import linalg
    from vgposp_amd.vgp_training import kernel_vjp
    torch = torch_dev
    rng = np.random.default_rng(d)
    n = 37
    X, s = rng.uniform(-2, 2, (n, d)), _scales(d)
    Kb = rng.normal(size=(n, n))
    sd = _dev(torch, s)
    Z = linalg.scale_points(_dev(torch, X), sd)
    g, Xb = kernel_vjp("matern12", Z, Z, AMP, LS, _dev(torch, Kb), scale=sd)
    rg, rX = numpy_ard.kernel_vjp_scaled("matern12", X, X, AMP, LS, s, Kb)
    gn = g.cpu().numpy()
    assert np.isfinite(gn).all()
    np.testing.assert_allclose(gn[:2], rg[:2], rtol=1e-10)
    np.testing.assert_allclose(Xb.cpu().numpy(), rX, rtol=1e-9, atol=1e-11 * np.abs(rX).max())
    np.testing.assert_allclose(gn[2:], rg[2:], rtol=1e-9, atol=1e-11 * np.abs(rg[2:]).max())


# ---- 4. vgposp_lml_grad_scaled -----------------------------------------------------------------
def _gp_problem(n, d, seed=0):
    rng = np.random.default_rng(seed + n + d)
    X = rng.uniform(-2, 2, (n, d))
    y = np.sin(2 * X).sum(1) + rng.normal(0, 0.1, n)
    return X, y


@pytest.mark.parametrize("kind", ogp.KERNELS)
@pytest.mark.parametrize("n", [1, 17, 300])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_lml_grad_scaled(torch_dev, kind, n, d):
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as psd
    torch = torch_dev
    X, y = _gp_problem(n, d)
    s, noise = _scales(d), 0.2
    base = getattr(psd, CLS[kind])(AMP, LS)
    gp = tfd.GaussianProcess(psd.FeatureScaled(base, s), X, observation_noise_variance=noise)
    lml, ga, gl, gn, gs = gp.log_prob_and_grads(y)
    got = np.concatenate([t.cpu().numpy().reshape(-1) for t in (ga, gl, gn, gs)])
    rl, rg = numpy_ard.lml_and_grads_scaled(kind, X, y, AMP, LS, noise, s)
    assert float(lml) == pytest.approx(rl, rel=1e-8)
    assert got.shape == (3 + d,)
    np.testing.assert_allclose(got, rg, rtol=1e-7, atol=1e-9 * np.abs(rg).max())
    # unit scales: the isotropic entry's three values
    gp1 = tfd.GaussianProcess(psd.FeatureScaled(base, np.ones(d)), X,
                              observation_noise_variance=noise)
    _, a1, l1, n1, _ = gp1.log_prob_and_grads(y)
    iso = tfd.GaussianProcess(base, X, observation_noise_variance=noise).log_prob_and_grads(y)
    assert len(iso) == 4
    np.testing.assert_allclose([float(a1), float(l1), float(n1)],
                               [float(t) for t in iso[1:]], rtol=1e-12)


# ---- 5. GP fit ---------------------------------------------------------------------------------
def test_gp_fit_trains_scale_diag(torch_dev):
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as psd
    from vgposp_amd.data_generation import grid_observations, grid_points
    from vgposp_amd.optimizers import AdamOptimizer, negate
    from vgposp_amd.variables import Softplus, Variable
    X = grid_points((6, 6, 6), jitter=0.05, seed=0)
    y = grid_observations(X)
    v0 = dict(amp=0.3, ls=0.1, noise=-2.0, scale=np.array([-0.4, 0.2, 0.9]))
    amp, ls, noise = (Softplus(Variable(v0[k], name=k)) for k in ("amp", "ls", "noise"))
    scale = Softplus(Variable(v0["scale"], name="scale_diag"))
    kernel = psd.FeatureScaled(psd.ExponentiatedQuadratic(amp, ls), scale)
    gp = tfd.GaussianProcess(kernel, X, observation_noise_variance=noise)
    train_op = AdamOptimizer(0.05).minimize(negate(gp.log_prob(y)))
    assert set(train_op.variables()) == {"amp", "ls", "noise", "scale"}
    got = [float(train_op.run()) for _ in range(10)]
    # oracle: the same transforms and Adam, driven by the reference gradients
    th = np.concatenate([[v0["amp"], v0["ls"], v0["noise"]], v0["scale"]])
    opt = ogp.AdamTF1(0.05)
    ref = []
    for _ in range(10):
        c = ogp.constrain(th)
        lml, g = numpy_ard.lml_and_grads_scaled("eq", X, y, c[0], c[1], c[2], c[3:])
        ref.append(lml)
        th = opt.step(th, -g * ogp.sigmoid(th))
    np.testing.assert_allclose(got, ref, rtol=1e-7)
    c = ogp.constrain(th)
    np.testing.assert_allclose([float(amp.numpy()), float(ls.numpy()), float(noise.numpy())],
                               c[:3], rtol=1e-7)
    np.testing.assert_allclose(scale.numpy(), c[3:], rtol=1e-7)


# ---- 6. VGP ------------------------------------------------------------------------------------
VGP_S = np.array([0.6, 1.0, 1.7])


def _vgp_problem(seed=3, N=600, M=24, nb=128, ls=0.7):
    """Inducing points: 24 of a jittered 3^3 grid with spacing 1.3 ls in SCALED coordinates, so the
    unjittered Kzz (whose log-det the KL term needs) stays well conditioned."""
    rng = np.random.default_rng(seed)
    h = 1.3 * ls
    g = (np.arange(3) - 1.0) * h
    Zz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    Zz = (Zz + rng.uniform(-0.1, 0.1, Zz.shape) * h)[:M]
    Xz = rng.uniform(-1.5 * h, 1.5 * h, (N, 3))
    y = np.sin(2 * Xz).sum(1) + rng.normal(0, 0.1, N)
    idx = rng.integers(0, N, nb)
    return Xz * VGP_S, y, Zz * VGP_S, idx


@pytest.fixture(scope="module")
def vgp_refs():
    """The oracle's loss and gradients (the scale part by central differences), once per kind."""
    X, y, Z, idx = _vgp_problem()
    return {kind: numpy_ard.vgp_loss_grads_scaled(kind, Z, X, y, X[idx], y[idx], 0.9, 0.7, 0.05,
                                                  VGP_S, 128 / 600)
            for kind in ("eq", "matern52")}


@pytest.mark.parametrize("kind", ["eq", "matern52"])
def test_vgp_objective_scaled(torch_dev, vgp_refs, kind):
    from vgposp_amd.vgp_training import VGPObjective
    torch = torch_dev
    X, y, Z, idx = _vgp_problem()
    obj = VGPObjective(kind, X, y)
    L, ga, gl, gs, gZ, gsc = obj.loss_and_grads(Z, 0.9, 0.7, 0.05, X[idx], y[idx], 128 / 600,
                                                scale=_dev(torch, VGP_S))
    rL, rga, rgl, rgs, rgZ, rgsc = vgp_refs[kind]
    assert float(L) == pytest.approx(rL, rel=1e-8)
    np.testing.assert_allclose([float(ga), float(gl), float(gs)], [rga, rgl, rgs], rtol=1e-6)
    np.testing.assert_allclose(gZ.cpu().numpy(), rgZ, rtol=1e-6, atol=1e-8 * np.abs(rgZ).max())
    np.testing.assert_allclose(gsc.cpu().numpy(), rgsc, rtol=1e-5,
                               atol=1e-6 * np.abs(rgsc).max())
    # the isotropic five-tuple is unchanged
    assert len(obj.loss_and_grads(Z, 0.9, 0.7, 0.05, X[idx], y[idx], 128 / 600)) == 5


def _vgp_graph(X, y, Z, B, kind, graph=True, group=None):
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as psd
    from vgposp_amd.optimizers import AdamOptimizer
    from vgposp_amd.variables import Softplus, Variable, placeholder
    amp = Softplus(Variable(0.54, name="amplitude"), offset=0.0)
    ls = Softplus(Variable(0.2, name="length_scale"), offset=1e-5)
    noise = Softplus(Variable(-2.0, name="observation_noise_variance"), offset=0.0)
    scale = Softplus(Variable(ogp.invert_softplus(VGP_S), name="scale_diag"), offset=0.0)
    kernel = psd.FeatureScaled(getattr(psd, CLS[kind])(amplitude=amp, length_scale=ls), scale)
    Zv = Variable(Z, name="inducing_index_points")
    loc, sc = tfd.VariationalGaussianProcess.optimal_variational_posterior(
        kernel=kernel, inducing_index_points=Zv, observation_index_points=X, observations=y,
        observation_noise_variance=noise)
    vgp = tfd.VariationalGaussianProcess(kernel, index_points=Z[:8], inducing_index_points=Zv,
                                         variational_inducing_observations_loc=loc,
                                         variational_inducing_observations_scale=sc,
                                         observation_noise_variance=noise)
    xb = placeholder(np.float64, [B, 3], name="x_train_batch")
    yb = placeholder(np.float64, [B], name="y_train_batch")
    loss = vgp.variational_loss(observations=yb, observation_index_points=xb,
                                kl_weight=float(B) / len(X))
    op = AdamOptimizer(learning_rate=0.01).minimize(loss, group=group, graph=graph)
    return op, xb, yb, (amp, ls, noise, scale, Zv)


@pytest.mark.parametrize("kind", ["eq", "matern52"])
def test_vgp_train_graph_equals_eager(torch_dev, kind):
    torch = torch_dev
    X, y, Z, _ = _vgp_problem()
    B = 128
    rng = np.random.default_rng(1)
    idx = [rng.integers(0, len(X), B) for _ in range(6)]
    res = {}
    for graph in (True, False):
        op, xb, yb, params = _vgp_graph(X, y, Z, B, kind, graph=graph)
        assert op.train_scale and op.z_off - op.s_off == 3
        start = params[3].numpy().copy()
        losses = [float(op.run({xb: X[i], yb: y[i]})) for i in idx]
        op.check()
        assert (op._g is not None) == graph
        res[graph] = (losses, [np.asarray(p.numpy()).copy() for p in params])
        assert not np.allclose(params[3].numpy(), start, rtol=1e-4)  # the scales did train
    np.testing.assert_allclose(res[True][0], res[False][0], rtol=1e-12)
    for a, b in zip(res[True][1], res[False][1]):
        np.testing.assert_allclose(a, b, rtol=1e-12)


def test_vgp_train_data_parallel_is_refused(torch_dev):
    X, y, Z, _ = _vgp_problem()
    with pytest.raises(NotImplementedError, match="FeatureScaled"):
        _vgp_graph(X, y, Z, 128, "eq", group=object())


# ---- 7. predictive surfaces --------------------------------------------------------------------
def test_gprm_mean_and_variance(torch_dev):
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as psd
    X, y = _gp_problem(150, 3)
    Xs = np.random.default_rng(9).uniform(-2, 2, (301, 3))
    s = _scales(3)
    base = psd.MaternFiveHalves(AMP, LS)
    mk = lambda k, f: tfd.GaussianProcessRegressionModel(
        k, index_points=f(Xs), observation_index_points=f(X), observations=y,
        observation_noise_variance=0.05)
    a, b = mk(psd.FeatureScaled(base, s), lambda p: p), mk(base, lambda p: p / s)
    for chunk in (None, 128):
        (m1, v1), (m2, v2) = (g.mean_and_variance(chunk_points=chunk) for g in (a, b))
        np.testing.assert_allclose(m1.cpu().numpy(), m2.cpu().numpy(), rtol=1e-12)
        np.testing.assert_allclose(v1.cpu().numpy(), v2.cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(a.stddev().cpu().numpy(), b.stddev().cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(a.mean().cpu().numpy(), b.mean().cpu().numpy(), rtol=1e-12)


def _vgp_pair(d, s, seed=2):
    """The same VGP with FeatureScaled(base, s) on raw points and with base on points / s."""
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as psd
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (400, d))
    y = np.sin(2 * X).sum(1) + rng.normal(0, 0.1, 400)
    Z = rng.uniform(-2, 2, (20, d))
    Xs = rng.uniform(-2, 2, (301, d))
    base = psd.ExponentiatedQuadratic(AMP, LS)
    out = []
    for k, f in ((psd.FeatureScaled(base, s), lambda p: p), (base, lambda p: p / s)):
        loc, sc = tfd.VariationalGaussianProcess.optimal_variational_posterior(
            kernel=k, inducing_index_points=f(Z), observation_index_points=f(X), observations=y,
            observation_noise_variance=0.05)
        out.append(tfd.VariationalGaussianProcess(
            k, index_points=f(Xs), inducing_index_points=f(Z),
            variational_inducing_observations_loc=loc,
            variational_inducing_observations_scale=sc, observation_noise_variance=0.05))
    return out


def test_vgp_variance_chunked(torch_dev):
    a, b = _vgp_pair(3, _scales(3))
    for chunk in (None, 100):
        np.testing.assert_allclose(a.variance(chunk_points=chunk).cpu().numpy(),
                                   b.variance(chunk_points=chunk).cpu().numpy(), rtol=1e-12)
    (m1, v1), (m2, v2) = (g.mean_and_variance(chunk_points=100) for g in (a, b))
    np.testing.assert_allclose(m1.cpu().numpy(), m2.cpu().numpy(), rtol=1e-12)
    np.testing.assert_allclose(v1.cpu().numpy(), v2.cpu().numpy(), rtol=1e-12)


def test_cov_vv_from_vgp(torch_dev):
    from vgposp_amd.covariance import cov_vv_from_vgp
    s = _scales(5)
    a, b = _vgp_pair(5, s)
    rng = np.random.default_rng(4)
    loc, tp = rng.uniform(-2, 2, (40, 3)), rng.uniform(-2, 2, (25, 2))
    got = cov_vv_from_vgp(a, loc, tp).cpu().numpy()
    ref = cov_vv_from_vgp(b, loc / s[:3], tp / s[3:]).cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12)
