"""GPU: the variance-reduction and entropy placements on a covariance that is never stored (the
vgposp_critg_* / vgposp_critgk_* entries through placement_criteria.SiteKernel) against the
longdouble references of tests/numpy_criteria_greedy.py and tests/numpy_cross_criteria.py, used as
they are: the fixtures' Sigma is fed as points, kernel, length scale, amplitude field and diagonal
(tests/test_site_kernel_reference.py shows on the CPU that these generate that Sigma to 1e-13 and
that the rounds' gaps hold on the generated matrix).

Tolerance 1e-9 (the project's tolerance for deltas): delta and s relative to the round's pick
delta, nom and the new rows of W and U relative to max diag Sigma.  F1 (n = 1,320) spans three
512-tiles, F2 (n = 819) two, both with a ragged last tile."""
import os
import sys

import numpy as np
import pytest

from tests import numpy_criteria_greedy as C
from tests import numpy_cross_criteria as X
from tests import numpy_kernel_cross as K
from tests import numpy_site_kernel as SK
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu
TOL = C.STATE_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [(f, c, "variance") for f in ("F1", "F2") for c in ("plain", "random", "oddeven")] \
    + [(f, "plain", "entropy") for f in ("F1", "F2")]


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def PC():
    from vgposp_amd import placement_criteria
    return placement_criteria


_dev = {}


def _fixture(PC, name):
    """(Sigma on the device, SiteKernel), uploaded once and never written."""
    import torch
    if name not in _dev:
        kind, Xs, amp, ls, a, diag = SK.fixture_site(name)
        site = PC.SiteKernel(kind, Xs, amp, ls, scale=a, noise=diag - a * a * amp * amp)
        _dev[name] = torch.tensor(C.fixture_cov(name), device="cuda"), site
    return _dev[name]


def _cross_fixture(PC, name):
    """(Sigma, SiteKernel, CrossKernel.from_site) of a fixture of numpy_cross_criteria."""
    import torch
    if name not in _dev:
        kind, Xs, Xt, amp, ls, a_s, a_t = K.fixture_points(name)
        site = PC.SiteKernel(kind, Xs, amp, ls, scale=a_s, noise=1e-2 * a_s * a_s)
        gen = PC.CrossKernel.from_site(site, Xt, target_scale=a_t)
        _dev[name] = torch.tensor(X.fixture(name)[0], device="cuda"), site, gen
    return _dev[name]


def _host(t):
    return t.cpu().numpy().copy()


@pytest.mark.parametrize("name,config,criterion", CONFIGS, ids=["-".join(c) for c in CONFIGS])
def test_picks_and_state(PC, name, config, criterion):
    """Every round of the reference: the pick, then the whole state; beside it the dense run on
    the fixture's stored Sigma, whose picks are the same and whose deltas lie within 1e-9."""
    require_longdouble()
    S, site = _fixture(PC, name)
    before = _host(site.X), _host(site.diag)
    T, cand = C.config_masks(name, config)
    T = None if criterion == "entropy" else T
    ref = C.reference(name, config, criterion)
    g = PC.CriterionPlacement(site, C.K_ROUNDS, criterion, candidates=cand, targets=T).init()
    dense = PC.CriterionPlacement(S, C.K_ROUNDS, criterion, candidates=cand, targets=T).init()
    smax = float(np.max(np.diag(C.fixture_cov(name))))
    worst = {"delta": 0.0, "s": 0.0, "nom": 0.0, "W": 0.0, "dense": 0.0}
    for r, want in enumerate(ref):
        g.step()
        dense.step()
        st = g.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        assert int(dense.selected[r]) == want.pick, r
        scale = float(want.pick_delta)
        err = {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
               "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
               "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax,
               "dense": abs(float(g.sel_delta[r]) - float(dense.sel_delta[r])) / scale}
        if criterion == "variance":
            err["s"] = np.max(np.abs(_host(st["s"]) - want.s)) / scale
        for key, e in err.items():
            worst[key] = max(worst[key], float(e))
        assert abs(float(g.sel_delta[r]) - scale) <= TOL * scale, r
    print(f"site-kernel criteria {name}-{config}-{criterion}: "
          + " ".join(f"{key} {v:.1e}" for key, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert [int(p) for p in dense.result()[0]] == [int(p) for p in picks]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (C.K_ROUNDS,)
    if cand is not None:
        assert cand[picks].all()
    assert g.state()["W"].shape == (C.K_ROUNDS, site.N)
    assert _host(site.X).tobytes() == before[0].tobytes()          # the points are only read
    assert _host(site.diag).tobytes() == before[1].tobytes()


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_placed_continues_a_free_run(PC, criterion):
    _, site = _fixture(PC, "F1")
    picks, deltas = PC.CriterionPlacement(site, 8, criterion).run().result()
    assert [int(p) for p in picks] == [w.pick for w in C.reference("F1", "plain", criterion)[:8]]
    g = PC.CriterionPlacement(site, 4, criterion, placed=picks[:4]).run()
    more, dmore = g.result()
    assert [int(p) for p in more] == [int(p) for p in picks[4:]]
    np.testing.assert_allclose(dmore, deltas[4:], rtol=TOL, atol=0)
    assert g.state()["W"].shape == (8, site.N)


def test_two_runs_are_bit_identical(PC):
    _, site = _fixture(PC, "F2")
    a = PC.CriterionPlacement(site, 6, "variance").run()
    b = PC.CriterionPlacement(site, 6, "variance").run()
    assert _host(a.sel_delta).tobytes() == _host(b.sel_delta).tobytes()
    for key in ("nom", "s", "delta", "W"):
        assert _host(a.state()[key]).tobytes() == _host(b.state()[key]).tobytes(), key


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_five_dimensional_sites(PC, criterion):
    """The 3^5 site set of numpy_kernel_cross.d5_case, Matern 3/2, diag = amp^2 + noise: the
    run-time-dimension form of the pass and of the column."""
    require_longdouble()
    Xs, _, ls, S, _ = K.d5_case()
    site = PC.SiteKernel(K.D5_KIND, Xs, K.D5_AMP, ls, noise=K.D5_NOISE)
    ref = C.reference_run(S, criterion, K.D5_K)
    gaps = C.round_gaps(ref, None)
    assert all(gap >= C.MIN_GAP and lowest for gap, lowest in gaps), gaps
    g = PC.CriterionPlacement(site, K.D5_K, criterion).init()
    smax = float(np.max(np.diag(S)))
    worst = 0.0
    for r, want in enumerate(ref):
        g.step()
        st = g.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        scale = float(want.pick_delta)
        errs = [np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
                np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
                np.max(np.abs(_host(st["W"][r]) - want.w)) / smax]
        if criterion == "variance":
            errs.append(np.max(np.abs(_host(st["s"]) - want.s)) / scale)
        worst = max(worst, *(float(e) for e in errs))
    print(f"site-kernel criteria 5-D {criterion}: worst {worst:.1e}, smallest gap "
          f"{min(gap for gap, _ in gaps):.1e}")
    assert worst <= TOL
    place = PC.placement_entropy if criterion == "entropy" else PC.placement_variance_reduction
    assert [int(a) for a in place(site, K.D5_K)] == [w.pick for w in ref]
    assert place(site, 0) == []


KEYS = ("delta", "s", "nom", "W", "U")


@pytest.mark.parametrize("name,cfg", X.CONFIGS, ids=["-".join(c) for c in X.CONFIGS])
def test_both_sides_generated(PC, name, cfg):
    """X1 and X2 through SiteKernel + CrossKernel.from_site against the longdouble rounds, and
    beside it the run with the same cross_kernel on the stored Sigma."""
    require_longdouble()
    S, site, gen = _cross_fixture(PC, name)
    om, cand = X.config(name, cfg)
    ref = X.reference(name, cfg)
    kw = dict(candidates=cand, cross_kernel=gen, target_weights=om)
    g = PC.CriterionPlacement(site, X.K_ROUNDS, "variance", **kw).init()
    dense = PC.CriterionPlacement(S, X.K_ROUNDS, "variance", **kw).init()
    smax = float(np.max(np.diag(X.fixture(name)[0])))
    worst = dict.fromkeys(KEYS, 0.0)
    apart = dict.fromkeys(KEYS, 0.0)
    for r, want in enumerate(ref):
        g.step()
        dense.step()
        st, sd = g.state(), dense.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        assert int(dense.selected[r]) == want.pick, r
        scale = float(want.pick_delta)
        err = {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
               "s": np.max(np.abs(_host(st["s"]) - want.s)) / scale,
               "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
               "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax,
               "U": np.max(np.abs(_host(st["U"][r]) - want.u)) / smax}
        for key, e in err.items():
            worst[key] = max(worst[key], float(e))
        assert abs(float(g.sel_delta[r]) - scale) <= TOL * scale, r
        for key in KEYS:
            a, b = (st[key][r], sd[key][r]) if key in ("W", "U") else (st[key], sd[key])
            rel = scale if key in ("delta", "s") else smax
            apart[key] = max(apart[key], float(np.max(np.abs(_host(a) - _host(b)))) / rel)
    print(f"both sides generated {name}-{cfg}: "
          + " ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + " | against the stored Sigma: " + " ".join(f"{k} {v:.1e}" for k, v in apart.items()))
    for key in KEYS:
        assert worst[key] <= TOL, (key, worst[key])
        assert apart[key] <= TOL, (key, apart[key])
    picks, _ = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert g.state()["U"].shape == (X.K_ROUNDS, gen.P)
    removed = np.sum(np.array([w.u for w in ref], dtype=np.float64) ** 2, axis=0)
    assert np.max(np.abs(_host(g.variance_removed()) - removed)) <= TOL * smax


GRID, MESH, KM = (8, 8, 8), (12, 12, 12), 8
AMP, NOISE, JITTER = 1.0, 1e-2, 1e-6


@pytest.mark.parametrize("criterion", ["variance", "entropy"])
def test_from_points_on_the_sites(PC, criterion):
    """An 8^3 grid: cov="matrix_free" returns the picks of cov="dense", and the deltas of the
    run on the SiteKernel it builds are those of the run on the assembled matrix to 1e-9."""
    from vgposp_amd import linalg
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_algorithm2 import placement_from_points
    Xs = grid_points(GRID, jitter=0.05, seed=0)
    ls = 2.0 * grid_spacing(GRID)
    dense = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, criterion=criterion)
    free = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, criterion=criterion,
                                 cov="matrix_free")
    assert [int(a) for a in free] == [int(a) for a in dense]
    assert all(isinstance(a, np.int64) for a in free) and len(set(int(a) for a in free)) == KM
    site = PC.SiteKernel("eq", Xs, AMP, ls, noise=NOISE + JITTER)
    Sigma = linalg.kernel_matrix("eq", Xs, None, AMP, ls, diag_shift=NOISE + JITTER)[0]
    picks, deltas = PC.CriterionPlacement(site, KM, criterion).run().result()
    dpicks, ddeltas = PC.CriterionPlacement(Sigma, KM, criterion).run().result()
    assert [int(a) for a in picks] == [int(a) for a in dpicks] == [int(a) for a in dense]
    np.testing.assert_allclose(deltas, ddeltas, rtol=TOL, atol=0)


def test_from_points_with_a_mesh_and_the_models_variance_reduction(PC):
    """An 8^3 site grid judged on a jittered 12^3 mesh with both sides generated: the picks of the
    dense run, deltas that sum to what GaussianProcessRegressionModel.variance says the sensors
    took off the prior variance of the mesh."""
    from vgposp_amd import distributions as tfd
    from vgposp_amd import psd_kernels as tfkern
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_algorithm2 import placement_from_points
    Xs = grid_points(GRID, jitter=0.05, seed=0)
    Xt = grid_points(MESH, jitter=0.3, seed=1)
    ls = 2.0 * grid_spacing(GRID)
    kw = dict(criterion="variance", target_points=Xt)
    dense = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, cross="dense", **kw)
    free = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, cov="matrix_free", **kw)
    assert [int(a) for a in free] == [int(a) for a in dense]
    both = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, cov="matrix_free",
                                 cross="matrix_free", **kw)
    assert [int(a) for a in both] == [int(a) for a in dense]
    site = PC.SiteKernel("eq", Xs, AMP, ls, noise=NOISE + JITTER)
    g = PC.CriterionPlacement(site, KM, "variance",
                              cross_kernel=PC.CrossKernel.from_site(site, Xt)).run()
    picks, deltas = g.result()
    picks = [int(a) for a in picks]
    assert picks == [int(a) for a in dense]
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=Xt,
        observation_index_points=Xs[picks], observations=np.zeros(KM),
        observation_noise_variance=NOISE, predictive_noise_variance=0.0, jitter=JITTER)
    prior = AMP * AMP
    removed = prior - gprm.variance().cpu().numpy()
    reduction, total = float(np.sum(removed)), float(np.sum(deltas))
    print(f"sum of deltas {total:.15g}, model's reduction {reduction:.15g}, relative difference "
          f"{abs(total - reduction) / reduction:.2e}")
    assert abs(total - reduction) <= 1e-9 * reduction
    got = g.variance_removed().cpu().numpy()
    assert got.shape == (len(Xt),) and np.max(np.abs(got - removed)) <= 1e-9 * prior


def test_argument_errors(PC):
    from vgposp_amd.data_generation import grid_points
    from vgposp_amd.placement_algorithm2 import placement_from_points
    S, site, gen = _cross_fixture(PC, "X2")
    n = site.N
    rng = np.random.default_rng(0)
    Xs, Xt = rng.random((20, 3)), rng.random((30, 3))
    with pytest.raises(ValueError, match="diag and a SiteKernel exclude each other"):
        PC.CriterionPlacement(site, 3, diag=np.ones(n))
    with pytest.raises(ValueError, match="cross_cov and a SiteKernel exclude each other"):
        PC.CriterionPlacement(site, 3, cross_cov=np.ones((5, n)))
    with pytest.raises(ValueError, match="cross_cov and a SiteKernel exclude each other"):
        PC.placement_variance_reduction(site, 3, cross_cov=np.ones((5, n)))
    with pytest.raises(ValueError, match=r"k must be in \[1, "):
        PC.CriterionPlacement(site, n + 1)
    with pytest.raises(ValueError, match="targets apply"):
        PC.CriterionPlacement(site, 3, "entropy", targets=[1, 2])
    with pytest.raises(ValueError, match="variance' only"):
        PC.CriterionPlacement(site, 3, "entropy", cross_kernel=gen)
    with pytest.raises(ValueError, match="outside"):
        PC.placement_entropy(site, 0, candidates=[n + 5])                # validated at k < 1 too
    # a cross_kernel that describes another field
    kind, Xf, Xtf, amp, ls, a_s, a_t = K.fixture_points("X2")
    other = [PC.CrossKernel("eq", Xf, Xtf, amp, ls, site_scale=a_s),           # kind
             PC.CrossKernel(kind, Xf, Xtf, 1.1 * amp, ls, site_scale=a_s),     # amp
             PC.CrossKernel(kind, Xf, Xtf, amp, 0.9 * ls, site_scale=a_s),     # ls
             PC.CrossKernel(kind, Xf + 1e-9, Xtf, amp, ls, site_scale=a_s),    # points
             PC.CrossKernel(kind, Xf, Xtf, amp, ls),                           # site scale
             PC.CrossKernel(kind, Xf, Xtf, amp, ls, site_scale=1.01 * a_s)]
    for bad in other:
        with pytest.raises(ValueError, match="must agree in kind, amp, ls, points and site scale"):
            PC.CriterionPlacement(site, 3, cross_kernel=bad)
    same = PC.CrossKernel(kind, Xf, Xtf, amp, ls, site_scale=a_s, target_scale=a_t)
    assert same.agrees_with(site) and gen.agrees_with(site)
    PC.CriterionPlacement(site, 3, cross_kernel=same)                     # an equal one is fine
    with pytest.raises(ValueError, match=f"cov_vv {n} locations"):
        PC.CriterionPlacement(site, 3, cross_kernel=PC.CrossKernel(kind, Xs, Xt, amp, ls))
    with pytest.raises(ValueError, match="from_site needs a placement_criteria.SiteKernel"):
        PC.CrossKernel.from_site(S, Xt)
    with pytest.raises(ValueError, match=r"target_points must be \[P, 3\]"):
        PC.CrossKernel.from_site(site, Xt[:, :2])
    with pytest.raises(ValueError, match="target_scale must have length 30"):
        PC.CrossKernel.from_site(site, Xt, target_scale=np.ones(20))
    # SiteKernel validates as CrossKernel does
    with pytest.raises(ValueError, match=r"points must be \[count, d\]"):
        PC.SiteKernel("eq", np.zeros((0, 3)), 1.0, 0.5)
    with pytest.raises(ValueError, match="1 <= d <= 8"):
        PC.SiteKernel("eq", np.zeros((4, 9)), 1.0, 0.5)
    with pytest.raises(ValueError, match="unknown kernel kind"):
        PC.SiteKernel("cubic", Xs, 1.0, 0.5)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="ls must be a finite, positive scalar"):
            PC.SiteKernel("eq", Xs, 1.0, bad)
        with pytest.raises(ValueError, match="amp must be a finite, positive scalar"):
            PC.SiteKernel("eq", Xs, bad, 0.5)
        a = np.ones(20)
        a[3] = bad
        with pytest.raises(ValueError, match="scale must be finite and positive"):
            PC.SiteKernel("eq", Xs, 1.0, 0.5, scale=a)
    with pytest.raises(ValueError, match="scale must have length 20"):
        PC.SiteKernel("eq", Xs, 1.0, 0.5, scale=np.ones(19))
    for bad in (-1e-3, np.nan, np.inf):
        with pytest.raises(ValueError, match="noise must be finite and not negative"):
            PC.SiteKernel("eq", Xs, 1.0, 0.5, noise=bad)
    with pytest.raises(ValueError, match="noise must have length 20"):
        PC.SiteKernel("eq", Xs, 1.0, 0.5, noise=np.ones(3))
    sk = PC.SiteKernel("eq", Xs[:, 0], 1.5, 0.5, noise=np.full(20, 0.25))   # 1-D points, [N] noise
    assert (sk.N, sk.d) == (20, 1) and len(sk.args()) == 8
    np.testing.assert_allclose(sk.diag.cpu().numpy(), 2.5)
    # placement_from_points
    Gs = grid_points((4, 4, 4), jitter=0.05, seed=0)
    Gt = grid_points((5, 5, 5), jitter=0.05, seed=1)
    with pytest.raises(ValueError, match="unknown cov"):
        placement_from_points(Gs, 3, criterion="variance", cov="sparse")
    with pytest.raises(ValueError, match="mutual-information placement factors Sigma"):
        placement_from_points(Gs, 3, cov="matrix_free")
    with pytest.raises(ValueError, match="cov='matrix_free' and cross='dense' exclude"):
        placement_from_points(Gs, 3, criterion="variance", target_points=Gt, cross="dense",
                              cov="matrix_free")
    with pytest.raises(ValueError, match="target_points apply"):
        placement_from_points(Gs, 3, criterion="entropy", target_points=Gt, cov="matrix_free")
    with pytest.raises(ValueError, match="cross needs target_points"):
        placement_from_points(Gs, 3, criterion="variance", cross="matrix_free", cov="matrix_free")


def test_example_rows_show_the_same_picks(monkeypatch, capsys):
    """examples/points_only_placement.py: the dense and the matrix-free row list the same picks
    (its main(), in this process)."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "examples"))
    import points_only_placement

    def rows(*flags):
        monkeypatch.setattr(sys, "argv", ["points_only_placement.py", "--sites", "5", "5", "5",
                                          "--k", "4", *flags])
        points_only_placement.main()
        out = capsys.readouterr().out
        got = [line for line in out.splitlines() if line.startswith(("dense", "matrix-free"))]
        assert len(got) == 2 and got[0].startswith("dense"), out
        return [line[line.index("["):] for line in got]
    for flags in ((), ("--criterion", "entropy"), ("--mesh", "8", "8", "8")):
        a, b = rows(*flags)
        assert a == b and a.count(",") == 3, (flags, a, b)
