"""GPU: variance-reduction placement on a cross-covariance that is never stored (the vgposp_critk_*
entries through placement_criteria.CriterionPlacement(cross_kernel=...)) against the longdouble
references of tests/numpy_cross_criteria.py, used as they are: the fixtures' R is fed as points,
kernel, length scale and amplitude field (tests/numpy_kernel_cross.py shows on the CPU that these
generate that R to 1e-13).

Tolerance 1e-9 (the project's tolerance for deltas): delta and s relative to the round's pick
delta, nom and the new rows of W and U relative to max diag Sigma.  With 512-target chunks X1
(P = 1,680) spans four chunks and X2 (P = 1,287) three, both with a ragged tail."""
import os
import sys

import numpy as np
import pytest

from tests import numpy_cross_criteria as X
from tests import numpy_kernel_cross as K
from tests.greedy_state_reference import require_longdouble

pytestmark = pytest.mark.gpu
TOL = X.STATE_TOL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("delta", "s", "nom", "W", "U")


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
    """(Sigma, R, CrossKernel) on the device, uploaded once and never written."""
    import torch
    if name not in _dev:
        kind, Xs, Xt, amp, ls, a_s, a_t = K.fixture_points(name)
        S, R = (torch.tensor(M, device="cuda") for M in X.fixture(name))
        _dev[name] = S, R, PC.CrossKernel(kind, Xs, Xt, amp, ls, site_scale=a_s, target_scale=a_t)
    return _dev[name]


def _host(t):
    return t.cpu().numpy().copy()


def _errors(st, r, want, smax):
    scale = float(want.pick_delta)
    return {"delta": np.max(np.abs(_host(st["delta"]) - want.delta)) / scale,
            "s": np.max(np.abs(_host(st["s"]) - want.s)) / scale,
            "nom": np.max(np.abs(_host(st["nom"]) - want.nom)) / smax,
            "W": np.max(np.abs(_host(st["W"][r]) - want.w)) / smax,
            "U": np.max(np.abs(_host(st["U"][r]) - want.u)) / smax}


@pytest.mark.parametrize("name,cfg", X.CONFIGS, ids=["-".join(c) for c in X.CONFIGS])
def test_picks_and_state(PC, name, cfg):
    """Every round of the reference: the pick, then the whole state; beside it the dense path on
    the fixture's stored R, whose picks are the same and whose state lies within 1e-9 too."""
    require_longdouble()
    S, R, gen = _fixture(PC, name)
    before = _host(S), _host(gen.X), _host(gen.Xt)
    om, cand = X.config(name, cfg)
    ref = X.reference(name, cfg)
    g = PC.CriterionPlacement(S, X.K_ROUNDS, "variance", candidates=cand, cross_kernel=gen,
                              target_weights=om).init()
    dense = PC.CriterionPlacement(S, X.K_ROUNDS, "variance", candidates=cand, cross_cov=R,
                                  target_weights=om).init()
    smax = float(np.max(np.diag(before[0])))
    worst = dict.fromkeys(KEYS, 0.0)
    apart = dict.fromkeys(KEYS, 0.0)
    for r, want in enumerate(ref):
        g.step()
        dense.step()
        st, sd = g.state(), dense.state()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        assert int(dense.selected[r]) == want.pick, r
        for key, e in _errors(st, r, want, smax).items():
            worst[key] = max(worst[key], float(e))
        scale = float(want.pick_delta)
        assert abs(float(g.sel_delta[r]) - scale) <= TOL * scale, r
        for key in KEYS:
            a, b = (st[key][r], sd[key][r]) if key in ("W", "U") else (st[key], sd[key])
            rel = scale if key in ("delta", "s") else smax
            apart[key] = max(apart[key], float(np.max(np.abs(_host(a) - _host(b)))) / rel)
    print(f"matrix-free criteria {name}-{cfg}: "
          + " ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + " | against dense: " + " ".join(f"{k} {v:.1e}" for k, v in apart.items()))
    for key in KEYS:
        assert worst[key] <= TOL, (key, worst[key])
        assert apart[key] <= TOL, (key, apart[key])
    picks, deltas = g.result()
    assert [int(p) for p in picks] == [w.pick for w in ref]
    assert all(isinstance(p, np.int64) for p in picks) and deltas.shape == (X.K_ROUNDS,)
    if cand is not None:
        assert cand[picks].all()
    st = g.state()
    assert st["U"].shape == (X.K_ROUNDS, gen.P) and st["W"].shape == (X.K_ROUNDS, S.shape[0])
    removed = np.sum(np.array([w.u for w in ref], dtype=np.float64) ** 2, axis=0)
    assert np.max(np.abs(_host(g.variance_removed()) - removed)) <= TOL * smax
    assert _host(S).tobytes() == before[0].tobytes()          # Sigma and the points are only read
    assert _host(gen.X).tobytes() == before[1].tobytes()
    assert _host(gen.Xt).tobytes() == before[2].tobytes()


def test_placed_continues_a_free_run(PC):
    S, _, gen = _fixture(PC, "X1")
    om, cand = X.config("X1", "weighted")
    kw = dict(candidates=cand, cross_kernel=gen, target_weights=om)
    picks, deltas = PC.CriterionPlacement(S, 8, "variance", **kw).run().result()
    assert [int(p) for p in picks] == [w.pick for w in X.reference("X1", "weighted")[:8]]
    g = PC.CriterionPlacement(S, 4, "variance", placed=picks[:4], **kw).run()
    more, dmore = g.result()
    assert [int(p) for p in more] == [int(p) for p in picks[4:]]
    np.testing.assert_allclose(dmore, deltas[4:], rtol=TOL, atol=0)
    assert g.state()["U"].shape == (8, gen.P)


def test_two_runs_are_bit_identical(PC):
    S, _, gen = _fixture(PC, "X2")
    a = PC.CriterionPlacement(S, 6, "variance", cross_kernel=gen).run()
    b = PC.CriterionPlacement(S, 6, "variance", cross_kernel=gen).run()
    assert _host(a.sel_delta).tobytes() == _host(b.sel_delta).tobytes()
    for key in ("nom", "s", "delta", "W", "U"):
        assert _host(a.state()[key]).tobytes() == _host(b.state()[key]).tobytes(), key


def test_five_dimensional_case(PC):
    """3^5 sites, 4^5 jittered targets, Matern 3/2, no amplitude field: the run-time-dimension form
    of the pass.  (The >= 1e-6 gap of its rounds: tests/test_kernel_cross_reference.py.)"""
    require_longdouble()
    (Xs, Xt, ls, S, _), ref = K.d5_reference()
    gen = PC.CrossKernel(K.D5_KIND, Xs, Xt, K.D5_AMP, ls)
    g = PC.CriterionPlacement(S, K.D5_K, "variance", cross_kernel=gen).init()
    smax = float(np.max(np.diag(S)))
    worst = dict.fromkeys(KEYS, 0.0)
    for r, want in enumerate(ref):
        g.step()
        assert int(g.selected[r]) == want.pick, (r, int(g.selected[r]), want.pick)
        for key, e in _errors(g.state(), r, want, smax).items():
            worst[key] = max(worst[key], float(e))
    print("matrix-free criteria 5-D: " + " ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for key, v in worst.items():
        assert v <= TOL, (key, v)
    got = PC.placement_variance_reduction(S, K.D5_K, cross_kernel=gen)
    assert [int(a) for a in got] == [w.pick for w in ref]
    assert PC.placement_variance_reduction(S, 0, cross_kernel=gen) == []


GRID, MESH, KM = (8, 8, 8), (12, 12, 12), 8
AMP, NOISE, JITTER = 1.0, 1e-2, 1e-6


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_from_points_and_the_models_variance_reduction(PC, weighted):
    """An 8^3 site grid judged on a jittered 12^3 mesh: the picks of cross="dense", deltas that sum
    to what GaussianProcessRegressionModel.variance says the sensors took off the weighted prior
    variance, and variance_removed() that difference target by target."""
    from vgposp_amd import distributions as tfd
    from vgposp_amd import linalg
    from vgposp_amd import psd_kernels as tfkern
    from vgposp_amd.data_generation import grid_points, grid_spacing
    from vgposp_amd.placement_algorithm2 import placement_from_points
    Xs = grid_points(GRID, jitter=0.05, seed=0)
    Xt = grid_points(MESH, jitter=0.3, seed=1)
    ls = 2.0 * grid_spacing(GRID)
    rng = np.random.default_rng(3)
    om = rng.uniform(0.5, 2.0, len(Xt))
    om[rng.random(len(Xt)) < 0.1] = 0.0
    om = om if weighted else None
    kw = dict(criterion="variance", target_points=Xt, target_weights=om)
    dense = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, cross="dense", **kw)
    free = placement_from_points(Xs, KM, "eq", AMP, ls, NOISE, JITTER, cross="matrix_free", **kw)
    assert [int(a) for a in free] == [int(a) for a in dense]
    assert all(isinstance(a, np.int64) for a in free) and len(set(int(a) for a in free)) == KM
    Sigma = linalg.kernel_matrix("eq", Xs, None, AMP, ls, diag_shift=NOISE + JITTER)[0]
    g = PC.CriterionPlacement(Sigma, KM, "variance", target_weights=om,
                              cross_kernel=PC.CrossKernel("eq", Xs, Xt, AMP, ls)).run()
    picks, deltas = g.result()
    picks = [int(a) for a in picks]
    assert picks == [int(a) for a in dense]
    gprm = tfd.GaussianProcessRegressionModel(
        tfkern.ExponentiatedQuadratic(AMP, ls), index_points=Xt,
        observation_index_points=Xs[picks], observations=np.zeros(KM),
        observation_noise_variance=NOISE, predictive_noise_variance=0.0, jitter=JITTER)
    prior = AMP * AMP
    removed = prior - gprm.variance().cpu().numpy()
    reduction = float(np.sum(removed) if om is None else om @ removed)
    total = float(np.sum(deltas))
    print(f"sum of deltas {total:.15g}, model's reduction {reduction:.15g}, "
          f"relative difference {abs(total - reduction) / reduction:.2e}")
    assert abs(total - reduction) <= 1e-9 * reduction
    got = g.variance_removed().cpu().numpy()
    print(f"variance_removed: worst difference {np.max(np.abs(got - removed)) / prior:.2e} of "
          "the prior")
    assert got.shape == (len(Xt),) and np.max(np.abs(got - removed)) <= 1e-9 * prior


def test_argument_errors(PC):
    from vgposp_amd.data_generation import grid_points
    from vgposp_amd.placement_algorithm2 import placement_from_points
    S, R, gen = _fixture(PC, "X2")
    n, P = S.shape[0], gen.P
    with pytest.raises(ValueError, match="cross_kernel and cross_cov exclude each other"):
        PC.CriterionPlacement(S, 3, cross_kernel=gen, cross_cov=R)
    with pytest.raises(ValueError, match="cross_kernel and targets exclude each other"):
        PC.CriterionPlacement(S, 3, cross_kernel=gen, targets=[1, 2])
    with pytest.raises(ValueError, match="variance' only"):
        PC.CriterionPlacement(S, 3, "entropy", cross_kernel=gen)
    with pytest.raises(ValueError, match="must be a placement_criteria.CrossKernel"):
        PC.CriterionPlacement(S, 3, cross_kernel=R)
    with pytest.raises(ValueError, match="exclude each other"):
        PC.placement_variance_reduction(S, 0, cross_kernel=gen, cross_cov=R)   # at k < 1 too
    with pytest.raises(ValueError, match=f"target_weights must have length {P}"):
        PC.CriterionPlacement(S, 3, cross_kernel=gen, target_weights=np.ones(P - 1))
    w = np.ones(P)
    w[17] = -1.0
    with pytest.raises(ValueError, match="finite and not negative"):
        PC.CriterionPlacement(S, 3, cross_kernel=gen, target_weights=w)
    with pytest.raises(ValueError, match=f"cov_vv {n - 1} locations"):
        PC.CriterionPlacement(S[:n - 1, :n - 1], 3, cross_kernel=gen)
    Xs, Xt = np.random.default_rng(0).random((20, 3)), np.random.default_rng(1).random((30, 3))
    with pytest.raises(ValueError, match=r"target_points must be \[P, 3\]"):
        PC.CrossKernel("eq", Xs, Xt[:, :2], 1.0, 0.5)
    with pytest.raises(ValueError, match="1 <= d <= 8"):
        PC.CrossKernel("eq", np.zeros((4, 9)), np.zeros((5, 9)), 1.0, 0.5)
    with pytest.raises(ValueError, match="unknown kernel kind"):
        PC.CrossKernel("cubic", Xs, Xt, 1.0, 0.5)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="ls must be a finite, positive scalar"):
            PC.CrossKernel("eq", Xs, Xt, 1.0, bad)
        with pytest.raises(ValueError, match="amp must be a finite, positive scalar"):
            PC.CrossKernel("eq", Xs, Xt, bad, 0.5)
        a = np.ones(20)
        a[3] = bad
        with pytest.raises(ValueError, match="site_scale must be finite and positive"):
            PC.CrossKernel("eq", Xs, Xt, 1.0, 0.5, site_scale=a)
    with pytest.raises(ValueError, match="target_scale must have length 30"):
        PC.CrossKernel("eq", Xs, Xt, 1.0, 0.5, target_scale=np.ones(20))
    with pytest.raises(ValueError, match="needs cross_cov"):
        PC.CriterionPlacement(S, 3).variance_removed()
    Gs = grid_points((4, 4, 4), jitter=0.05, seed=0)
    Gt = grid_points((5, 5, 5), jitter=0.05, seed=1)
    for cross in ("dense", "matrix_free"):
        with pytest.raises(ValueError, match="cross needs target_points"):
            placement_from_points(Gs, 3, criterion="variance", cross=cross)
    with pytest.raises(ValueError, match="unknown cross"):
        placement_from_points(Gs, 3, criterion="variance", target_points=Gt, cross="sparse")
    with pytest.raises(ValueError, match="target_points apply"):
        placement_from_points(Gs, 3, criterion="entropy", target_points=Gt, cross="matrix_free")


def test_example_with_the_flag_prints_the_same_picks(monkeypatch, capsys):
    """examples/mesh_targets.py --matrix-free: the table of the run without the flag, up to the
    timing and the variances' last digits (its main(), in this process)."""
    monkeypatch.syspath_prepend(os.path.join(ROOT, "examples"))
    import mesh_targets

    def picks(*flags):
        monkeypatch.setattr(sys, "argv", ["mesh_targets.py", "--sites", "5", "5", "5", "--mesh",
                                          "8", "8", "8", "--k", "4", *flags])
        mesh_targets.main()
        out = capsys.readouterr().out
        rows = [line for line in out.splitlines() if line.startswith(("mesh", "in-V"))]
        assert len(rows) == 2, out
        return [line[line.index("["):] for line in rows]
    assert picks("--matrix-free") == picks()
