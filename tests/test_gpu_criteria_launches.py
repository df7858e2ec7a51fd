"""GPU: the launch sequence of the criteria rounds, family by family.  init() with one placed
sensor (a forced round) and one free round run under the library's profiler; the scopes recorded,
how often each was entered and the bytes its model counts are compared with a table.

n = 600 is two 512-tiles with a ragged edge, P = 700 likewise on the target side, S = 5 samples,
d = 2.  The table was recorded on commit c83b583 ("Criteria placement from samples alone"), before
the host side of criteria.hip was single-sourced; it is a record of that commit, not derived from
the code under test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, P, S, D = 600, 700, 5, 2
AMP, LS, NOISE = 1.3, 0.3, 1e-2
PLACED = [7]
CASES = [("crit", "variance"), ("crit", "entropy"), ("critx", "variance"), ("critk", "variance"),
         ("critg", "variance"), ("critg", "entropy"), ("critgk", "variance"),
         ("critf", "variance"), ("critf", "entropy")]

# (family, criterion) -> {scope: (times entered, bytes of its model)}
_SEL = {"criteria_select": (2, 28800.0), "criteria_update": (2, 43200.0)}
_ROW = dict(_SEL, criteria_row=(2, 52800.0))       # 8 n (5 + round) per round
TABLE = {
    ("crit", "variance"): dict(_ROW, criteria_symv=(2, 2884800.0), criteria_symv_sq=(1, 1442400.0)),
    ("crit", "entropy"): dict(_ROW, criteria_symv=(2, 2884800.0)),
    # the u-row adds 8 P (4 + round) for a stored R, 8 P (4 + d + round) for a generated one
    ("critx", "variance"): dict(_SEL, criteria_row=(2, 103200.0), criteria_gemv_t=(2, 6720000.0),
                                criteria_gemv_t_sq=(1, 3360000.0)),
    ("critk", "variance"): dict(_SEL, criteria_row=(2, 125600.0), criteria_kgemv_t=(2, 62400.0),
                                criteria_kgemv_t_sq=(1, 31200.0)),
    ("critg", "variance"): dict(_ROW, criteria_ksymv=(2, 76800.0), criteria_ksymv_sq=(1, 38400.0)),
    ("critg", "entropy"): dict(_ROW, criteria_ksymv=(2, 76800.0)),
    ("critgk", "variance"): dict(_SEL, criteria_row=(2, 125600.0), criteria_kgemv_t=(2, 62400.0),
                                 criteria_kgemv_t_sq=(1, 31200.0)),
    ("critf", "variance"): dict(_ROW, criteria_fsymv=(2, 96000.0), criteria_fsymv_sq=(1, 120000.0),
                                gemm_f64=(2, 96400.0), row_sumsq=(1, 28800.0)),
    ("critf", "entropy"): dict(_ROW, criteria_fsymv=(2, 96000.0), row_sumsq=(1, 28800.0)),
}


def host_problem():
    """The points, the targets, Sigma, R and the factor on the host (float64)."""
    rng = np.random.default_rng(20261021)
    X, Xt = rng.uniform(0.0, 1.0, (N, D)), rng.uniform(0.0, 1.0, (P, D))
    F = rng.standard_normal((N, S)) / np.sqrt(S)

    def eq(A, B):
        d2 = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
        return AMP * AMP * np.exp(-0.5 * d2 / (LS * LS))
    return X, Xt, eq(X, X) + NOISE * np.eye(N), eq(Xt, X), F


def placement(PC, family, criterion, k=1, problem=None):
    """A CriterionPlacement of `family` on the problem above, k free rounds after PLACED."""
    X, Xt, Sigma, R, F = problem or host_problem()
    kw = dict(criterion=criterion, placed=PLACED)
    if family == "crit":
        return PC.CriterionPlacement(Sigma, k, **kw)
    if family == "critx":
        return PC.CriterionPlacement(Sigma, k, cross_cov=R, **kw)
    if family == "critk":
        return PC.CriterionPlacement(Sigma, k, cross_kernel=PC.CrossKernel("eq", X, Xt, AMP, LS),
                                     **kw)
    if family == "critf":
        return PC.CriterionPlacement(PC.FactoredCovariance(F, noise=NOISE), k, **kw)
    site = PC.SiteKernel("eq", X, AMP, LS, noise=NOISE)
    if family == "critg":
        return PC.CriterionPlacement(site, k, **kw)
    assert family == "critgk", family
    return PC.CriterionPlacement(site, k, cross_kernel=PC.CrossKernel.from_site(site, Xt), **kw)


def recorded(PC, family, criterion, problem=None):
    """{scope: (times entered, bytes)} of init() (one forced round) and one free round."""
    import torch

    from vgposp_amd import _lib
    g = placement(PC, family, criterion, problem=problem)
    assert g._family == "vgposp_" + family
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        g.init().step()
        torch.cuda.synchronize()
        dump = _lib.prof_dump()
    finally:
        _lib.prof_enable(False)
    assert int(g.selected[0]) == PLACED[0] and int(g.selected[1]) not in (-1, PLACED[0])
    return {name: (v[1], v[3]) for name, v in dump.items()}


@pytest.fixture(scope="module")
def problem():
    import torch
    torch.cuda.set_device(0)
    return host_problem()


@pytest.mark.parametrize("family,criterion", CASES, ids=["-".join(c) for c in CASES])
def test_launch_table(problem, family, criterion):
    from vgposp_amd import placement_criteria as PC
    got = recorded(PC, family, criterion, problem)
    want = TABLE[family, criterion]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, (count, nbytes) in want.items():
        assert got[name][0] == count, (name, got[name], count)
        assert got[name][1] == pytest.approx(nbytes, rel=1e-6), (name, got[name], nbytes)
