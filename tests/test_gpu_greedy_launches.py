"""GPU: the launch sequence of every caller of csrc/greedy.hip.  Each case runs under the
library's profiler; the scopes recorded, how often each was entered and the bytes its model counts
are compared with a table.  Every scope counts, those of the factorization too: that pins the
early-exit form and the inverse of vgposp_greedy_init_ex, and the classical (no Strassen), not
inverting factorization of vgposp_greedy_init_slab.

n = 1040 (F1 of tests/greedy_state_reference.py) is two CH = 1024 candidate chunks with a ragged
second one and three RC / TRMV_COLS = 512 tiles; kmax = 4.  The table was recorded on the MI355X
on commit 3d30fed ("Criteria placement: single-source the rounds, checks and dispatch"), before
the host side of greedy.hip was single-sourced; it is a record of that commit, not derived from
the code under test."""
import pytest

from tests import greedy_state_reference as R

pytestmark = pytest.mark.gpu

N, KMAX = 1040, 4
COVER, CUTOFF = (13, 10, 8), 2
PLACED = R.PLACED[:3]
SLAB = (512, 1040)

# case -> {scope: (times entered, bytes of its model)}
_GEMM = {"gemm_f64[nt,narrow]": (16, 15520260.0), "gemm_f64[nt,triB,narrow]": (2, 8060928.0),
         "potrf_diag": (9, 2101248.0)}
# vgposp_greedy_init_ex: the factorization with the inverse, the column norms of all of L^-1
_INIT = dict(_GEMM, **{"gemm_f64[nn,triA,narrow]": (8, 11509760.0),
                       "gemm_f64[nn,triB,narrow]": (8, 11403260.0),
                       "trtri_leaf": (9, 2359296.0), "greedy_colsq": (1, 4355520.0)})
# two rounds: 8 n (6 + 2 round) per update; the refresh reads 24 n
_TWO = dict(_INIT, greedy_update=(2, 116480.0), greedy_select=(2, 0.0))
TABLE = {
    "lazy-width8": dict(_TWO, greedy_refresh=(2, 49920.0), greedy_trmv_spec=(1, 4397120.0)),
    "lazy-width1": dict(_TWO, greedy_refresh=(2, 49920.0), greedy_trmv=(1, 4347200.0)),
    "full": dict(_TWO, greedy_trmv_spec=(1, 4397120.0)),
    "condition-batch1": dict(_INIT, greedy_update=(3, 199680.0), greedy_trmv=(2, 8694400.0)),
    "condition-batch4": dict(_INIT, greedy_update=(3, 199680.0),
                             greedy_trmv_batch=(1, 4363840.0)),
    "window": dict(_TWO, greedy_window=(2, 0.0), greedy_trmv=(1, 4347200.0)),
    # vgposp_greedy_init_slab: the factorization alone, then the inverse of the slab's columns;
    # a slab's column norms report no bytes
    "slab": dict(_GEMM, **{"gemm_f64[nn,triA,narrow]": (10, 5842944.0),
                           "gemm_f64[nn,triB,narrow]": (10, 5963776.0),
                           "trtri_leaf": (14, 3670016.0), "greedy_colsq": (1, 0.0),
                           "greedy_update": (2, 59136.0), "greedy_select": (2, 0.0),
                           "greedy_refresh": (2, 49920.0), "greedy_trmv": (1, 4347200.0)}),
}


def _two_steps(g, lazy):
    g.init()
    g.step(lazy)
    g.step(lazy)
    return g


def _lazy(K, width):
    from vgposp_amd import _lib
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    old = _lib.load().vgposp_greedy_speculation()
    _lib.call("vgposp_greedy_set_speculation", width)
    try:
        return _two_steps(GreedyPlacement(K, KMAX, copy=True), True)
    finally:
        _lib.call("vgposp_greedy_set_speculation", old)


def _full(K):
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    return _two_steps(GreedyPlacement(K, KMAX, copy=True), False)


def _condition(K, batch):
    from vgposp_amd.placement_algorithm2 import GreedyPlacement
    g = GreedyPlacement(K, KMAX - len(PLACED), copy=True, placed=PLACED, condition_batch=batch)
    assert g.kmax == KMAX
    return g.init()


def _window(K):
    from vgposp_amd.snippets_a3 import WindowGreedy
    g = WindowGreedy(K, KMAX, COVER, CUTOFF, copy=True).init()
    g.step()
    g.step()
    return g


def _slab(K):
    """One rank's rounds 0 and 1 of the partitioned sharded placement on its slab; the deltas of
    the other slab (another rank's, all-gathered there) are zero."""
    from vgposp_amd.sharded_placement import HipGreedyBackend
    b = HipGreedyBackend(K, KMAX, copy=True)
    c0, c1 = SLAB
    b.init_slab(c0, c1)
    b.delta()[:c0].zero_()
    b.update(0, c0, c1)
    b.select(0, True, c0, c1)
    b.extract(1, c0, c1)
    b.update(1, c0, c1, extract=False)
    b.select(1, True, c0, c1)
    return b.g


CASES = {
    "lazy-width8": lambda K: _lazy(K, 8),
    "lazy-width1": lambda K: _lazy(K, 1),
    "full": _full,
    "condition-batch1": lambda K: _condition(K, 1),
    "condition-batch4": lambda K: _condition(K, 4),
    "window": _window,
    "slab": _slab,
}


def recorded(case, K):
    """{scope: (times entered, bytes)} of a case, and the picks it made."""
    import torch

    from vgposp_amd import _lib
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        g = CASES[case](K)
        torch.cuda.synchronize()
        dump = _lib.prof_dump()
    finally:
        _lib.prof_enable(False)
    g.check()
    return {name: (v[1], v[3]) for name, v in dump.items()}, [int(a) for a in g.selected]


@pytest.fixture(scope="module")
def cov():
    import torch
    torch.cuda.set_device(0)
    K = torch.as_tensor(R.fixture_cov("F1")).cuda()
    assert K.shape == (N, N)
    return K


@pytest.mark.parametrize("case", list(CASES))
def test_launch_table(cov, case):
    got, picks = recorded(case, cov)
    rounds = len(PLACED) if case.startswith("condition") else 2
    assert len(set(picks[:rounds])) == rounds and min(picks[:rounds]) >= 0, picks
    if case.startswith("condition"):
        assert picks[:rounds] == PLACED
    if case == "slab":
        assert all(SLAB[0] <= y < SLAB[1] for y in picks[:rounds]), picks
    want = TABLE[case]
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name, (count, nbytes) in want.items():
        assert got[name][0] == count, (name, got[name], count)
        assert got[name][1] == pytest.approx(nbytes, rel=1e-6), (name, got[name], nbytes)
