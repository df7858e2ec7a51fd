"""Argument validation of the bounded-lazy entries of exact_greedy.hip, without a GPU: every bad
argument is reported under its own number before any device work (fake pointers, a workspace
size that passes the workspace check)."""
import ctypes

import pytest

from vgposp_amd import _lib

P = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced
WS_BYTES = 1 << 40

# the common leading arguments (1 .. 23): a 3 x 3 x 3 grid, m = 7, kmax = 1
COMMON = dict(kind=0, X=P, I0=3, I1=3, I2=3, amp=1.0, ls=1.0, diag_shift=0.01, jitter=1e-6,
              threshold=1e-7, offsets=P, m=7, tau=P, ntau=1, kmax=1, cutoff=1, radius=1,
              cg_iters=4, qdiag=P, cache=P, selected=P, ws=P, ws_bytes=WS_BYTES)
TABLES = dict(tab_off=P, tab_nb=P, tab_cnt=P, T=7, K=1, hi_scale=1.0, mu=0.0)

# entry -> its own trailing arguments (24 ..), in ABI order, all valid
ENTRIES = {
    "vgposp_exact_bounds": dict(TABLES, c0=0, c1=27, stream=None),
    "vgposp_exact_tighten_pending": dict(TABLES, picks=P, stream=None),
    "vgposp_exact_pretighten": dict(TABLES, M=64, stream=None),
    "vgposp_exact_steps": dict(round0=0, round1=1, k=1, batch=1, picks=P, pick_delta=P,
                               stream=None),
    "vgposp_exact_refine_pending": dict(batch=1, picks_in=P, cg_tol=0.0, stream=None),
}
TABLE_ENTRIES = ("vgposp_exact_bounds", "vgposp_exact_tighten_pending", "vgposp_exact_pretighten")
REG_ENTRIES = TABLE_ENTRIES[1:]   # the register bounds kernel only: the 7-point taper (m = 7)


def _rc(entry, **bad):
    """The status of `entry` with the valid arguments, except those given in `bad`."""
    args = dict(COMMON, **ENTRIES[entry])
    assert set(bad) <= set(args), bad
    args.update(bad)
    return getattr(_lib.load(), entry)(*args.values())


def _expect(entry, number, **bad):
    assert _rc(entry, **bad) == -number, (entry, bad)
    err = _lib.last_error()
    assert f"{entry}: bad argument {number} " in err, err


# the table checks the three entries share: (bad argument, its number)
TABLE_CASES = [
    (dict(T=0), 27), (dict(T=897), 27),
    (dict(K=0), 28), (dict(K=57), 28),
    (dict(hi_scale=0.5), 29),
    (dict(mu=-1.0), 30),
]


@pytest.mark.parametrize("entry", TABLE_ENTRIES)
@pytest.mark.parametrize("bad,number", TABLE_CASES)
def test_table_arguments(entry, bad, number):
    _expect(entry, number, **bad)


def test_table_pointers():
    # vgposp_exact_bounds numbers the three tables one by one ...
    _expect("vgposp_exact_bounds", 24, tab_off=None)
    _expect("vgposp_exact_bounds", 25, tab_nb=None)
    _expect("vgposp_exact_bounds", 26, tab_cnt=None)
    # ... the two LIST entries report any missing table as argument 24
    for entry in REG_ENTRIES:
        for name in ("tab_off", "tab_nb", "tab_cnt"):
            _expect(entry, 24, **{name: None})


def test_own_last_argument():
    _expect("vgposp_exact_bounds", 31, c0=-1)
    _expect("vgposp_exact_bounds", 31, c0=5, c1=4)
    _expect("vgposp_exact_bounds", 31, c1=28)
    _expect("vgposp_exact_tighten_pending", 31, picks=None)
    _expect("vgposp_exact_pretighten", 31, M=0)
    _expect("vgposp_exact_pretighten", 31, M=32769)


def test_seven_point_stencil_required():
    for entry in REG_ENTRIES:
        _expect(entry, 12, m=5)


@pytest.mark.parametrize("entry", TABLE_ENTRIES)
def test_grid_of_two_to_the_31_nodes(entry):
    _expect(entry, 3, I0=2048, I1=1024, I2=1024)


def test_bounds_single_node_stencil_needs_no_neighbour_table():
    # m = 1: no offsets, no neighbour table; an empty candidate range returns before any launch
    assert _rc("vgposp_exact_bounds", m=1, offsets=None, tab_nb=None, T=1, c0=0, c1=0) == 0
    assert _rc("vgposp_exact_bounds", m=1, offsets=None, tab_nb=None, T=1, c0=27, c1=27) == 0
    # ... and the later checks still run
    _expect("vgposp_exact_bounds", 28, m=1, offsets=None, tab_nb=None, T=1, K=0)


def test_steps_arguments():
    e = "vgposp_exact_steps"
    _expect(e, 24, round0=-1)
    _expect(e, 24, round0=1, round1=0)
    _expect(e, 24, round1=2)
    _expect(e, 26, k=0)
    _expect(e, 26, k=2)
    _expect(e, 27, batch=0)
    _expect(e, 27, batch=33)
    _expect(e, 28, picks=None)


def test_refine_pending_arguments():
    e = "vgposp_exact_refine_pending"
    _expect(e, 24, batch=0)
    _expect(e, 24, batch=33)
    _expect(e, 25, picks_in=None)
    _expect(e, 26, cg_tol=-1.0)
