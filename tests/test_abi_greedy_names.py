"""Argument validation of every vgposp_greedy_* entry of greedy.hip, without a GPU: a bad argument
is reported under the entry's own name and at its position in the entry's own prototype (fake
pointers, a workspace size that passes the workspace check), and a workspace that is too small is
reported before any device work.

How an entry answers a null `ws` or `info` (by position, or "workspace is null" with VGPOSP_E_WS /
"info is null") is a record of commit 3d30fed, as is every position except the ones that commit
reported under another entry's name or position: n, kmax, round of _select, _select_window and
_force (2, 4, 5 there), the name of _init_ex (vgposp_greedy_init there), name and positions of
_init_slab (those of _prepare / _finish_slab), of _update (those of _update_ex) and of _step at
round 0 (those of _update_ex / _select)."""
import ctypes

import pytest

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced
BIG = 1 << 44
NBIG = (1 << 21) + 1             # above the 2048 chunks of 1024 candidates

MAT = dict(Sigma=P8, n=10, lda=10, kmax=3)
SIZES = dict(n=10, kmax=3, round=1)
INIT = dict(jitter=0.0, threshold=1e-8, cache_init=float("inf"))
PICKS = dict(selected=P8, sel_delta=None, evals=None)
WS = dict(ws=P8, ws_bytes=BIG, stream=None)
VIEW = dict(ws=P8, n=10, kmax=3)
SLAB = dict(c0=0, c1=10, tmp=P8, tmp_bytes=BIG)

# (the bad arguments, the argument that is reported); a null ws / info comes per entry below
BAD_MAT = [(dict(Sigma=None), "Sigma"), (dict(n=0), "n"), (dict(n=NBIG, lda=NBIG), "n"),
           (dict(lda=9), "lda"), (dict(kmax=0), "kmax"), (dict(kmax=11), "kmax")]
BAD_SIZES = [(dict(n=0), "n"), (dict(n=NBIG), "n"), (dict(kmax=0), "kmax"), (dict(kmax=11), "kmax"),
             (dict(round=-1), "round"), (dict(round=3), "round")]
BAD_ROUND = [(dict(round=-1), "round"), (dict(round=3), "round")]
BAD_INIT = [(dict(jitter=-1.0), "jitter"), (dict(jitter=1e301), "jitter"),
            (dict(threshold=-1.0), "threshold"), (dict(cache_init=float("nan")), "cache_init")]
BAD_RANGE = [(dict(c0=-1), "c0"), (dict(c0=5, c1=4), "c0"), (dict(c1=11), "c0")]
BAD_SLAB = [(dict(c0=-128), "c0"), (dict(c0=1), "c0"), (dict(c1=11), "c1"), (dict(c1=5), "c1"),
            (dict(tmp=None), "tmp")]
BAD_VIEW = [(dict(ws=None), "ws"), (dict(n=0), "n"), (dict(kmax=0), "kmax")]
WS_BY_POSITION, WS_BY_NAME = [(dict(ws=None), "ws")], [(dict(ws=None), "workspace is null")]
INFO_BY_POSITION, INFO_BY_NAME = [(dict(info=None), "info")], [(dict(info=None), "info is null")]

# entry -> (its valid arguments in ABI order, its bad ones)
ENTRIES = {
    "vgposp_greedy_init": (
        dict(MAT, info=P8, **WS), BAD_MAT + INFO_BY_POSITION + WS_BY_POSITION),
    "vgposp_greedy_init_ex": (
        dict(MAT, **INIT, info=P8, **WS), BAD_MAT + BAD_INIT + INFO_BY_POSITION + WS_BY_POSITION),
    "vgposp_greedy_prepare": (
        dict(MAT, **INIT, info=P8, **WS), BAD_MAT + BAD_INIT + INFO_BY_NAME + WS_BY_NAME),
    "vgposp_greedy_init_slab": (
        dict(MAT, **INIT, **SLAB, info=P8, **WS),
        BAD_MAT + BAD_INIT + BAD_SLAB + INFO_BY_NAME + WS_BY_NAME),
    "vgposp_greedy_finish_slab": (
        dict(MAT, **SLAB, **WS), BAD_MAT + BAD_SLAB + WS_BY_POSITION),
    "vgposp_greedy_step": (
        dict(MAT, round=1, lazy=1, **PICKS, **WS),
        BAD_MAT + BAD_ROUND + [(dict(selected=None), "selected")] + WS_BY_NAME
        # round 0 has no mat-vec, so no speculation either
        + [(dict(round=0, Sigma=None), "Sigma"), (dict(round=0, n=0), "n"),
           (dict(round=0, lda=9), "lda"), (dict(round=0, kmax=11), "kmax"),
           (dict(round=0, ws=None), "workspace is null")]),
    "vgposp_greedy_update": (
        dict(MAT, round=1, c0=0, c1=10, selected=P8, **WS),
        BAD_MAT + BAD_ROUND + BAD_RANGE + [(dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_update_ex": (
        dict(MAT, round=1, c0=0, c1=10, selected=P8, extract=1, **WS),
        BAD_MAT + BAD_ROUND + BAD_RANGE + [(dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_extract": (
        dict(MAT, round=1, own0=0, own1=10, selected=P8, **WS),
        BAD_MAT + BAD_ROUND + [(dict(round=0), "round"), (dict(own0=-1), "own0"),
                               (dict(own0=5, own1=4), "own0"), (dict(own1=11), "own0"),
                               (dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_select": (
        dict(SIZES, lazy=1, c0=0, c1=10, **PICKS, **WS),
        BAD_SIZES + BAD_RANGE + [(dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_select_window": (
        dict(SIZES, I0=5, I1=2, I2=1, cutoff=1, c0=0, c1=10, **PICKS, **WS),
        BAD_SIZES + BAD_RANGE + [(dict(I0=0), "I0"), (dict(I2=2), "I0"), (dict(cutoff=-1), "cutoff"),
                                 (dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_force": (
        dict(SIZES, forced=P8, j=0, selected=P8, **WS),
        BAD_SIZES + [(dict(forced=None), "forced"), (dict(j=-1), "j"),
                     (dict(selected=None), "selected")] + WS_BY_NAME),
    "vgposp_greedy_condition": (
        dict(MAT, m=2, k=1, batch=4, placed=P8, selected=P8, ws=P8, ws_bytes=BIG, scratch=P8,
             scratch_bytes=BIG, stream=None),
        BAD_MAT + [(dict(m=0), "m"), (dict(m=4), "m"), (dict(k=-1), "k"), (dict(k=2), "k"),
                   (dict(batch=0), "batch"), (dict(batch=3), "batch"), (dict(placed=None), "placed"),
                   (dict(selected=None), "selected"), (dict(scratch=None), "scratch"),
                   (dict(scratch_bytes=16), "scratch 16 <")] + WS_BY_NAME),
    "vgposp_greedy_mask": (
        dict(VIEW, allowed=P8, stream=None),
        BAD_VIEW + [(dict(n=NBIG), "n"), (dict(kmax=11), "kmax"), (dict(allowed=None), "allowed")]),
    "vgposp_greedy_exclude": (
        dict(VIEW, idx=0, stream=None), BAD_VIEW + [(dict(idx=-1), "idx"), (dict(idx=10), "idx")]),
    "vgposp_greedy_cache": (dict(VIEW, cache=P8), BAD_VIEW + [(dict(cache=None), "cache")]),
    "vgposp_greedy_xcol": (dict(VIEW, xcol=P8), BAD_VIEW + [(dict(xcol=None), "xcol")]),
    "vgposp_greedy_fact_ws": (
        dict(VIEW, fws=P8, fws_bytes=P8),
        BAD_VIEW + [(dict(fws=None), "fws"), (dict(fws_bytes=None), "fws")]),
    "vgposp_greedy_buffers": (dict(VIEW, delta=None, piv=None, piv_len=None), BAD_VIEW),
    "vgposp_greedy_spec_table": (dict(VIEW, column=None, fill_round=None, slots=None), BAD_VIEW),
    # never called with valid arguments: it copies from the device
    "vgposp_greedy_spec_stats": (dict(VIEW, passes=None, hits=None, cached=None), BAD_VIEW),
    "vgposp_greedy_set_speculation": (
        dict(width=8), [(dict(width=0), "width"), (dict(width=3), "width"),
                        (dict(width=16), "width")]),
}
NOT_TABLED = {"vgposp_greedy_workspace_bytes", "vgposp_greedy_condition_workspace_bytes",
              "vgposp_greedy_slab_tmp_bytes", "vgposp_greedy_speculation"}


def _cases():
    for entry, (args, cases) in ENTRIES.items():
        for bad, what in cases:
            yield pytest.param(entry, args, bad, what,
                               id=f"{entry}-{'-'.join(f'{k}={v}' for k, v in bad.items())}"
                               .replace("c_void_p(8)", "ptr"))


def _args(entry, args):
    """Typed for the pointer-to-pointer outputs of the query entries."""
    types = _lib.SIGNATURES[entry][1]
    assert len(args) == len(types), entry
    return [ctypes.cast(v, t) if v is P8 and t is not ctypes.c_void_p else v
            for v, t in zip(args.values(), types)]


@pytest.mark.parametrize("entry,args,bad,what", _cases())
def test_bad_argument(entry, args, bad, what):
    assert set(bad) <= set(args), bad
    rc = getattr(_lib.load(), entry)(*_args(entry, dict(args, **bad)))
    err = _lib.last_error()
    if what in args:                        # by position
        number = list(args).index(what) + 1
        assert rc == -number, (rc, err)
        assert err.startswith(f"{entry}: bad argument {number}"), err
        assert not err[len(f"{entry}: bad argument {number}"):][:1].isdigit(), err
    elif what == "info is null":
        assert rc == -(list(args).index("info") + 1), (rc, err)
        assert err.startswith(f"{entry}: info is null"), err
    else:                                   # "workspace is null", "scratch 16 <"
        assert rc == _lib.E_WS, (rc, err)
        assert err.startswith(f"{entry}: {what}"), err


@pytest.mark.parametrize("entry", [e for e, (args, _) in ENTRIES.items() if "ws_bytes" in args])
def test_checks_precede_device_work(entry):
    """The valid arguments pass every check up to the workspace size."""
    args = ENTRIES[entry][0]
    assert getattr(_lib.load(), entry)(*_args(entry, dict(args, ws_bytes=16))) == _lib.E_WS
    assert _lib.last_error().startswith(f"{entry}: workspace 16 <"), _lib.last_error()


def test_set_speculation_keeps_the_width():
    lib = _lib.load()
    old = lib.vgposp_greedy_speculation()
    for bad, _ in ENTRIES["vgposp_greedy_set_speculation"][1]:
        assert lib.vgposp_greedy_set_speculation(bad["width"]) == -1
    assert lib.vgposp_greedy_speculation() == old


def test_every_entry_is_covered():
    greedy = {s for s in _lib.SIGNATURES if s.startswith("vgposp_greedy_")}
    assert greedy == set(ENTRIES) | NOT_TABLED
    assert not set(ENTRIES) & NOT_TABLED
    for entry, (args, cases) in ENTRIES.items():
        res, types = _lib.SIGNATURES[entry]
        assert res is ctypes.c_int and len(args) == len(types), entry
        reported = {what for _, what in cases if what in args}
        # every argument an entry checks is tried
        assert reported, entry
    for entry in NOT_TABLED - {"vgposp_greedy_speculation"}:
        assert _lib.SIGNATURES[entry][0] is ctypes.c_size_t, entry
