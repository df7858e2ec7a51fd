"""Argument validation of every criteria entry of criteria.hip, without a GPU: the six families'
_init / _step / _buffers entries and the ten pass entries report a bad argument under its own
position and under the entry's own name (fake pointers, a workspace size that passes the workspace
check), and the _buffers entries of every family put nom, score, delta, W (and U) where
vgposp_crit_buffers / vgposp_critx_buffers put them."""
import ctypes

import pytest

from vgposp_amd import _lib

P8 = ctypes.c_void_p(8)          # a non-null pointer that is never dereferenced
BIG = 1 << 44

# the argument groups, in ABI order, all valid
SIG = dict(Sigma=P8, n=10, lda=10, diag=None)
SGEN = dict(kind=0, X=P8, n=10, d=2, amp=P8, ls=P8, site_scale=None, diag=None)
KGEN = dict(kind=0, Xt=P8, P=12, X=P8, d=2, amp=P8, ls=P8, target_scale=None, site_scale=None)
SFAC = dict(F=P8, n=10, s=6, ldf=6, noise=None)
CROSS = dict(R=P8, P=12, ldr=10)
RULE = dict(kmax=3, criterion=0, threshold=1e-8, targets=None, allowed=None)
XRULE = dict(weights=None, kmax=3, threshold=1e-8, allowed=None)
ROUND = dict(kmax=3, round=0, forced=None, j=0, selected=P8, sel_delta=None)
WS = dict(ws=P8, ws_bytes=BIG, stream=None)
XY = dict(x=P8, y=P8)

# group -> [(the bad arguments, the argument that is reported)]
BAD = {
    "SIG": [(dict(Sigma=None), "Sigma"), (dict(n=0), "n"), (dict(n=(1 << 21) + 1), "n"),
            (dict(lda=9), "lda")],
    "SGEN": [(dict(kind=4), "kind"), (dict(kind=-1), "kind"), (dict(X=None), "X"),
             (dict(n=0), "n"), (dict(d=0), "d"), (dict(d=9), "d"), (dict(amp=None), "amp"),
             (dict(ls=None), "ls")],
    "KGEN": [(dict(kind=4), "kind"), (dict(kind=-1), "kind"), (dict(Xt=None), "Xt"),
             (dict(P=0), "P"), (dict(P=(1 << 24) + 1), "P"), (dict(X=None), "X"),
             (dict(d=0), "d"), (dict(d=9), "d"), (dict(amp=None), "amp"), (dict(ls=None), "ls")],
    "SFAC": [(dict(F=None), "F"), (dict(n=0), "n"), (dict(s=0, ldf=0), "s"),
             (dict(s=4097, ldf=4097), "s"), (dict(ldf=5), "ldf")],
    "CROSS": [(dict(R=None), "R"), (dict(P=0), "P"), (dict(P=(1 << 24) + 1), "P"),
              (dict(ldr=9), "ldr")],
    "RULE": [(dict(kmax=0), "kmax"), (dict(kmax=11), "kmax"), (dict(criterion=2), "criterion"),
             (dict(threshold=-1.0), "threshold")],
    "XRULE": [(dict(kmax=0), "kmax"), (dict(kmax=11), "kmax"), (dict(threshold=-1.0), "threshold")],
    "ROUND": [(dict(kmax=0), "kmax"), (dict(kmax=11), "kmax"), (dict(round=3), "round"),
              (dict(round=-1), "round"), (dict(forced=P8, j=-1), "j"),
              (dict(selected=None), "selected")],
    "WS": [(dict(ws=None), "ws")],
    "XY": [(dict(x=None), "x"), (dict(y=None), "y")],
    "N1": [(dict(n=0), "n"), (dict(n=(1 << 21) + 1), "n")],
}
GROUPS = dict(SIG=SIG, SGEN=SGEN, KGEN=KGEN, SFAC=SFAC, CROSS=CROSS, RULE=RULE, XRULE=XRULE,
              ROUND=ROUND, WS=WS, XY=XY, N1=dict(n=10, diag=None))

# entry -> its groups in ABI order (the groups whose bad arguments are tried)
ROUND_ENTRIES = {
    "vgposp_crit_init": ("SIG", "RULE", "WS"),
    "vgposp_crit_step": ("SIG", "ROUND", "WS"),
    "vgposp_critx_init": ("SIG", "CROSS", "XRULE", "WS"),
    "vgposp_critx_step": ("SIG", "CROSS", "ROUND", "WS"),
    "vgposp_critk_init": ("SIG", "KGEN", "XRULE", "WS"),
    "vgposp_critk_step": ("SIG", "KGEN", "ROUND", "WS"),
    "vgposp_critg_init": ("SGEN", "RULE", "WS"),
    "vgposp_critg_step": ("SGEN", "ROUND", "WS"),
    "vgposp_critgk_init": ("N1", "KGEN", "XRULE", "WS"),
    "vgposp_critgk_step": ("N1", "KGEN", "ROUND", "WS"),
    "vgposp_critf_init": ("SFAC", "RULE", "WS"),
    "vgposp_critf_step": ("SFAC", "ROUND", "WS"),
}

# the pass entries: their arguments in ABI order and the bad ones; a null workspace is
# VGPOSP_E_WS there, not a position
KGEMV = dict(kind=0, Xt=P8, P=12, X=P8, n=10, d=2, amp=P8, ls=P8, target_scale=None,
             site_scale=None)
PASS_ENTRIES = {
    "vgposp_symv_upper": (dict(A=P8, n=10, lda=10, diag=None),
                          [(dict(A=None), "A"), (dict(n=-1), "n"), (dict(n=(1 << 21) + 1), "n"),
                           (dict(lda=9), "lda")]),
    "vgposp_gemv_t": (dict(R=P8, P=12, n=10, ldr=10),
                      [(dict(R=None), "R"), (dict(P=-1), "P"), (dict(P=(1 << 24) + 1), "P"),
                       (dict(n=-1), "n"), (dict(n=(1 << 21) + 1), "n"), (dict(ldr=9), "ldr")]),
    "vgposp_kernel_gemv_t": (KGEMV, BAD["KGEN"][:2] + [(dict(Xt=None), "Xt"), (dict(P=-1), "P"),
                                                        (dict(X=None), "X"), (dict(n=-1), "n"),
                                                        (dict(d=0), "d"), (dict(d=9), "d"),
                                                        (dict(amp=None), "amp"),
                                                        (dict(ls=None), "ls")]),
    "vgposp_kernel_symv": (SGEN, [c for c in BAD["SGEN"] if c[1] != "n"] + [(dict(n=-1), "n")]),
    "vgposp_factor_symv": (SFAC, [c for c in BAD["SFAC"] if c[1] != "n"]
                           + [(dict(n=-1), "n"), (dict(n=(1 << 22) + 1), "n")]),
}
PASS_ENTRIES.update({name + "_sq": v for name, v in list(PASS_ENTRIES.items())})

BUFFERS = {   # entry -> (its sizes in ABI order, the number of outputs)
    "vgposp_crit_buffers": (("n", "kmax"), 4),
    "vgposp_critx_buffers": (("n", "P", "kmax"), 5),
    "vgposp_critk_buffers": (("n", "P", "kmax"), 5),
    "vgposp_critg_buffers": (("n", "kmax"), 4),
    "vgposp_critgk_buffers": (("n", "P", "kmax"), 5),
    "vgposp_critf_buffers": (("n", "s", "kmax"), 4),
}
SIZES = dict(n=600, P=700, s=5, kmax=4)


def _cases(table):
    for entry, spec in table.items():
        if isinstance(spec[0], str):      # the names of its groups
            args = {}
            for grp in spec:
                assert not set(args) & set(GROUPS[grp]), (entry, grp)
                args.update(GROUPS[grp])
            cases = [c for grp in spec for c in BAD[grp]]
        else:
            args = dict(spec[0], **XY, **WS)
            cases = spec[1] + BAD["XY"]
        for bad, name in cases:
            yield pytest.param(entry, args, bad, list(args).index(name) + 1,
                               id=f"{entry}-{'-'.join(f'{k}={v}' for k, v in bad.items())}"
                               .replace("c_void_p(8)", "ptr"))


def _expect(entry, args, bad, number):
    assert len(args) == len(_lib.SIGNATURES[entry][1]), entry
    assert set(bad) <= set(args), bad
    lib = _lib.load()
    assert getattr(lib, entry)(*dict(args, **bad).values()) == -number, (entry, bad)
    err = _lib.last_error()
    assert err.startswith(f"{entry}: bad argument {number}"), err
    assert not err[len(f"{entry}: bad argument {number}"):][:1].isdigit(), err
    # ... and the valid arguments pass every check up to the workspace size
    assert getattr(lib, entry)(*dict(args, ws_bytes=16).values()) == _lib.E_WS, entry
    assert _lib.last_error().startswith(f"{entry}: workspace 16 <"), _lib.last_error()


@pytest.mark.parametrize("entry,args,bad,number", _cases(ROUND_ENTRIES))
def test_round_entries(entry, args, bad, number):
    _expect(entry, args, bad, number)


@pytest.mark.parametrize("entry,args,bad,number", _cases(PASS_ENTRIES))
def test_pass_entries(entry, args, bad, number):
    _expect(entry, args, bad, number)


def test_every_entry_is_covered():
    crit = {s for s in _lib.SIGNATURES
            if s.startswith("vgposp_crit") and not s.endswith("_workspace_bytes")}
    assert crit == set(ROUND_ENTRIES) | set(BUFFERS)
    assert len(PASS_ENTRIES) == 10


def _buffers(entry, ws=4096, **over):
    sizes, nout = BUFFERS[entry]
    ptr = [ctypes.c_void_p() for _ in range(nout)]
    vals = [dict(SIZES, **over)[k] for k in sizes]
    rc = getattr(_lib.load(), entry)(ctypes.c_void_p(ws) if ws else None, *vals,
                                     *[ctypes.byref(p) for p in ptr])
    return rc, [p.value for p in ptr]


@pytest.mark.parametrize("entry", BUFFERS)
def test_buffers_arguments(entry):
    sizes, nout = BUFFERS[entry]
    assert len(_lib.SIGNATURES[entry][1]) == 1 + len(sizes) + nout
    for number, bad in enumerate([dict(ws=None)] + [{k: 0} for k in sizes], start=1):
        assert _buffers(entry, **bad)[0] == -number, (entry, bad)
        assert _lib.last_error().startswith(f"{entry}: bad argument {number} "), _lib.last_error()
    # every output is optional
    assert getattr(_lib.load(), entry)(ctypes.c_void_p(4096), *[SIZES[k] for k in sizes],
                                       *[None] * nout) == 0


def test_buffers_offsets():
    """nom, score, delta, W at crit_layout's offsets in every family; U follows the location
    side, whose pass area only critgk (no pass over Sigma) does without."""
    rc, crit = _buffers("vgposp_crit_buffers")
    assert rc == 0 and crit[0] > 4096 and all(a < b for a, b in zip(crit, crit[1:]))
    n, kmax = SIZES["n"], SIZES["kmax"]
    assert crit[1] - crit[0] >= 8 * n and crit[3] - crit[2] >= 8 * n
    for entry in ("vgposp_critg_buffers", "vgposp_critf_buffers"):
        assert _buffers(entry) == (0, crit), entry
    rc, critx = _buffers("vgposp_critx_buffers")
    assert rc == 0 and critx[:4] == crit and critx[4] >= crit[3] + 8 * kmax * n
    assert _buffers("vgposp_critk_buffers") == (0, critx)
    rc, critgk = _buffers("vgposp_critgk_buffers")
    assert rc == 0 and critgk[:4] == crit
    # the location side's partials are those of vgposp_symv_upper, aligned to 256 bytes
    up = _lib.query("vgposp_symv_upper_workspace_bytes", n)
    assert 0 <= critx[4] - critgk[4] - up < 256
    # the offsets do not depend on where the workspace lies
    rc, moved = _buffers("vgposp_critx_buffers", ws=4096 + 512)
    assert rc == 0 and [p - 512 for p in moved] == critx
