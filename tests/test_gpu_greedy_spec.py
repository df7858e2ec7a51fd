"""GPU: the speculative multi-column mat-vec of vgposp_greedy_step (csrc/greedy.hip,
vgposp_greedy_set_speculation) changes speed only.

Width w forms, in one pass over L^-1, the pick's column q_a and up to w - 1 columns the next rounds
will probably ask for; a round whose pick is cached reads nothing of L^-1.  Every output of every
round must be the width-1 (classic) one bit for bit — no tolerance anywhere in this file: delta,
piv, xcol, cache, selected, sel_delta, evals and the head of the workspace that holds prm, sdiag,
nom, prec, delta, cache, W and V.

Inputs: F1 of tests/greedy_state_reference.py (n = 1,040: three 512-row chunks, three column
tiles, two candidate chunks, R.ROUNDS rounds) and G, the benchmark's family at
placement_split((12, 12, 8), 0) (n = 1,152, EQ, ls = 2h, diagonal + 1e-2 + 1e-6, k = 16: 15
mat-vec rounds).  Every test restores the width it found.
"""
import numpy as np
import pytest

from tests import greedy_state_reference as R
from tests.greedy_driver import KEYS, PARAMS
from tests.greedy_driver import Greedy as Driver

pytestmark = pytest.mark.gpu

G_SHAPE, G_K = (12, 12, 8), 16


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module", autouse=True)
def _device():
    import torch
    torch.cuda.set_device(0)


class width:
    """vgposp_greedy_set_speculation(w) for a with-block; restores the previous width."""

    def __init__(self, w):
        self.new = w

    def __enter__(self):
        from vgposp_amd import _lib
        self.old = _lib.load().vgposp_greedy_speculation()
        _lib.call("vgposp_greedy_set_speculation", self.new)

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_greedy_set_speculation", self.old)


_cov = {}


def g_cov(seed=0):
    if seed not in _cov:
        from oracle import gp as ogp
        from vgposp_amd.workloads import placement_split
        X, ls = placement_split(G_SHAPE, seed)
        _cov[seed] = ogp.kernel_matrix("eq", X, X, 1.0, ls)[0] + R.NOISE * np.eye(len(X))
    return _cov[seed]


def cov_of(name):
    return R.fixture_cov("F1") if name == "F1" else g_cov(0)


def Greedy(K, kmax, lda=None, shift=0):
    """The whole of K with placement_algorithm2's constants."""
    return Driver(K, K.shape[0], kmax, PARAMS, lda, shift)


def rounds(g, first, k, lazy):
    """k rounds from round `first`; per round the state and the counters."""
    recs, stats = [], []
    for r in range(first, first + k):
        g.step(r, lazy)
        recs.append(g.read())
        stats.append(g.stats())
    return recs, stats


_runs = {}


def run(name, w, lazy=True, lda=None, shift=0, masked=False, placed=(), k=None):
    """init (+ mask, + conditioning) and the rounds at width w, once per process."""
    key = (name, w, lazy, lda, shift, masked, tuple(placed), k)
    if key not in _runs:
        K = cov_of(name)
        k_ = k or (R.ROUNDS if name == "F1" else G_K)
        m = len(placed)
        with width(w):
            g = Greedy(K, m + k_, lda, shift).init()
            blocked = R.third_mask(g.n) if masked else np.zeros(g.n, dtype=bool)
            if masked:
                g.mask(blocked)
            if m:
                g.condition(placed, k_, 8)
            recs, stats = rounds(g, m, k_, lazy)
            out = {"recs": recs, "stats": stats, "table": g.table(), "blocked": blocked,
                   "buf": g.buf.cpu().numpy().copy(), "host0": g.host0, "n": g.n, "m": m}
        _runs[key] = out
    return _runs[key]


def assert_same_rounds(got, ref, label):
    assert len(got) == len(ref)
    for r, (a, b) in enumerate(zip(got, ref)):
        for key in KEYS:
            assert _same(a[key], b[key]), (label, "round", r, key)


def written(rec, r, n, kmax):
    """What round r and the rounds before it wrote, of a record of a run without placed sensors:
    a second run in one workspace leaves the first run's later rounds in the rest (pivots and
    rows of W and V from round r on, the picks after round r)."""
    al = lambda b: (b + 255) // 256 * 256
    head = al(64) + 5 * al(8 * n)                    # prm, sdiag, nom, prec, delta, cache
    rows = al(8 * kmax * n)                          # W, then V: row t is written by round t + 1
    st = rec["state"]
    assert len(st) == head + 2 * rows
    out = {k: rec[k] for k in ("delta", "cache") + (("xcol",) if r else ())}  # round 0: no column
    out.update({k: rec[k][:r + 1] for k in ("selected", "sel_delta", "evals")})
    out["piv"] = rec["piv"][:2 + 2 * r]
    out["state"] = np.concatenate([st[:head], st[head:head + 8 * r * n],
                                   st[head + rows:head + rows + 8 * r * n]])
    return out


WIDTHS = [2, 4, 8]
MODES = [pytest.param(True, id="lazy"), pytest.param(False, id="full")]


# ---- 1. the same bits at every width ----
@pytest.mark.parametrize("lazy", MODES)
@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("name", ["F1", "G"])
def test_same_bits_at_every_width(name, w, lazy):
    ref, got = run(name, 1, lazy), run(name, w, lazy)
    assert_same_rounds(got["recs"], ref["recs"], (name, w, lazy))
    # the comparison is not vacuous: the speculating rounds ran, and the classic ones did not
    # touch the counters
    nr = len(ref["recs"]) - 1
    assert ref["stats"][-1] == (0, 0, 0)
    assert got["stats"][-1][0] + got["stats"][-1][1] == nr and got["stats"][-1][0] >= 1


@pytest.mark.parametrize("w", WIDTHS)
@pytest.mark.parametrize("lda,shift", [(1041, 0), (1042, 0), (1042, 1)])
def test_same_bits_in_every_layout(lda, shift, w):
    """Odd lda (scalar loads), even lda with row padding (16-byte loads), and an even lda on a base
    8 bytes off 16-byte alignment (scalar loads); the padding and the surroundings keep their
    sentinel and Sigma stays above the diagonal."""
    ref, got = run("F1", 1, True, lda, shift), run("F1", w, True, lda, shift)
    assert_same_rounds(got["recs"], ref["recs"], (lda, shift, w))
    assert got["stats"][-1][0] >= 1
    n, buf, buf0 = got["n"], got["buf"], got["host0"]
    assert _same(buf, ref["buf"])
    assert _same(buf[:shift], buf0[:shift])
    M, M0 = buf[shift:].reshape(n, lda), buf0[shift:].reshape(n, lda)
    assert _same(M[:, n:], M0[:, n:])
    iu = np.triu_indices(n, 1)
    assert _same(M[:, :n][iu], M0[:, :n][iu])


# ---- 2. both paths ran ----
@pytest.mark.parametrize("w", [4, 8])
def test_hits_and_passes_on_G(w):
    passes, hits, cached = run("G", w)["stats"][-1]
    print(f"G width {w}: passes {passes} hits {hits} cached {cached}")
    assert hits >= 2 and passes >= 2 and passes + hits == G_K - 1
    assert 1 <= cached <= (w - 1) * passes


def test_width_1_never_speculates():
    assert run("G", 1)["stats"][-1] == (0, 0, 0)
    assert run("G", 1)["table"] == []


# ---- 3. a hit on an old column ----
@pytest.mark.parametrize("w,k", [(4, 32), (8, G_K)])
def test_hit_on_a_column_cached_rounds_earlier(w, k):
    """A round r hits when its pick selected[r - 1] is in the table; at least one hit on G lands on
    a column that a pass two or more rounds earlier formed (a column is kept for the whole run,
    not only for the next round).  At width 8 that happens within G's 16 rounds (the third hit);
    at width 4 the exact top-3 prediction makes every hit of the first 16 rounds one round old, so
    that case runs k = 32 rounds (the first older hit is in round 26, by the policy simulated on
    the CPU)."""
    got = run("G", w, k=k)
    assert_same_rounds(got["recs"], run("G", 1, k=k)["recs"], ("G", w, k))
    filled = dict(got["table"])
    picks = got["recs"][-1]["selected"]
    ages, before = [], 0
    for r, (_, hits, _) in enumerate(got["stats"]):
        if hits > before:
            a = int(picks[r - 1])
            assert a in filled and 1 <= filled[a] < r, (r, a)
            ages.append(r - filled[a])
        before = hits
    print(f"G width {w}: rounds between fill and hit {ages}")
    assert len(ages) == got["stats"][-1][1]
    assert max(ages) >= 2, ages


# ---- 4. re-init clears the cache ----
def test_reinit_forgets_the_previous_problem():
    """G, then another Sigma (seed 1) assembled into the same buffer and run in the same
    workspace: byte-equal to that problem in a fresh workspace, with the same counters."""
    K1 = g_cov(1)
    assert not _same(K1, g_cov(0))
    with width(8):
        g = Greedy(g_cov(0), G_K).init()
        rounds(g, 0, G_K, True)
        assert g.stats()[2] > 0
        g.load(K1)
        g.init()
        assert g.stats() == (0, 0, 0)
        again, stats = rounds(g, 0, G_K, True)
        fresh = Greedy(K1, G_K).init()
        want, wstats = rounds(fresh, 0, G_K, True)
        assert stats == wstats and g.table() == fresh.table()
    with width(1):
        classic = rounds(Greedy(K1, G_K).init(), 0, G_K, True)[0]
    assert_same_rounds(want, classic, "second problem, classic")
    for r in range(G_K):
        a, b = written(again[r], r, g.n, G_K), written(want[r], r, g.n, G_K)
        for key in a:
            assert _same(a[key], b[key]), ("second problem", "round", r, key)


# ---- 5. constraints ----
def _check_table(got):
    picks = [int(a) for a in got["recs"][-1]["selected"]]
    cols = [c for c, _ in got["table"]]
    assert len(set(cols)) == len(cols)
    for c, fill in got["table"]:
        assert 0 <= c < got["n"] and max(got["m"], 1) <= fill < len(picks)
        assert not got["blocked"][c], c                 # never a masked location
        assert c not in picks[:fill], (c, fill)         # never one selected (or placed) by then


@pytest.mark.parametrize("w", [4, 8])
def test_candidate_mask(w):
    ref, got = run("F1", 1, masked=True), run("F1", w, masked=True)
    assert_same_rounds(got["recs"], ref["recs"], ("masked", w))
    assert got["stats"][-1][2] > 0
    _check_table(got)


@pytest.mark.parametrize("w", [4, 8])
def test_placed_sensors(w):
    """R.PLACED conditioned on with batch 8, then free rounds: the first free round's mat-vec is
    for the last placed sensor, and no placed sensor is ever speculated on."""
    ref, got = run("F1", 1, placed=R.PLACED), run("F1", w, placed=R.PLACED)
    assert_same_rounds(got["recs"], ref["recs"], ("placed", w))
    assert got["stats"][-1][2] > 0
    assert not set(R.PLACED) & {c for c, _ in got["table"]}
    _check_table(got)


def test_unconstrained_tables():
    for name in ("F1", "G"):
        for w in WIDTHS:
            _check_table(run(name, w))


# ---- 6. one graph ----
def test_rounds_in_one_graph():
    """Re-copy of Sigma, init and the k rounds of G captured into one graph at width 8: hit or
    miss, a round is the same launch sequence, so the replays give the eager run's picks, deltas
    and evaluation counts, and its counters."""
    import torch
    want = run("G", 8)
    last = want["recs"][-1]
    with width(8):
        g = Greedy(g_cov(0), G_K).init()
        rounds(g, 0, G_K, True)  # warm-up (module loads)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g.buf.copy_(g.src)
            g.init()
            for r in range(G_K):
                g.step(r, True)
        for _ in range(2):
            g.selected.fill_(-1)
            graph.replay()
            torch.cuda.synchronize()
            rec = g.read()
            for key in ("selected", "sel_delta", "evals", "delta", "state"):
                assert _same(rec[key], last[key]), key
            assert g.stats() == want["stats"][-1]
