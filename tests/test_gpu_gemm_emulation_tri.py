"""The structured products of the factorization on the int8 matrix cores (vgposp_gemm_emulated_tri:
lower SYRK, tri-B, tri-A as staircases of block products) at sizes that run in a second or two, the
block width lowered to 256 so that a 768-order product has several steps.

* integer-valued operands give the exact product, bit for bit, with beta, at ragged orders, the
  SYRK's strict upper triangle untouched and the strict upper triangle of X (NaN) never read;
* a scratch too small for the whole product (tiles) gives the same bits;
* operands that stress the scaling stay within the derived truncation bound;
* the fused factor + inverse reaches the drivers, meets the classical tolerance, is deterministic,
  and the profile counters show the launches the routing rule moves and the planner's flops.
"""
import numpy as np
import pytest
import torch

from test_gemm_emulation_host import emulation_setting
from test_gemm_emulation_tri_host import SYRK, TRMM_A, TRMM_B, plan, tri_block
from test_gpu_gemm_emulation import _scale_bits
from test_gpu_strassen import _potrf

pytestmark = pytest.mark.gpu

GIB = 1 << 30
SENTINEL = np.float64(-7.25e300)


@pytest.fixture(scope="module")
def L():
    from vgposp_amd import _lib, linalg
    torch.cuda.set_device(0)
    assert _lib.load().vgposp_gemm_emulation_available() == 1, "libhipblaslt.so.1 did not resolve"
    return linalg


@pytest.fixture(autouse=True)
def width_256():
    with tri_block(256):
        yield


def _tri(L, kind, m, n, k, alpha, A, B, beta, C, nbytes=GIB // 4):
    from vgposp_amd._lib import call
    ws = L.workspace(nbytes)
    call("vgposp_gemm_emulated_tri", kind, m, n, k, float(alpha), L._p(A), A.stride(0),
         L._p(B) if B is not None else None, B.stride(0) if B is not None else 0, float(beta),
         L._p(C), C.stride(0), L._p(ws), ws.numel(), L._stream())
    torch.cuda.synchronize()


def _int_case(kind, m, n, seed):
    """Integer operands below 2^20 (every partial sum below 2^50: int64 and fp64 hold it), C0 below
    2^40, the exact A B in int64; the strict upper triangle of X is NaN on the device side."""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.integers(-2 ** 20 + 1, 2 ** 20, s).astype(np.int64)  # noqa: E731
    if kind == SYRK:
        k = 384
        A, B = r(n, k), None
        AB, Ad, Bd = A @ A.T, A.astype(np.float64), None
    elif kind == TRMM_B:
        k = n
        A, X = r(m, n), np.tril(r(n, n))
        AB, Ad = A @ X, A.astype(np.float64)
        Bd = X.astype(np.float64)
        Bd[np.triu_indices(n, 1)] = np.nan
    else:
        k = m
        X, B = np.tril(r(m, m)), r(m, n)
        AB, Bd = X @ B, B.astype(np.float64)
        Ad = X.astype(np.float64)
        Ad[np.triu_indices(m, 1)] = np.nan
    C0 = rng.integers(-2 ** 40, 2 ** 40, (m, n)).astype(np.int64)
    return k, Ad, Bd, C0, AB


CASES = [(SYRK, 768, 768), (TRMM_B, 640, 768), (TRMM_A, 768, 640),
         (SYRK, 640, 640), (TRMM_B, 512, 640), (TRMM_A, 640, 512)]  # the last three ragged: 640 = 2.5 x 256


@pytest.fixture(scope="module")
def int_cases():
    return {c: _int_case(*c, seed=20 + i) for i, c in enumerate(CASES)}


def _run_int(L, case, data, alpha, beta, nbytes=GIB // 4):
    kind, m, n = case
    k, Ad, Bd, C0, AB = data
    C = L.as_device(C0.astype(np.float64))
    if kind == SYRK:
        C[torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"), 1)] = float(SENTINEL)
    _tri(L, kind, m, n, k, alpha, L.as_device(Ad), L.as_device(Bd) if Bd is not None else None,
         beta, C, nbytes)
    return C.cpu().numpy()


@pytest.mark.parametrize("alpha,beta", [(1.0, 0.0), (-1.0, 1.0)])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_exact_products(L, int_cases, case, alpha, beta):
    kind, m, n = case
    k, _, _, C0, AB = int_cases[case]
    steps, _ = plan(kind, m, n, k, GIB // 4)
    assert len(steps) >= 3 and len({s[0] for s in steps}) == 1  # several steps, one tile
    got = _run_int(L, case, int_cases[case], alpha, beta)
    exact = (int(alpha) * AB + int(beta) * C0).astype(np.float64)
    if kind == SYRK:
        il, iu = np.tril_indices(n), np.triu_indices(n, 1)
        np.testing.assert_array_equal(got[il], exact[il])
        # the strict upper triangle keeps the sentinel byte for byte
        assert np.all(got[iu].view(np.int64) == SENTINEL.view(np.int64))
    else:
        assert not np.isnan(got).any()  # one load of X's NaN triangle would make a NaN row
        np.testing.assert_array_equal(got, exact)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_tiles_give_the_same_bits(L, int_cases, case):
    """A scratch one byte short of the whole product, and one of two thirds: the planner tiles, the
    results are the untiled bits."""
    kind, m, n = case
    k = int_cases[case][0]
    steps, _ = plan(kind, m, n, k, GIB // 4)
    whole = steps[0][13]
    ref = _run_int(L, case, int_cases[case], -1.0, 1.0)
    for nbytes in (whole - 1, 2 * whole // 3):
        tiled, _ = plan(kind, m, n, k, nbytes)
        assert len({s[0] for s in tiled}) > 1
        got = _run_int(L, case, int_cases[case], -1.0, 1.0, nbytes)
        np.testing.assert_array_equal(got.view(np.int64), ref.view(np.int64))
    # the block cap does the same as a small scratch
    from vgposp_amd import _lib
    _lib.call("vgposp_gemm_emulation_set_block_cap", whole - 1)
    try:
        got = _run_int(L, case, int_cases[case], -1.0, 1.0)
    finally:
        _lib.call("vgposp_gemm_emulation_set_block_cap", 0)
    np.testing.assert_array_equal(got.view(np.int64), ref.view(np.int64))


@pytest.mark.parametrize("kind", [SYRK, TRMM_B, TRMM_A])
def test_truncation_bound_on_scaled_operands(L, kind):
    """|C - C_ref|_ij <= 2 k 2^-s max_k|a_ik| max_k|b_kj| + 4 u |C_ref|_ij + 2^-1075 against a
    long-double product, the vectors of both operands scaled by 2^[-40, 40], one zero row (the bound
    of tests/test_gpu_gemm_emulation.py; the maxima of the bound are over the whole stored vector,
    which is at least what a triangle mode reads)."""
    n = 512
    k = 1024 if kind == SYRK else n
    rng = np.random.default_rng(30 + kind)
    A = rng.standard_normal((n, k)) * 2.0 ** rng.integers(-40, 41, (n, 1))
    B = rng.standard_normal((k, n)) * 2.0 ** rng.integers(-40, 41, (1, n))
    A[7] = 0.0
    if kind == SYRK:
        B = A.T.copy()
    elif kind == TRMM_B:
        B = np.tril(B)
    else:
        A = np.tril(A)
    ref = A.astype(np.longdouble) @ B.astype(np.longdouble)
    C = torch.full((n, n), 7.0, dtype=torch.float64, device="cuda")
    _tri(L, kind, n, n, k, 1.0, L.as_device(A), None if kind == SYRK else L.as_device(B), 0.0, C)
    got = C.cpu().numpy()
    scale = np.abs(A).max(1)[:, None].astype(np.longdouble) * np.abs(B).max(0)[None, :]
    s = _scale_bits(k)
    assert s == 57
    bound = 2 * k * np.longdouble(2.0) ** -s * scale + 4 * np.longdouble(2.0) ** -53 * np.abs(ref) \
        + np.longdouble(2.0) ** -1075
    err = np.abs(got.astype(np.longdouble) - ref)
    live = np.tril(np.ones((n, n), dtype=bool)) if kind == SYRK else np.ones((n, n), dtype=bool)
    rel = (err / np.maximum(scale, np.longdouble(2.0) ** -900))[live]
    print(f"kind {kind}: largest |C - C_ref|_ij / (max|a_i| max|b_j|) = {float(rel.max()):.3e}")
    assert np.all(err[live] <= bound[live]), float((err[live] / bound[live]).max())
    assert np.all(got[7][live[7]] == 0.0)
    if kind == SYRK:
        assert np.all(got[~live] == 7.0)


def _psyrk_routed(n, k, min_dim, out):
    """potrf.hip's routing rule for psyrk(n, k): a driver where the plain half is eligible."""
    h = n // 2
    if n % 2 == 0 and min(h, k) >= min_dim and h % 256 == 0 and k % 256 == 0:
        out.append((n, k))


def _routed_syrks(n, min_dim, out):
    """The psyrk calls of potrf_rec(n) (split at 128 * (ceil(n / 128) // 2)) that go to the driver."""
    if n <= 128:
        return
    n1 = 128 * (-(-n // 128) // 2)
    _routed_syrks(n1, min_dim, out)
    _psyrk_routed(n - n1, n1, min_dim, out)
    _routed_syrks(n - n1, min_dim, out)


def _tree_launches(n, k, min_dim):
    """(fp64 structured leaves, plain products) of the split tree psyrk(n, k) runs without a driver."""
    h = n // 2
    if n % 2 or min(h, k) < min_dim or h % 256 or k % 256:
        return 1, 0
    a = _tree_launches(h, k, min_dim)
    return 2 * a[0], 2 * a[1] + 1


DRIVER_SCOPES = ("gemm_i8[syrk]", "gemm_i8[trmm_b]", "gemm_i8[trmm_a]")


def _profiled(fn):
    """fn's result and the profile counters of its launches: {name: (ms, launches, flops, bytes)}
    (the dump prints seven digits; the drivers' scopes are queried for their exact flops)."""
    from vgposp_amd import _lib
    _lib.prof_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = _lib.prof_dump()
        for name in DRIVER_SCOPES:
            if name in prof:
                prof[name] = _lib.prof_query(name)
        return out, prof
    finally:
        _lib.prof_enable(False)


def _structured(on):
    from vgposp_amd import _lib
    _lib.call("vgposp_potrf_set_emulation_structured", int(on))


def test_through_the_factorization(L):
    """n = 2,048 at threshold 256: the SYRKs of orders 1,024 and 512 go to the driver (the inverse's
    products of this size are the level-batched launches, which the routing leaves alone)."""
    from oracle import gp as ogp
    from vgposp_amd.workloads import placement_split
    X, ls = placement_split((16, 16, 8), 0)
    S = ogp.kernel_matrix("eq", X, X, 1.0, ls)[0] + (1e-2 + 1e-6) * np.eye(len(X))
    Lref = np.linalg.cholesky(S)
    prob = dict(S=S, L=Lref, Linv=np.linalg.inv(Lref))
    S, il = prob["S"], np.tril_indices(2048)
    routed = []
    _routed_syrks(2048, 256, routed)
    assert sorted(routed) == [(512, 512), (512, 512), (1024, 1024)]
    with emulation_setting(256, 16):
        for invert, ref in ((1, prob["Linv"]), (0, prob["L"])):
            A = _potrf(L, S, invert)
            Ah = A.cpu().numpy()
            np.testing.assert_allclose(Ah[il], ref[il], rtol=1e-9, atol=1e-10 * np.abs(ref).max())
            np.testing.assert_array_equal(np.triu(Ah, 1), np.triu(S, 1))
            assert torch.equal(A, _potrf(L, S, invert))  # a second run is bit-identical
        Aon, on = _profiled(lambda: _potrf(L, S, 1))
        _structured(0)
        try:
            Aoff, off = _profiled(lambda: _potrf(L, S, 1))
        finally:
            _structured(1)
    assert not torch.equal(Aon, Aoff)  # the drivers did run
    print({k: v[1] for k, v in on.items()}, {k: v[1] for k, v in off.items()})
    # gemm_i8 flops of the drivers = the planner's count over the routed products
    want = sum(plan(SYRK, n, n, k, GIB)[1] for n, k in routed)
    assert on["gemm_i8[syrk]"][2] == want and on["gemm_i8[syrk]"][1] == sum(n // 256 for n, _ in routed)
    assert "gemm_i8[syrk]" not in off and "gemm_i8[trmm_b]" not in on and "gemm_i8[trmm_a]" not in on
    # the launches the routing moved: every structured fp64 leaf and every plain int8 product of the
    # routed trees is gone, nothing else changed; no triangular class moved at this size
    leaves = sum(_tree_launches(n, k, 256)[0] for n, k in routed)
    plains = sum(_tree_launches(n, k, 256)[1] for n, k in routed)
    f64 = lambda d: sum(v[1] for name, v in d.items() if name.startswith("gemm_f64"))  # noqa: E731
    assert f64(off) - f64(on) == leaves
    assert off["gemm_i8"][1] - on["gemm_i8"][1] == plains
    for name in set(on) | set(off):
        if "tri" in name and name.startswith("gemm_f64"):
            assert on[name][1] == off[name][1], name


def test_inverse_reaches_the_trmm_drivers(L):
    """n = 8,192 at threshold 2,048: above the level-batched part of the inverse (order 4,096) the
    top node's W = L21 X11 and X21 = -X22 W go to the tri-B and tri-A drivers; the profile shows no
    fp64 launch of the two triangular classes for them, and the result is the classical one to the
    factorization's tolerance."""
    from vgposp_amd.workloads import placement_split
    X, ls = placement_split((32, 16, 16), 0)
    n = len(X)
    Sd = torch.empty((n, n), dtype=torch.float64, device="cuda")
    L.kernel_matrix("eq", L.as_device(X), None, 1.0, ls, diag_shift=1e-2 + 1e-6, out=Sd[None])
    S = Sd.cpu().numpy()

    def run():
        return _potrf(L, S, 1)

    with tri_block(1024):
        want = {kind: plan(kind, 4096, 4096, 4096, GIB)[1] for kind in (SYRK, TRMM_B, TRMM_A)}
        with emulation_setting(2048, 0):
            Acl, cl = _profiled(run)
        with emulation_setting(2048, 16):
            Aon, on = _profiled(run)
            assert torch.equal(Aon, run())
            _structured(0)
            try:
                _, off = _profiled(run)
            finally:
                _structured(1)
    il = np.tril_indices(n)
    a, c = Aon.cpu().numpy()[il], Acl.cpu().numpy()[il]
    np.testing.assert_allclose(a, c, rtol=1e-9, atol=1e-10 * np.abs(c).max())
    assert torch.equal(torch.triu(Aon, 1), torch.triu(Sd, 1))
    print({k: v[1] for k, v in on.items()}, {k: v[1] for k, v in off.items()})
    def launches(d, cls):  # the class's wide and narrow launches
        return sum(d.get(f"gemm_f64[{cls}{w}]", (0, 0))[1] for w in ("", ",narrow"))

    for kind, name, cls in ((TRMM_B, "gemm_i8[trmm_b]", "nn,triB"), (TRMM_A, "gemm_i8[trmm_a]", "nn,triA")):
        assert on[name][2] == want[kind]
        # classical: one structured launch for the product; split tree: two leaves; driver: none
        assert launches(cl, cls) - launches(on, cls) == 1
        assert launches(off, cls) - launches(on, cls) == 2
    assert on["gemm_i8[syrk]"][2] == want[SYRK]
