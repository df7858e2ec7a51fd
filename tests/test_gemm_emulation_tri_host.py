"""Host side of the structured int8 drivers (gemm_emul.hip), no GPU: the planner that cuts a lower
SYRK, a tri-B or a tri-A product into tiles and staircase steps, and the workspace queries, which
the drivers must leave as they were."""
import ctypes

import numpy as np
import pytest

SYRK, TRMM_B, TRMM_A = 0, 1, 2
FIELDS = 14
GIB = 1 << 30
# the emulation areas of the factorization's workspace at n = 32,768 and 65,536 (the difference of
# vgposp_potrf_workspace_bytes with the int8 library present and counted absent, PARENT_WS below)
AREA_32K = 14864810496 - 3053453824   # 11.0 GiB + the maxima
AREA_65K = 37715444224 - 11945378304  # 24.0 GiB + the maxima

# vgposp_potrf_workspace_bytes(n) and vgposp_greedy_workspace_bytes(65536, 50) of the parent commit
# (6c656b9, "Emulate the large fp64 products of the Cholesky on int8 matrix cores"), read from that
# commit's own library with hipBLASLt resolved and the default setting (8192, 16).
PARENT_WS = {16384: 754975232, 32768: 14864810496, 65536: 37715444224}
PARENT_GREEDY_65536_50 = 37838331392
# the same with the library counted absent (vgposp_gemm_emulation_set_unavailable(1))
PARENT_WS_ABSENT = {16384: 754975232, 32768: 3053453824, 65536: 11945378304}
PARENT_GREEDY_65536_50_ABSENT = 12068265472

# int8 flops (2 * 16 * rows * columns * depth, summed over the steps) of the structured products of
# the 65k step at the default block width 2,048, as DESIGN.md §4 states them
DESIGN_FLOPS = {
    (SYRK, 16384, 16384, 16384, AREA_32K): 79164837199872.0,
    (TRMM_B, 16384, 16384, 16384, AREA_32K): 79164837199872.0,
    (TRMM_A, 16384, 16384, 16384, AREA_32K): 79164837199872.0,
    (SYRK, 32768, 32768, 32768, AREA_65K): 598134325510144.0,
    (TRMM_B, 32768, 32768, 32768, AREA_65K): 598134325510144.0,
    (TRMM_A, 32768, 32768, 32768, AREA_65K): 598134325510144.0,
}


class tri_block:
    """vgposp_gemm_emulation_set_tri_block(width) for a with-block; 0 (the default) afterwards."""

    def __init__(self, width):
        self.width = width

    def __enter__(self):
        from vgposp_amd import _lib
        _lib.call("vgposp_gemm_emulation_set_tri_block", self.width)

    def __exit__(self, *exc):
        from vgposp_amd import _lib
        _lib.call("vgposp_gemm_emulation_set_tri_block", 0)
        return False


def plan(kind, m, n, k, nbytes):
    """[(tile, r0, r1, c0, c1, ka, kb, i0, i1, j0, j1, k0, k1, tile_bytes)], flops; None if nothing fits."""
    from vgposp_amd import _lib
    lib = _lib.load()
    fl = ctypes.c_double()
    cnt = lib.vgposp_gemm_emulation_tri_plan(kind, m, n, k, nbytes, None, 0, ctypes.byref(fl))
    if cnt < 0:
        return None, 0.0
    buf = (ctypes.c_int64 * (FIELDS * cnt))()
    assert lib.vgposp_gemm_emulation_tri_plan(kind, m, n, k, nbytes, buf, cnt, ctypes.byref(fl)) == cnt
    return [tuple(buf[FIELDS * q:FIELDS * (q + 1)]) for q in range(cnt)], fl.value


def _al(x):
    return (x + 255) // 256 * 256


def _up(x, to=128):
    return (x + to - 1) // to * to


def check_plan(kind, m, n, k, nbytes, width):
    steps, flops = plan(kind, m, n, k, nbytes)
    assert steps is not None
    g = 128 if max(m, n) > 4096 else 1  # coverage at the granularity every bound is a multiple of
    assert m % g == 0 and n % g == 0 and width % g == 0
    cover = np.zeros((m // g, n // g), dtype=np.int32)
    fl = 0.0
    tiles = {}
    for (tile, r0, r1, c0, c1, ka, kb, i0, i1, j0, j1, k0, k1, tb) in steps:
        assert 0 <= r0 <= i0 < i1 <= r1 <= m and 0 <= c0 <= j0 < j1 <= c1 <= n
        assert 0 <= ka <= k0 < k1 <= kb <= k
        assert i1 - i0 <= width or kind == TRMM_B
        assert j1 - j0 <= width or kind != TRMM_B
        # the depth is exactly the structured range of the block, on 128-entry boundaries
        want = {SYRK: (0, k), TRMM_B: (j0, k), TRMM_A: (0, i1)}[kind]
        assert (k0, k1) == want
        assert k0 % 128 == 0 and (k0 - ka) % 128 == 0 and ka % 128 == 0
        assert k1 % 128 == 0 or k1 == k
        cover[i0 // g:-(-i1 // g), j0 // g:-(-j1 // g)] += 1
        if kind == SYRK:
            assert j1 <= i1  # nothing right of the block row's own diagonal block
        fl += 2.0 * 16 * (i1 - i0) * (j1 - j0) * _up(k1 - k0)
        t = tiles.setdefault(tile, dict(key=(r0, r1, c0, c1, ka, kb), cm=0, cn=0, tb=tb))
        assert t["key"] == (r0, r1, c0, c1, ka, kb) and t["tb"] == tb
        if (i1 - i0) * (j1 - j0) > t["cm"] * t["cn"]:
            t["cm"], t["cn"] = i1 - i0, j1 - j0
    assert fl == flops
    # every block of the result exactly once (SYRK: of the lower triangle; above it only the upper
    # half of a diagonal block, which the reconstruction masks)
    if kind == SYRK:
        I, J = np.indices(cover.shape)
        assert np.all(cover[J <= I] == 1)
        assert np.all(cover[J * g >= (I * g // width + 1) * width] == 0)
    else:
        assert np.all(cover == 1)
    # planes + maxima + the largest int32 block of every tile fit
    for t in tiles.values():
        r0, r1, c0, c1, ka, kb = t["key"]
        kp = _up(kb - ka)
        shared = kind == SYRK and (r0, r1) == (c0, c1)
        need = _al(8 * (r1 - r0)) + _al(16 * (r1 - r0) * kp) + _al(64 * t["cm"] * t["cn"])
        if not shared:
            need += _al(8 * (c1 - c0)) + _al(16 * (c1 - c0) * kp)
        assert need == t["tb"] <= nbytes
    return steps, flops, tiles


@pytest.mark.parametrize("kind", [SYRK, TRMM_B, TRMM_A])
@pytest.mark.parametrize("n,area", [(16384, AREA_32K), (32768, AREA_65K)])
def test_planner_at_the_step_sizes(kind, n, area):
    """The routed products of n = 32,768 (order 16,384 in 11.0 GiB) and of 65,536 (order 32,768 in
    24.0 GiB; the order-16,384 ones fit as at 32,768) at the default block width."""
    steps, flops, tiles = check_plan(kind, n, n, n, area, 2048)
    assert flops == DESIGN_FLOPS[(kind, n, n, n, area)]
    # whole where it fits: everything at 16,384 and the top SYRK at 32,768; the top tri-B and tri-A
    # of the 65k step in 2 x 2 tiles (each operand element split at most twice)
    assert len(tiles) == (4 if kind != SYRK and n == 32768 else 1)
    nb = n // 2048
    assert len(steps) == (2 * nb if len(tiles) == 4 else nb)


@pytest.mark.parametrize("kind", [SYRK, TRMM_B, TRMM_A])
@pytest.mark.parametrize("m,n", [(768, 640), (640, 768), (768, 768), (640, 640), (1152, 896),
                                 (896, 896)])
def test_planner_small_and_ragged(kind, m, n):
    if kind == SYRK:
        m = n
    k = {SYRK: 384, TRMM_B: n, TRMM_A: m}[kind]
    with tri_block(256):
        _, flops, tiles = check_plan(kind, m, n, k, GIB, 256)
        assert len(tiles) == 1
        whole = tiles[0]["tb"]
        for cap in (whole - 1, 2 * whole // 3):  # one byte short of the whole product; two thirds
            _, tflops, tiled = check_plan(kind, m, n, k, cap, 256)
            assert len(tiled) > 1
            assert tflops == flops  # tiling cuts the same staircase
        assert plan(kind, m, n, k, 4096)[0] is None  # not even one block


def test_workspace_queries_equal_the_parents():
    from vgposp_amd import _lib
    have = bool(_lib.load().vgposp_gemm_emulation_available())
    for absent in ([True] if not have else [False, True]):
        _lib.call("vgposp_gemm_emulation_set_unavailable", int(absent))
        try:
            for n, want in (PARENT_WS_ABSENT if absent else PARENT_WS).items():
                assert _lib.query("vgposp_potrf_workspace_bytes", n) == want
            assert _lib.query("vgposp_greedy_workspace_bytes", 65536, 50) == \
                (PARENT_GREEDY_65536_50_ABSENT if absent else PARENT_GREEDY_65536_50)
        finally:
            _lib.call("vgposp_gemm_emulation_set_unavailable", 0)


def test_bad_block_width_is_rejected():
    from vgposp_amd import _lib
    assert _lib.load().vgposp_gemm_emulation_set_tri_block(100) != 0
    assert _lib.load().vgposp_gemm_emulation_set_tri_block(-128) != 0
