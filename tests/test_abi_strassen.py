"""Workspace queries of the Strassen setting (host-only: the library loads without a GPU)."""
import ctypes

from vgposp_amd import _lib

q = _lib.query


def _get():
    md, lv = ctypes.c_int64(), ctypes.c_int()
    _lib.call("vgposp_potrf_strassen", ctypes.byref(md), ctypes.byref(lv))
    return md.value, lv.value


def test_strassen_workspace_queries():
    old = _get()
    try:
        _lib.call("vgposp_potrf_set_strassen", 512, 0)
        assert _get() == (512, 0)
        base = {n: q("vgposp_potrf_workspace_bytes", n) for n in (640, 896, 1024, 2048)}
        greedy0 = q("vgposp_greedy_workspace_bytes", 2048, 10)
        base16k = q("vgposp_potrf_workspace_bytes", 16384)
        _lib.call("vgposp_potrf_set_strassen", 512, 2)
        # grows only for n >= 2 min_dim with levels > 0, and only where a plain product of the
        # recursion is eligible (none at n = 1024: its largest are 512 x 256 x 256); the greedy
        # workspace follows
        for n, b in base.items():
            grown = q("vgposp_potrf_workspace_bytes", n)
            assert (grown > b) if n >= 2048 else (grown == b), (n, grown, b)
        # n = 2048: the largest need is the SYRK's plain part, 512 x 512 x 1024, one level (its
        # quarters are 256 < min_dim): 256 x 512 + 512 x 256 doubles
        grow = q("vgposp_potrf_workspace_bytes", 2048) - base[2048]
        assert grow == 8 * 2 * 256 * 512
        assert q("vgposp_greedy_workspace_bytes", 2048, 10) - greedy0 == grow
        _lib.call("vgposp_potrf_set_strassen", 8192, 2)
        assert q("vgposp_potrf_workspace_bytes", 16384) == base16k  # nothing eligible: classical
        _lib.call("vgposp_potrf_set_strassen", 512, 2)
        # one A-side and one B-side temporary per level taken
        assert q("vgposp_gemm_strassen_workspace_bytes", 1024, 1024, 1024, 1) == 8 * 2 * 512 * 512
        assert q("vgposp_gemm_strassen_workspace_bytes", 1024, 1024, 1024, 2) == \
            8 * 2 * (512 * 512 + 256 * 256)
        assert q("vgposp_gemm_strassen_workspace_bytes", 768, 512, 1024, 2) == \
            8 * (384 * 512 + 512 * 256)   # 384 is no multiple of 256: one level
        assert q("vgposp_gemm_strassen_workspace_bytes", 1024, 1024, 384, 2) == 0
        assert q("vgposp_gemm_strassen_workspace_bytes", 1024, 1024, 1024, 0) == 0
        # batched: one recursion at the batched per-matrix stride (16 MiB of split-K partials, no
        # Strassen scratch), never below one single-matrix workspace
        per = base[2048] - 8 * ((8 << 20) - (2 << 20))
        one = q("vgposp_potrf_workspace_bytes", 2048)
        assert q("vgposp_potrf_batched_workspace_bytes", 2048, 1) == max(per, one)
        assert q("vgposp_potrf_batched_workspace_bytes", 2048, 3) == max(3 * per, one)
        # bad settings are rejected and leave the setting alone
        assert _lib.load().vgposp_potrf_set_strassen(300, 1) == -1
        assert _lib.load().vgposp_potrf_set_strassen(512, 3) == -2
        assert _get() == (512, 2)
    finally:
        _lib.call("vgposp_potrf_set_strassen", *old)
