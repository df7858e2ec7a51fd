"""The speculation setting of the greedy rounds at the ABI (host-only: the library loads without
a GPU)."""
from vgposp_amd import _lib

q = _lib.query


def test_speculation_setting_and_workspace():
    lib = _lib.load()
    for sym in ("vgposp_greedy_set_speculation", "vgposp_greedy_speculation",
                "vgposp_greedy_spec_stats", "vgposp_greedy_spec_table"):
        assert hasattr(lib, sym), sym
        assert sym in _lib.header_symbols()
    old = lib.vgposp_greedy_speculation()
    assert old in (1, 2, 4, 8)
    try:
        sizes = {}
        for w in (1, 2, 4, 8):
            _lib.call("vgposp_greedy_set_speculation", w)
            assert lib.vgposp_greedy_speculation() == w
            # rejected widths leave the setting alone
            for bad in (0, 3, 16, -1):
                assert lib.vgposp_greedy_set_speculation(bad) == -1
            assert lib.vgposp_greedy_speculation() == w
            # a caller who queries first and changes the width later stays correct
            sizes[w] = [q("vgposp_greedy_workspace_bytes", n, k)
                        for n, k in ((64, 4), (1040, 6), (2048, 10), (65536, 50))]
        assert sizes[1] == sizes[2] == sizes[4] == sizes[8]
        # the growth over the classic layout at the benchmark's size: seven partial slices of
        # ceil(n / 512) x n, eight right-hand sides, 4 k columns and the table — under 1 GiB
        n, k = 65536, 50
        spec = 8 * (7 * (n // 512) * n + 8 * n + 4 * k * n) + 8 * (32 + 8 * k) + n
        assert spec < 1 << 30
        assert sizes[8][3] > spec
    finally:
        _lib.call("vgposp_greedy_set_speculation", old)
