"""One greedy workspace driven through the C-ABI directly: the helper of
tests/test_gpu_greedy_state.py and tests/test_gpu_greedy_spec.py."""
import ctypes

import numpy as np

SENTINEL = 12345.678  # fills what surrounds Sigma in a padded buffer: read as data it is >> tol
RC = 512              # rows per chunk of the mat-vec (csrc/greedy.hip)
PARAMS = (0.0, 1e-8, np.inf)   # (jitter, threshold, cache_init) of placement_algorithm2
KEYS = ("delta", "piv", "xcol", "cache", "selected", "sel_delta", "evals", "state")


def _call(name, *args):
    from vgposp_amd._lib import call
    return call(name, *args)


def _stream():
    from vgposp_amd.linalg import _stream
    return _stream()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class Greedy:
    """Sigma = K[:n, :n] sits in a buffer of row pitch lda that starts `shift` doubles into its
    allocation, everything around it holds SENTINEL; the workspace starts as NaN bytes, so
    anything read before it is written shows."""

    def __init__(self, K, n, kmax, params=PARAMS, lda=None, shift=0):
        import torch
        from vgposp_amd._lib import query
        self.n, self.kmax, self.lda, self.shift = int(n), int(kmax), int(lda or n), int(shift)
        self.params = tuple(float(p) for p in params)
        self.buf = torch.empty(self.shift + self.n * self.lda, dtype=torch.float64, device="cuda")
        assert self.buf.data_ptr() % 16 == 0
        self.S = ctypes.c_void_p(self.buf.data_ptr() + 8 * self.shift)
        self.load(K)
        self.ws = torch.empty(query("vgposp_greedy_workspace_bytes", self.n, self.kmax),
                              dtype=torch.uint8, device="cuda")
        self.ws.fill_(0xFF)
        self.info = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.selected = torch.full((self.kmax,), -1, dtype=torch.int64, device="cuda")
        self.sel_delta = torch.zeros(self.kmax, dtype=torch.float64, device="cuda")
        self.evals = torch.zeros(self.kmax, dtype=torch.int64, device="cuda")
        self.delta, self.piv = self._views("vgposp_greedy_buffers", self.n, None)
        assert self.piv.numel() == 2 + 2 * self.kmax
        self.xcol, = self._views("vgposp_greedy_xcol", self.n)
        self.cache, = self._views("vgposp_greedy_cache", self.n)
        # prm, sdiag, nom, prec, delta, cache, W, V: everything ahead of the mat-vec partials,
        # which sit (256-byte aligned, ceil(n / RC) rows of n) right ahead of xcol
        part = -(-self.n // RC) * self.n * 8
        self.state = self.ws[:self.xcol.data_ptr() - self.ws.data_ptr()
                             - (part + 255) // 256 * 256]
        # the speculation's table: cached column and fill round per slot
        self.tcol, self.tround = self._views("vgposp_greedy_spec_table", None, None,
                                             dtype="int64")
        self.slots = self.tcol.numel()
        self._keep = []

    def load(self, K):
        import torch
        host = np.full(self.shift + self.n * self.lda, SENTINEL)
        host[self.shift:].reshape(self.n, self.lda)[:, :self.n] = K[:self.n, :self.n]
        self.host0 = host
        self.src = torch.as_tensor(host).cuda()
        self.buf.copy_(self.src)

    def _views(self, entry, *counts, dtype="float64"):
        """The pointers a query entry returns, as views of the workspace; a count of None is
        the entry's trailing int64 output."""
        import torch
        ptrs, last = [ctypes.c_void_p() for _ in counts], ctypes.c_int64()
        tail = [ctypes.byref(last)] if None in counts else []
        _call(entry, self._ws(), self.n, self.kmax, *[ctypes.byref(p) for p in ptrs], *tail)
        out = []
        for ptr, count in zip(ptrs, counts):
            count = last.value if count is None else count
            off = ptr.value - self.ws.data_ptr()
            assert 0 <= off and off + 8 * count <= self.ws.numel()
            out.append(self.ws[off:off + 8 * count].view(getattr(torch, dtype)))
        return out

    def _ws(self):
        return ctypes.c_void_p(self.ws.data_ptr())

    def _sigma(self):
        return self.S, self.n, self.lda, self.kmax

    def _tail(self):
        return self._ws(), self.ws.numel(), _stream()

    def _picks(self):
        return _p(self.selected), _p(self.sel_delta), _p(self.evals)

    def init(self):
        _call("vgposp_greedy_init_ex", *self._sigma(), *self.params, _p(self.info), *self._tail())
        return self

    def mask(self, blocked):
        import torch
        allowed = torch.as_tensor((~np.asarray(blocked, dtype=bool)).astype(np.uint8)).cuda()
        self._keep.append(allowed)
        _call("vgposp_greedy_mask", self._ws(), self.n, self.kmax, _p(allowed), _stream())

    def condition(self, placed, k, batch):
        import torch
        from vgposp_amd._lib import query
        pl = torch.as_tensor(np.asarray(placed, dtype=np.int64)).cuda()
        nbytes = query("vgposp_greedy_condition_workspace_bytes", self.n, batch)
        assert nbytes > 0
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        scratch.fill_(0xFF)
        self._keep += [pl, scratch]
        _call("vgposp_greedy_condition", *self._sigma(), len(placed), k, batch, _p(pl),
              _p(self.selected), self._ws(), self.ws.numel(), _p(scratch), scratch.numel(),
              _stream())

    def step(self, r, lazy):
        _call("vgposp_greedy_step", *self._sigma(), r, int(lazy), *self._picks(), *self._tail())

    def update(self, r, c0, c1, extract=1):
        _call("vgposp_greedy_update_ex", *self._sigma(), r, c0, c1, _p(self.selected),
              int(extract), *self._tail())

    def select(self, r, lazy, c0, c1):
        _call("vgposp_greedy_select", self.n, self.kmax, r, int(lazy), c0, c1, *self._picks(),
              *self._tail())

    def extract(self, r, own0, own1):
        _call("vgposp_greedy_extract", *self._sigma(), r, own0, own1, _p(self.selected),
              *self._tail())

    def read(self):
        rec = {k: getattr(self, k).cpu().numpy().copy() for k in KEYS}
        assert int(self.info.cpu()[0]) == 0
        return rec

    def matrix(self):
        return self.buf.cpu().numpy().copy()

    def stats(self):
        """(passes, hits, cached) of the run so far."""
        import torch
        torch.cuda.synchronize()
        v = [ctypes.c_int64(-1) for _ in range(3)]
        _call("vgposp_greedy_spec_stats", self._ws(), self.n, self.kmax,
              *[ctypes.byref(x) for x in v])
        return tuple(x.value for x in v)

    def table(self):
        """[(column, fill round)] of the cached columns, in slot order."""
        cached = self.stats()[2]
        assert 0 <= cached <= self.slots
        return list(zip((int(c) for c in self.tcol[:cached].cpu()),
                        (int(r) for r in self.tround[:cached].cpu())))
