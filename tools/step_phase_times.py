"""One profiled 65k placement step (the library's per-launch event timing): ms, launches, flops
and bytes of every phase, the fp64 GEMM by class included.  One JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from vgposp_amd import _lib, linalg  # noqa: E402
from vgposp_amd.placement_algorithm2 import GreedyPlacement  # noqa: E402
from vgposp_amd.workloads import placement_split  # noqa: E402

X, ls = placement_split((64, 32, 32), 0)
N, k = len(X), 50
Xd = linalg.as_device(X)
Sigma = torch.empty((N, N), dtype=torch.float64, device="cuda")
g = GreedyPlacement(Sigma, k)


def step():
    linalg.kernel_matrix("eq", Xd, None, 1.0, ls, diag_shift=1e-2 + 1e-6, out=Sigma[None])
    g.run(k)


step()
torch.cuda.synchronize()
g.check()
_lib.prof_enable(True)
step()
torch.cuda.synchronize()
prof = {n: {"ms": v[0], "launches": v[1], "flops": v[2], "bytes": v[3]}
        for n, v in sorted(_lib.prof_dump().items())}
_lib.prof_enable(False)
print(json.dumps(prof))
