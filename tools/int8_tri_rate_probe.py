"""The int8 x int8 -> int32 rate of hipBLASLt (torch._int_mm) on the staircase shapes of the
structured products (SYRK lower, tri-B, tri-A) of the 65k step: sixteen distinct planes, both
operands K-contiguous views (leading dimension 32,768) of two plane pools, as the drivers of
gemm_emul.hip address them.  Writes one JSON (profiles/gemm_emul_tri_rates.json)."""
import json
import sys
import time

import torch

NP, LD = 16, 32768


def rate(pa, pb, m, n, k, a_k0=0, b_k0=0, reps=2):
    """(m x k)(n x k)^T on sixteen planes; ms for the sixteen and POPS."""
    def run():
        for t in range(NP):
            torch._int_mm(pa[t, :m, a_k0:a_k0 + k], pb[t, :n, b_k0:b_k0 + k].t())
    run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    return {"m": m, "n": n, "k": k, "ms": round(ms, 3), "pops": round(NP * 2.0 * m * n * k / ms / 1e12, 3)}


def main(out_path):
    pa = torch.randint(-128, 128, (NP, LD, LD), dtype=torch.int8, device="cuda")
    pb = torch.randint(-128, 128, (NP, LD, LD), dtype=torch.int8, device="cuda")
    out = {"syrk_rows": [], "trib_columns": [], "tria_rows": []}
    for b in (1024, 2048, 4096):
        for K in (16384, 32768):
            nb = K // b  # the SYRK's order equals its depth at both levels of the 65k step
            for i in (0, nb // 2, nb - 1):
                out["syrk_rows"].append(dict(b=b, block_row=i, **rate(pa, pa, b, (i + 1) * b, K)))
        for n in (16384, 32768):
            for kk in (b, n // 2, n):
                out["trib_columns"].append(dict(b=b, **rate(pa, pb, n, b, kk, n - kk, n - kk)))
                out["tria_rows"].append(dict(b=b, **rate(pa, pb, b, n, kk)))
        print(json.dumps({"b": b, "done": True}), flush=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1])
