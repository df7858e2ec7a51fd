#!/bin/bash
# trtri with the split triangular-A TRMM: parity (GEMM/potrf/placement + full-size 65k checks),
# then the 65k placement step
# Run from the repository root; results go to $OUT (default build/ab).
set -e
O=${OUT:-build/ab}; mkdir -p $O
timeout -k 10 600 python -u -m pytest tests/test_gpu_linalg.py tests/test_gpu_placement.py tests/test_gpu_fullsize.py tests/test_gpu_gp.py -x -q --timeout 300 --timeout-method thread > $O/tc_tests.log 2>&1
echo ok tests
timeout -k 10 300 python -u bench.py --full --no-cpu --no-vgp --no-c2 --steps 2 --warmup 1 > $O/tc_bench.log 2>&1
echo ok bench
