#!/bin/bash
# A/B of GEMM library variants on one box: parity of the b128 variant, then the 16384^3 layout
# sweep and the 65k placement step for the default build and every tools/variants/*.so
# Run from the repository root; results go to $OUT (default build/ab).
set -e
O=${OUT:-build/ab}; mkdir -p $O
VGPOSP_LIB=$PWD/tools/variants/lib_b128.so timeout -k 10 300 python -u -m pytest tests/test_gpu_linalg.py tests/test_gpu_placement.py -x -q --timeout 200 --timeout-method thread > $O/ab3_tests.log 2>&1
echo ok tests
for lib in default tools/variants/lib_b128.so tools/variants/lib_prio.so tools/variants/lib_b128prio.so; do
  if [ $lib = default ]; then unset VGPOSP_LIB; else export VGPOSP_LIB=$PWD/$lib; fi
  echo "== $lib" >> $O/ab3_layouts.txt
  timeout -k 10 300 python -u tools/gemm_layouts.py >> $O/ab3_layouts.txt 2>&1
  timeout -k 10 300 python -u bench.py --full --no-cpu --no-vgp --no-c2 --steps 2 --warmup 1 2>&1 | grep '^{' | cut -c1-200 >> $O/ab3_layouts.txt
  echo ok $lib
done
