#!/bin/bash
# A/B of the GEMM tile-group size (row tiles per XCD band): the 16384^3 layout sweep and the
# 65k placement step for the default build and each tools/variants/lib_group*.so
# Run from the repository root; results go to $OUT (default build/ab).
set -e
O=${OUT:-build/ab}; mkdir -p $O
for lib in default tools/variants/lib_group*.so; do
  if [ $lib = default ]; then unset VGPOSP_LIB; else export VGPOSP_LIB=$PWD/$lib; fi
  echo "== $lib" >> $O/ab4_layouts.txt
  timeout -k 10 300 python -u tools/gemm_layouts.py >> $O/ab4_layouts.txt 2>&1
  timeout -k 10 300 python -u bench.py --full --no-cpu --no-vgp --no-c2 --steps 2 --warmup 1 2>&1 | grep '^{' | cut -c1-200 >> $O/ab4_layouts.txt
  echo ok $lib
done
