#!/bin/bash
# One gpurun call: GPU test suite, a validated bench.py run, then the A/B of
# the working-tree build against every variant in cuda_mapreduce_amd/lib/variants
# (end-to-end GB/s, interleaved) and their kernel times.
#   tools/check_ab.sh [TAG]      (REPS=3 interleaved bench runs per build)
export TMPDIR=/tmp
export WC_OUT=${WC_OUT:-out}  # where this script keeps its results
mkdir -p "$WC_OUT"
TAG=${1:-ab}
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread \
  > $WC_OUT/${TAG}_gtest.log 2>&1
rc=$?
tail -4 $WC_OUT/${TAG}_gtest.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "gpu tests rc=$rc: stopping"; exit 1; fi
timeout -k 10 300 python bench.py --full --steps 200 --warmup 10 > $WC_OUT/${TAG}_bench.json 2> $WC_OUT/${TAG}_bench.err
rc=$?
cut -c1-400 $WC_OUT/${TAG}_bench.json; tail -3 $WC_OUT/${TAG}_bench.err
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "bench rc=$rc: stopping"; exit 1; fi
REPS=${REPS:-3} bash tools/vbench.sh || exit 1
bash tools/vprof.sh
