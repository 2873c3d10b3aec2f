#!/bin/bash
# End-to-end bench.py GB/s of the default build and every variant in
# cuda_mapreduce_amd/lib/variants, interleaved (A B C A B C ...) REPS times,
# 50 timed steps each; prints every run and the median per build.
# tools/vbench.sh [bench args]   (REPS=3 by default)
export TMPDIR=/tmp
export WC_OUT=${WC_OUT:-out}  # where this script keeps its results
mkdir -p "$WC_OUT"
REPS=${REPS:-3}
libs="cuda_mapreduce_amd/lib/libwc.so $(ls cuda_mapreduce_amd/lib/variants/*.so 2>/dev/null)"
: > $WC_OUT/vb_all.txt
for r in $(seq $REPS); do
  for so in $libs; do
    n=$(basename $so .so)
    WC_LIB=$PWD/$so timeout -k 10 150 python3 bench.py --full --no-oracle --steps 50 --warmup 10 "$@" > $WC_OUT/vb_$n.json 2> $WC_OUT/vb_$n.err
    rc=$?
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "FAILED $so rc=$rc"; tail -3 $WC_OUT/vb_$n.err; exit 1; fi
    python3 -c "
import json; d=[json.loads(l) for l in open('$WC_OUT/vb_$n.json') if l.startswith('{')][-1]
print('$n', d['value'])" >> $WC_OUT/vb_all.txt
  done
done
python3 - "$*" <<'PY'
import os
import collections, statistics, sys
runs = collections.defaultdict(list)
for line in open(os.environ["WC_OUT"] + "/vb_all.txt"):
    n, v = line.split()
    runs[n].append(float(v))
for n, v in runs.items():
    print("%-14s median %7.1f GB/s  runs %s  %s" % (n, statistics.median(v), " ".join("%.1f" % x for x in v), sys.argv[1]))
PY
