#!/bin/bash
# Round-end validation of the shipped build: the whole GPU suite, the default
# bench (validated), kernel statistics at v100k and v1m, step timelines.
export TMPDIR=/tmp
export WC_OUT=${WC_OUT:-out}  # where this script keeps its results
mkdir -p "$WC_OUT"
mkdir -p $WC_OUT/final
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $WC_OUT/final/gtest.log 2>&1 || { tail -20 $WC_OUT/final/gtest.log; exit 1; }
tail -1 $WC_OUT/final/gtest.log
timeout -k 10 300 python3 bench.py --full > $WC_OUT/final/bench_default.json 2> $WC_OUT/final/bench_default.err || { tail -5 $WC_OUT/final/bench_default.err; exit 1; }
python3 -c "import json; d=json.loads(open('$WC_OUT/final/bench_default.json').read().strip().splitlines()[-1]); print('bench', d['value'], d['ms_per_step'], d['steps'], d['validated'], d['stages']['device_ms'])"
bash tools/kstats.sh final_v100k > $WC_OUT/final/kstats_v100k.txt 2>&1 || exit 1
bash tools/kstats.sh final_v1m --vocab 1000000 > $WC_OUT/final/kstats_v1m.txt 2>&1 || exit 1
head -12 $WC_OUT/final/kstats_v100k.txt
bash tools/step_timelines.sh > $WC_OUT/final/step_timelines.txt 2>&1 || exit 1
grep -E "==|step span" $WC_OUT/final/step_timelines.txt
