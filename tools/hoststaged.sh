#!/bin/bash
# host-staged config on one GPU: native pinned pool (build time, peak RSS) + replay over PCIe, oracle-validated
export TMPDIR=/tmp
export WC_OUT=${WC_OUT:-out}  # where this script keeps its results
mkdir -p "$WC_OUT"
timeout -k 10 300 python bench.py --full --config 1tb-8gpu-host-staged --gpus 1 --gb-per-gpu ${GB:-16} --steps 2 --warmup 1 \
  > $WC_OUT/hs.json 2> $WC_OUT/hs.err || { tail -5 $WC_OUT/hs.err; exit 1; }
python3 -c "
import json; d=json.loads(open('$WC_OUT/hs.json').read())
print('host-staged', d['value'], 'GB/s', d['ms_per_step'], 'ms valid', d['validated'], d.get('validation'), d.get('host_pool'))"
