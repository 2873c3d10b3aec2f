#!/bin/bash
# torch.distributed.run launcher path of bench.py at --nproc-per-node 1 with the
# RCCL communicator forced on (WC_MERGE_ALWAYS=1), once per merge protocol.
export TMPDIR=/tmp
export WC_OUT=${WC_OUT:-out}  # where this script keeps its results
mkdir -p "$WC_OUT"
for m in shuffle dense; do
  WC_MERGE_ALWAYS=1 timeout -k 10 240 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 \
    --master-addr 127.0.0.1 --master-port $((29600 + RANDOM % 200)) bench.py --full --gpus 1 --steps 10 --warmup 2 \
    --merge $m > $WC_OUT/dist_$m.json 2> $WC_OUT/dist_$m.err || { tail -20 $WC_OUT/dist_$m.err; exit 1; }
  cut -c1-300 $WC_OUT/dist_$m.json
done
