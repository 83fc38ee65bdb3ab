#!/bin/bash
# Rehearsal of bench.py's multi-rank path on a one-GPU box: torchrun with 2 ranks sharing cuda:0
# (HE_BENCH_SHARED_DEVICE=1: gloo collectives, since RCCL needs one GPU per rank), learner leg
# included (bench.py --full), so the barrier / max-over-ranks timing, the learner's collectives and the
# rank agreement after the learner leg run at world 2.
set -o pipefail
OUT=${HE_RECORD_DIR:-records}  # the log goes where the GPU sessions keep their records
mkdir -p "$OUT"
export TMPDIR=/tmp HE_BENCH_SHARED_DEVICE=1
timeout -k 10 500 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 \
  bench.py --full --gpus 2 --steps 20 --warmup 5 > "$OUT/bench_world2.log" 2>&1
rc=$?
grep "^{" "$OUT/bench_world2.log" | cut -c1-1500
exit $rc
