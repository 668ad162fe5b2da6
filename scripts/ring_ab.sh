#!/bin/bash
# ring prefetch in the row-reduction skeleton (HEAD) against batch-then-drain (ab/noring.so): step and streaming rows, C3 and C5's classifier
R=$PWD
OUT_DIR=${OUT_DIR:-results}; mkdir -p "$OUT_DIR"
bash scripts/env_sweep.sh r04k_ring2 "" "MI355_LIB=$R/ab/noring.so"
BENCH_ARGS="--model vgg16_bn --batch 16 --size 512 --dtype fp16" bash scripts/env_sweep.sh r04k_ring2_c5 "" "MI355_LIB=$R/ab/noring.so"
for v in "" "MI355_LIB=$R/ab/noring.so"; do
  echo "== [${v:-defaults}]" >> $OUT_DIR/r04k_ring2.txt
  env $v python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --kernel-table 2>&1 >/dev/null | grep -E "pool2|sum of plan" >> $OUT_DIR/r04k_ring2.txt
  echo "== C5 [${v:-defaults}]" >> $OUT_DIR/r04k_ring2.txt
  env $v python bench.py --full --model vgg16_bn --batch 16 --size 512 --dtype fp16 --steps 10 --warmup 3 --no-cpu-baseline --kernel-table 2>&1 >/dev/null | grep -E "pool2|bn_bwd|sum of plan" >> $OUT_DIR/r04k_ring2.txt
done
cat $OUT_DIR/r04k_ring2.txt $OUT_DIR/r04k_ring2_c5.txt
