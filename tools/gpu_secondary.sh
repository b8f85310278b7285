#!/bin/bash
# secondary workloads for profiles/: ViT-L/14@336 B = 32 in bf16 and with the fp8 operand path (same box, twice each), config 3's
# shape on one GPU (B = 256 x 5 descriptions) and config 3's per-rank size (B = 512 x 5).    tools/gpu_secondary.sh TAG
TAG=${1:-sec}; OUT=gpurun_out/$TAG; mkdir -p $OUT
for rep in 1 2; do
  python tools/bench_arch.py vit_l14_336 > $OUT/vitl_bf16_$rep.log 2>&1 || { tail -3 $OUT/vitl_bf16_$rep.log; exit 1; }
  python tools/bench_arch.py vit_l14_336 --fp8=3 > $OUT/vitl_fp8_$rep.log 2>&1 || { tail -3 $OUT/vitl_fp8_$rep.log; exit 1; }
  tail -2 $OUT/vitl_bf16_$rep.log; tail -2 $OUT/vitl_fp8_$rep.log
done
python bench.py --full --descriptions 5 --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_config3_shape.json 2>$OUT/c3.err || { tail -3 $OUT/c3.err; exit 1; }
cut -c1-250 $OUT/bench_config3_shape.json
python bench.py --full --batch 512 --descriptions 5 --steps 6 --warmup 2 --no-cpu-baseline --no-dense-compare > $OUT/bench_config3_per_rank.json 2>$OUT/c3r.err || { tail -3 $OUT/c3r.err; exit 1; }
cut -c1-250 $OUT/bench_config3_per_rank.json
