#!/bin/bash
# round 3, session B: new parity tests + step timeline
set -o pipefail
TAG=${1:-r3b}
ROOT=$(pwd)
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
python -m pytest tests/test_hip_ops.py tests/test_model_gpu.py -m gpu -x -q -s -k "vit_l14 and 3" > $OUT/pytest_new.log 2>&1 || { tail -40 $OUT/pytest_new.log; exit 1; }
grep -E "^\[c4|^\[vit-l|passed|failed" $OUT/pytest_new.log | tail -30
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err || { tail $OUT/bench.err; exit 1; }
cut -c1-400 $OUT/bench.json
cd /tmp
rocprofv3 --kernel-trace -d $OUT/trace --output-format csv -- python3 $ROOT/bench.py --no-cpu-baseline --no-roofline --no-dense-compare --steps 10 --warmup 3 > $OUT/trace_bench.log 2>&1 || exit 1
cd $ROOT
python3 tools/trace_idle.py $OUT/trace $OUT/timeline_step.txt | tee $OUT/trace_idle.txt
rm -rf $OUT/trace
