#!/bin/bash
# round 3, session A: XCD-owned walk of the persistent NT GEMM -- parity, step A/B, FETCH_SIZE A/B, idle trace
set -o pipefail
TAG=${1:-r3a}
ROOT=$(pwd)
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
python -m pytest tests/test_hip_ops.py -m gpu -x -q -k "gemm_nt" > $OUT/pytest_nt.log 2>&1 || { tail -20 $OUT/pytest_nt.log; exit 1; }
tail -2 $OUT/pytest_nt.log
tools/gpu_ab.sh $OUT "CE_NT_CHUNK=0" "CE_NT_CHUNK=-1" "CE_NT_CHUNK=5" "CE_NT_CHUNK=0" "CE_NT_CHUNK=-1" || exit 1
BARGS="--single-stream --no-cpu-baseline --no-roofline --no-dense-compare --steps 3 --warmup 1"
cd /tmp
CE_NT_CHUNK=0 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch_old --output-format csv -- python3 $ROOT/bench.py $BARGS > $OUT/pmc_fetch_old.log 2>&1 || exit 1
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch_new --output-format csv -- python3 $ROOT/bench.py $BARGS > $OUT/pmc_fetch_new.log 2>&1 || exit 1
rocprofv3 --kernel-trace -d $OUT/trace --output-format csv -- python3 $ROOT/bench.py --no-cpu-baseline --no-roofline --no-dense-compare --steps 10 --warmup 3 > $OUT/trace_bench.log 2>&1 || exit 1
cd $ROOT
echo "== FETCH, launch-wide walk (CE_NT_CHUNK=0)"; python3 tools/pmc_fetch_only.py $OUT/pmc_fetch_old nt160p | tee $OUT/fetch_old.txt
echo "== FETCH, XCD-owned walk"; python3 tools/pmc_fetch_only.py $OUT/pmc_fetch_new nt160p | tee $OUT/fetch_new.txt
python3 tools/trace_idle.py $OUT/trace | tee $OUT/trace_idle.txt
rm -rf $OUT/pmc_fetch_old $OUT/pmc_fetch_new $OUT/trace
