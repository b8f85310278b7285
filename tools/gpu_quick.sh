#!/bin/bash
# quick loop: GEMM / LN op tests, then two default benches with the class table.  Usage: tools/gpu_quick.sh TAG [pytest -k expr]
set -o pipefail
TAG=${1:-quick}
KEXPR=${2:-"gemm_nt or layernorm"}
ROOT=$(pwd)
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
python -m pytest tests/test_hip_ops.py -m gpu -x -q -k "$KEXPR" > $OUT/pytest_ops.log 2>&1 || { tail -30 $OUT/pytest_ops.log; exit 1; }
tail -1 $OUT/pytest_ops.log
for rep in 1 2; do
  python bench.py --full --steps 15 --warmup 4 --no-cpu-baseline --no-dense-compare > $OUT/bench_$rep.json 2> $OUT/bench_$rep.err || { tail -5 $OUT/bench_$rep.err; exit 1; }
  python - $OUT/bench_$rep.json <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
cl = d["roofline"]["classes"]
print(f"{d['ms_per_step']:7.3f} ms/step  loss {d['config']['loss']}  sum of classes {sum(c['ms_per_step'] for c in cl):.2f}")
for c in cl[:14]:
    print(f"   {c['kernel'][:44]:44s} {c['launches_per_step']:5.0f} x {c['avg_us']:7.1f} us = {c['ms_per_step']:.3f} ms  {c['tflops']:7.0f} TF/s {c['gbps']:6.0f} GB/s")
PY
done
