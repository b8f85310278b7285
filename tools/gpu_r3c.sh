#!/bin/bash
# round 3, session C: fp16 residual stream -- op tests, model tests in both stream formats, step time A/B
set -o pipefail
TAG=${1:-r3c}
ROOT=$(pwd)
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
true
true
python -m pytest tests/test_hip_ops.py tests/test_model_gpu.py -m gpu -x -q -s -k "layernorm or tiny or region or noise_floor" > $OUT/pytest_model.log 2>&1 || { tail -60 $OUT/pytest_model.log; exit 1; }
grep -E "noise floor|passed|failed|fp16 stream|config 3 per rank|gradient rel-L2" $OUT/pytest_model.log | tail -20
for rep in 1 2; do
for s16 in 0 1; do
  CE_STREAM16=$s16 python bench.py --full --steps 15 --warmup 4 --no-cpu-baseline --no-dense-compare > $OUT/bench_s$s16.json 2> $OUT/bench_s$s16.err || { tail -5 $OUT/bench_s$s16.err; exit 1; }
  python - "CE_STREAM16=$s16" $OUT/bench_s$s16.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
cl = d["roofline"]["classes"]
pick = {c["kernel"]: c for c in cl}
def g(sub):
    return sum(c["ms_per_step"] for c in cl if sub in c["kernel"])
print(f"{sys.argv[1]:16s} {d['ms_per_step']:7.3f} ms/step  loss {d['config']['loss']}  ln_fwd {g('ln_fwd'):.3f} ln_bwd {g('ln_bwd'):.3f} resid-epilogue GEMMs {g('BIAS_RESID'):.3f}  all classes {sum(c['ms_per_step'] for c in cl):.2f}", flush=True)
PY
done
done
