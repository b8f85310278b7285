#!/bin/bash
# same-box A/B of prebuilt library variants on the step: tools/diag/ab_libs.sh OUT_DIR LIB1 LIB2 ... (each run twice, interleaved)
OUT=${1:?usage: see above}; shift; mkdir -p $OUT
for rep in 1 2; do
  for lib in "$@"; do
    CE_DIAG_LIB=$lib python tools/diag/bench_with_lib.py --full --steps 15 --warmup 4 --no-cpu-baseline --no-dense-compare $BENCH_ARGS > $OUT/ab.json 2>$OUT/ab.err || { tail -3 $OUT/ab.err; exit 1; }
    python - "$lib" $OUT/ab.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
cl = d.get("roofline", {}).get("classes", [])
nt = {c["kernel"].split()[-1] if "gemm_nt160" in c["kernel"] else c["kernel"]: c["ms_per_step"] for c in cl}
keys = ["BF16", "BIAS_RESID_F16", "GELUGRAD_BF16", "BIAS_GELU", "BIAS_BF16"]
print(f"{sys.argv[1][-28:]:28s} {d['ms_per_step']:7.3f} ms/step  " + " ".join(f"{k}={nt.get(k, 0):.3f}" for k in keys) + f"  all {sum(c['ms_per_step'] for c in cl):.2f}")
PY
  done
done
