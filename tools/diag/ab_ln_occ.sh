#!/bin/bash
# LayerNorm ablations (timing only where the flag says so): compile-time flag sets of layernorm.hip against the default build, on the step.
#   tools/diag/ab_ln_occ.sh OUT_DIR "-DFLAG ..." ...
OUT=${1:?usage: see above}; shift; mkdir -p $OUT
i=0
for flags in "-DCE_DIAG_NONE" "$@"; do
  i=$((i+1))
  hipcc -O3 -std=c++17 -fPIC -munsafe-fp-atomics -w --offload-arch=gfx950 $flags -x hip -c clip_event_amd/csrc/layernorm.hip -o /tmp/ln_$i.o || exit 1
  hipcc -shared -fPIC --offload-arch=gfx950 -o /tmp/libce_ln_$i.so /tmp/ln_$i.o $(ls clip_event_amd/build/*.o | grep -v "/layernorm.hip.o") || exit 1
done
for rep in 1 2; do
i=0
for flags in "-DCE_DIAG_NONE" "$@"; do
  i=$((i+1))
  CE_DIAG_LIB=/tmp/libce_ln_$i.so python tools/diag/bench_with_lib.py --full --steps 15 --warmup 4 --no-cpu-baseline --no-dense-compare > $OUT/b.json 2>$OUT/b.err || { tail -3 $OUT/b.err; exit 1; }
  python - "$flags" $OUT/b.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
cl = {c["kernel"]: c for c in d["roofline"]["classes"]}
print(f"{sys.argv[1]:36s} {d['ms_per_step']:7.3f} ms/step  ln_bwd {cl['ln_bwd']['ms_per_step']:.3f} ms ({cl['ln_bwd']['avg_us']:.1f} us)  ln_fwd {cl['ln_fwd']['ms_per_step']:.3f}")
PY
done
done
