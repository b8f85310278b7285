#!/bin/bash
# A/B of the epilogue store cache policy (CE_EPI_ST_AUX: 0 plain, 16 sc1, 2 nt) x tile walk (CE_NT_CHUNK 0 / -1) in the step,
# plus a FETCH_SIZE pass for the sc1 + XCD-owned combination.  Usage: tools/diag/ab_store_policy.sh TAG
set -o pipefail
TAG=${1:-stpol}
ROOT=$(pwd)
OUT=$ROOT/gpurun_out/$TAG
mkdir -p $OUT
export TMPDIR=/tmp
for aux in 0 16 2; do
  ( hipcc -O3 -std=c++17 -fPIC -munsafe-fp-atomics -w --offload-arch=gfx950 -DCE_EPI_ST_AUX=$aux -x hip -c clip_event_amd/csrc/gemm.hip -o /tmp/st_$aux.o &&
    hipcc -shared -fPIC --offload-arch=gfx950 -o /tmp/libce_st_$aux.so /tmp/st_$aux.o $(ls clip_event_amd/build/*.o | grep -v "/gemm.hip.o") ) &
done
wait
ls -la /tmp/libce_st_*.so || exit 1
for rep in 1 2; do
 for chunk in 0 -1; do
  for aux in 0 16 2; do
    CE_NT_CHUNK=$chunk CE_DIAG_LIB=/tmp/libce_st_$aux.so python tools/diag/bench_with_lib.py --full --steps 15 --warmup 4 --no-cpu-baseline --no-dense-compare > $OUT/st_${aux}_${chunk}_$rep.json 2> $OUT/st.err || { tail -5 $OUT/st.err; exit 1; }
    python - "aux=$aux chunk=$chunk" $OUT/st_${aux}_${chunk}_$rep.json <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
cl = {c["kernel"].split(" ")[-1] + ("p" if "160p" in c["kernel"] else ""): c for c in d["roofline"]["classes"] if "nt160" in c["kernel"]}
print(f"{sys.argv[1]:22s} {d['ms_per_step']:7.3f} ms/step  " + "  ".join(f"{k} {v['ms_per_step']:.3f}" for k, v in cl.items()), flush=True)
PY
  done
 done
done
BARGS="--single-stream --no-cpu-baseline --no-roofline --no-dense-compare --steps 3 --warmup 1"
cd /tmp
CE_DIAG_LIB=/tmp/libce_st_16.so rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch_sc1 --output-format csv -- python3 $ROOT/tools/diag/bench_with_lib.py $BARGS > $OUT/pmc_fetch_sc1.log 2>&1 || exit 1
CE_DIAG_LIB=/tmp/libce_st_16.so rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write_sc1 --output-format csv -- python3 $ROOT/tools/diag/bench_with_lib.py $BARGS > $OUT/pmc_write_sc1.log 2>&1 || exit 1
cd $ROOT
python3 tools/pmc_traffic.py $OUT/pmc_fetch_sc1 $OUT/pmc_write_sc1 > $OUT/pmc_traffic_sc1_xcd.json
python3 tools/pmc_fetch_only.py $OUT/pmc_fetch_sc1 nt160 | tee $OUT/fetch_sc1_xcd.txt
rm -rf $OUT/pmc_fetch_sc1 $OUT/pmc_write_sc1
