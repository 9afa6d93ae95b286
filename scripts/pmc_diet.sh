#!/bin/bash
# Instruction counters of expand_fast on 2pc N=9 for two builds of the engine library, a saved one
# (e.g. the parent commit's, as scripts/gpu_lib_ab.sh takes) and the in-tree build, swapped into place in
# turn: one counters-only rocprofv3 pass each, no tracing beside it, and one --kernel-trace --stats pass
# each in a run of its own. scripts/pmc_diet.py sums the counters over the dispatches of at least
# 100 us (profiles/r08_instruction_diet.txt).
#   scripts/pmc_diet.sh <saved library .so> <output directory>
set -o pipefail
BASE=$(realpath "${1:?saved library}") || exit 1
mkdir -p "${2:?output directory}" && O=$(realpath "$2") || exit 1
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp SR_LIB_DIGEST_CHECK=0
LIB=stateright_amd/libstateright_gpu.so
cp "$LIB" "$O/lib_new.so" || exit 1
cp "$BASE" "$O/lib_base.so" || exit 1
ARGS="--gpus 1 --rm-count 9 --steps 2 --warmup 1"
for v in base new; do
    cp "$O/lib_$v.so" $LIB || exit 1
    timeout -k 10 200 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_INSTS_SALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE SQ_INSTS_LDS --output-format csv -d "$O/pmc_$v" -o p -- python3 bench.py $ARGS > "$O/pmc_$v.log" 2>&1 ||
        { echo "pmc $v failed"; tail -5 "$O/pmc_$v.log"; cp "$O/lib_new.so" $LIB; exit 1; }
    timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt_$v" -o t -- python3 bench.py $ARGS > "$O/kt_$v.log" 2>&1 ||
        { echo "kernel trace $v failed"; tail -5 "$O/kt_$v.log"; cp "$O/lib_new.so" $LIB; exit 1; }
done
cp "$O/lib_new.so" $LIB
rm -f "$O/lib_base.so" "$O/lib_new.so"
python3 scripts/pmc_diet.py "$O" | tee "$O/summary.txt"
