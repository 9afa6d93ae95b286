# Counter passes for the paxos expand kernel (counters with --kernel-trace only, one set per pass).
set -o pipefail
BENCH="$(cd "$(dirname "$0")/.." && pwd)/bench.py"
cd /tmp && export TMPDIR=/tmp
OUT=$GRAFT_REPO_ROOT/gpurun_out/pmc_paxos
mkdir -p $OUT
i=0
while read -r line; do
  [ -z "$line" ] && continue
  i=$((i+1))
  timeout -k 10 180 rocprofv3 --pmc $line --kernel-trace --output-format csv -d $OUT/p$i -o p$i -- python3 "$BENCH" --full --model paxos --steps 1 --warmup 0 --cpu-baseline 0 > $OUT/p$i.log 2>&1 || exit 1
done <<'PASSES'
SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM SQ_INSTS_VALU
SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INST_LEVEL_VMEM SQ_ACTIVE_INST_VALU
TCC_HIT_sum TCC_MISS_sum TCC_EA0_RDREQ_sum TCC_EA0_WRREQ_sum
PASSES
