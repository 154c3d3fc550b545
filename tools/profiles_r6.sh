#!/bin/bash
# Round-6 profiling recipe for one bench workload (run via gpurun from the repo root): the bench
# line, a kernel trace, and the PMC passes of tools/profiles_run.sh (HBM bytes, instruction mix,
# VALU issue with GRBM_GUI_ACTIVE for the clock), each rocprofv3 pass under its own time limit;
# the chain stops at the first failure.
#   tools/profiles_r6.sh OUT "bench args" [KERNEL SCHEME LAST]
#   e.g. tools/profiles_r6.sh gpurun_out/p_rats_ir "--workload rats_ir" mmb_ir_jit_kernel reference 4
# The raw rocprofv3 CSVs are summarised on the box (tools/profiles_pmc_summary.py -> OUT/s_*) and
# removed, so the session's output stays far below gpurun's 64 MiB copy-back limit.
set -e
OUT=$1
BARGS=$2
KERNEL=${3:-sweep_kernel}
SCHEME=${4:-gibbs_amm}
LAST=${5:-10}
mkdir -p $OUT
export TMPDIR=/tmp
ARGS="--no-cpu-baseline $BARGS"
timeout -k 10 400 python bench.py --full $BARGS > $OUT/bench.json 2> $OUT/bench.err
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -o run -- python3 bench.py $ARGS > $OUT/trace.log 2>&1
timeout -k 10 400 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc_fetch -o run -- python3 bench.py $ARGS > $OUT/pmc_fetch.log 2>&1
timeout -k 10 400 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc_write -o run -- python3 bench.py $ARGS > $OUT/pmc_write.log 2>&1
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VALU_FMA_F64 SQ_INSTS_VALU_MUL_F64 SQ_INSTS_VALU_ADD_F64 SQ_INSTS_VALU_TRANS_F64 SQ_INSTS_VALU_INT32 SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $OUT/pmc_sq1 -o run -- python3 bench.py $ARGS > $OUT/pmc_sq1.log 2>&1
timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_WAIT_ANY SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INSTS_VMEM_RD GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_sq2 -o run -- python3 bench.py $ARGS > $OUT/pmc_sq2.log 2>&1
python3 tools/profiles_pmc_summary.py $OUT $OUT/s --last $LAST --kernel $KERNEL --scheme $SCHEME > $OUT/summary.log 2>&1
find $OUT -name "*.csv" ! -name "run_kernel_stats.csv" -delete
find $OUT -name "*.db" -delete
echo "profiles done: $OUT"
