#!/bin/bash
# Round-6 final-build session (run via gpurun from the repo root; tools/gsafe.sh semantics: a step
# that fails an ordinary way does not stop the rest, a time limit / abort / fault ends it).
#   tools/final_r6.sh tests|prof|prof_a|prof_b|bench [OUT]
PART=${1:-tests}
OUT=${2:-gpurun_out/final6}
mkdir -p $OUT
export OUT
export TMPDIR=/tmp
case $PART in
tests)
  tools/gsafe.sh \
    "timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $OUT/gpu_tests.log 2>&1" \
    "timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $OUT/smoke.log 2>&1"
  tail -3 $OUT/gpu_tests.log; tail -1 $OUT/smoke.log ;;
prof|prof_a)
  tools/gsafe.sh \
    "tools/profiles_r6.sh $OUT/rats '--steps 200 --warmup 100' sweep_kernel gibbs_amm 10" \
    "tools/profiles_r6.sh $OUT/ref '--scheme reference --steps 200 --warmup 100' sweep_kernel reference 10" \
    "tools/profiles_lg_r6.sh $OUT/lg" ;;&
prof|prof_b)
  tools/gsafe.sh \
    "tools/profiles_r6.sh $OUT/rats_ir '--workload rats_ir' mmb_ir_jit_kernel reference 4" \
    "tools/profiles_r6.sh $OUT/seeds_ir '--workload seeds_ir' mmb_ir_jit_kernel seeds 10" \
    "tools/profiles_r6.sh $OUT/rgir '--workload rats_gibbs_ir' mmb_ir_jit_kernel gibbs_amm 4" ;;
bench)
  run() { n=$1; shift; echo "$n"; timeout -k 10 400 python bench.py --full "$@" > $OUT/$n.json 2> $OUT/$n.err || return $?; }
  tools/gsafe.sh \
    "$(declare -f run); run rats_driver --gpus 1 --steps 20 --warmup 5" \
    "$(declare -f run); run rats_default" \
    "$(declare -f run); run rats_reference --scheme reference" \
    "$(declare -f run); run rats_gibbs_ir --workload rats_gibbs_ir" \
    "$(declare -f run); run rats_ir --workload rats_ir" \
    "$(declare -f run); run seeds_ir --workload seeds_ir" \
    "$(declare -f run); run line_amm --workload line_amm" \
    "$(declare -f run); run logistic --workload logistic" \
    "$(declare -f run); run logistic_forward --workload logistic --gradient forward --no-cpu-baseline" \
    "timeout -k 10 400 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > $OUT/torchrun1.json 2> $OUT/torchrun1.err"
  for f in $OUT/*.json; do python3 -c "import json,sys; d=json.loads(open('$f').read().strip().splitlines()[-1]); print('$f', '%.4g' % d['value'], round(d['roofline'].get('frac', 0), 3))" || true; done ;;
esac
