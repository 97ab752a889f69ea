#!/bin/bash
# One GPU-box session of round 5.  Stages (each isolated: own process + timeout), chosen by $1:
#   new      the tests written / changed this round (fp32 decode mode, exchange hardening)
#   all      the full GPU suite;  allk: the same with PYTEST_K as -k expression and without -x
#   beam     the BASELINE-size decode parity tests (new fixture: bf16 criterion + fp32 token-exact)
#   smoke    __graft_entry__.smoke()
#   bench    the default bench line;  benchq: training leg only
#   profstep rocprofv3 kernel table of the CAPTURED step only (bench.py --timed-only: warm-up + timed replays, nothing else)
#   prof     kernel table of the whole default training leg (as rounds 1-4)
#   mfma / traffic / trafficd   PMC passes (scripts/pmc_*.sh)
#   ab       same-box A/B of environment switches: AB="NAME=a NAME=b ..."
#   gemmbig  scripts/gemm_big_bench.py (tile variants of the large GEMMs)
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-out}      # where the stages write their logs, relative to the repository root
mkdir -p "$OUT"
export PYTHONPATH=$PWD TMPDIR=/tmp
STAGES=${1:-"new all smoke benchq"}
for st in $STAGES; do
  echo "=== stage $st $(date +%T)"
  case $st in
    new)    timeout 900 python -m pytest tests/test_gpu_decode_f32.py tests/test_gpu_sync_ln.py -m gpu -q -p no:cacheprovider > $OUT/new_gpu.log 2>&1; echo "rc=$?"; grep -E "^FAILED|^ERROR|Error|assert" $OUT/new_gpu.log | head -40; tail -4 $OUT/new_gpu.log ;;
    all)    timeout 1500 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/all_gpu.log 2>&1; echo "rc=$?"; tail -6 $OUT/all_gpu.log ;;
    allk)   timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider ${PYTEST_K:+-k "$PYTEST_K"} > $OUT/all_gpu.log 2>&1; echo "rc=$?"; grep -E "^FAILED|^ERROR" $OUT/all_gpu.log | head -40; tail -5 $OUT/all_gpu.log ;;
    beam)   timeout 1200 python -m pytest tests/test_gpu_fullsize.py -m gpu -q -p no:cacheprovider -k "beam or fixture" > $OUT/beam.log 2>&1; echo "rc=$?"; grep -E "^FAILED|^ERROR" $OUT/beam.log | head; tail -4 $OUT/beam.log ;;
    smoke)  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "rc=$?"; tail -3 $OUT/smoke.log ;;
    bench)  timeout 900 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "rc=$?"; tail -c 1500 $OUT/bench.json; tail -3 $OUT/bench.err ;;
    benchq) timeout 600 python bench.py --full --no-cpu-baseline --no-decode > $OUT/benchq.json 2> $OUT/benchq.err; echo "rc=$?"; grep -o '"ms_per_step": [0-9.]*\|"static_batch_ms_per_step": [0-9.]*\|"feed_overhead_frac": [-0-9.e]*' $OUT/benchq.json; tail -3 $OUT/benchq.err ;;
    ab)     for kv in ${AB:-}; do fn=$(echo "$kv" | tr '/=:' '___'); echo "--- $kv"; env $kv timeout 600 python bench.py --no-cpu-baseline --no-decode --steps 40 --timed-only ${AB_ARGS:-} > $OUT/ab_$fn.json 2> $OUT/ab_$fn.err; grep -o '"ms_per_step": [0-9.]*' $OUT/ab_$fn.json; tail -1 $OUT/ab_$fn.err | cut -c1-200; done ;;
    profstep) (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OLDPWD/$OUT/profs -o r1 -- python $OLDPWD/bench.py --steps 40 --warmup 2 --timed-only > $OLDPWD/$OUT/profstep.log 2>&1); echo "rc=$?"
            python scripts/prof_summary.py $(find $OUT/profs -name "*.db" | head -1) 42 > $OUT/rocprof_captured_step.txt 2>&1
            python scripts/prof_gaps.py $(find $OUT/profs -name "*.db" | head -1) > $OUT/rocprof_captured_step_gaps.txt 2>&1
            rm -rf $OUT/profs; head -${PROF_HEAD:-50} $OUT/rocprof_captured_step.txt; tail -2 $OUT/profstep.log; head -${GAP_HEAD:-30} $OUT/rocprof_captured_step_gaps.txt ;;
    prof)   (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OLDPWD/$OUT/prof -o r1 -- python $OLDPWD/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-decode > $OLDPWD/$OUT/prof.log 2>&1); echo "rc=$?"
            python scripts/prof_summary.py $(find $OUT/prof -name "*.db" | head -1) > $OUT/rocprof_kernel_stats.txt 2>&1
            rm -rf $OUT/prof; head -${PROF_HEAD:-45} $OUT/rocprof_kernel_stats.txt ;;
    profd)  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OLDPWD/$OUT/profd -o r1 -- python $OLDPWD/bench.py --mode decode --sentences 600 --no-cpu-baseline > $OLDPWD/$OUT/profd.log 2>&1); echo "rc=$?"
            python scripts/prof_summary.py $(find $OUT/profd -name "*.db" | head -1) 1 > $OUT/rocprof_decode.txt 2>&1; rm -rf $OUT/profd; head -40 $OUT/rocprof_decode.txt ;;
    mfma)   bash scripts/pmc_mfma.sh ;;
    traffic) bash scripts/pmc_traffic.sh ;;
    trafficd) bash scripts/pmc_traffic_decode.sh ;;
    gemmsched) timeout 600 python scripts/gemm_big_bench.py --sched > $OUT/gemm_sched.txt 2>&1; echo "rc=$?"; tail -12 $OUT/gemm_sched.txt ;;
    gemmbig) timeout 600 python scripts/gemm_big_bench.py > $OUT/gemm_big.txt 2>&1; echo "rc=$?"; tail -40 $OUT/gemm_big.txt ;;
    twin)   bash scripts/launch_blocking_twin.sh ;;
    soak)   timeout 600 python scripts/soak_decode.py 200 4 > $OUT/soak_decode.json 2> $OUT/soak_decode.err; echo "rc=$?"; cat $OUT/soak_decode.json; tail -3 $OUT/soak_decode.err ;;
    decode) timeout 600 python bench.py --mode decode > $OUT/bench_decode.json 2> $OUT/bench_decode.err; echo "rc=$?"; tail -c 900 $OUT/bench_decode.json ;;
  esac
done
echo "=== done $(date +%T)"
