#!/bin/bash
# One GPU-box session of round 3: full GPU suite, smoke, the default bench line (training + decode + cpu_baseline),
# kernel table, MFMA counters, the 256-sentence side measurement.  Each stage isolated (own process + timeout).
set -u
cd "$(dirname "$0")/.."
OUT=${OUT:-out}      # where the stages write their logs, relative to the repository root
mkdir -p "$OUT"
export PYTHONPATH=$PWD TMPDIR=/tmp
STAGES=${1:-"all smoke bench prof mfma side"}
for st in $STAGES; do
  echo "=== stage $st $(date +%T)"
  case $st in
    all)    timeout 1500 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $OUT/all_gpu.log 2>&1; echo "rc=$?"; tail -6 $OUT/all_gpu.log ;;
    allk)   timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider > $OUT/all_gpu.log 2>&1; echo "rc=$?"; tail -15 $OUT/all_gpu.log ;;
    dp)     timeout 900 python -m pytest tests/test_gpu_dp.py tests/test_gpu_fullsize.py -m gpu -q -p no:cacheprovider > $OUT/dp.log 2>&1; echo "rc=$?"; tail -15 $OUT/dp.log ;;
    smoke)  timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; echo "rc=$?"; tail -3 $OUT/smoke.log ;;
    bench)  timeout 900 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "rc=$?"; tail -c 1500 $OUT/bench.json; tail -3 $OUT/bench.err ;;
    benchq) timeout 600 python bench.py --full --no-cpu-baseline --no-decode > $OUT/benchq.json 2> $OUT/benchq.err; echo "rc=$?"; grep -o '"ms_per_step": [0-9.]*' $OUT/benchq.json ;;
    prof)   (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OLDPWD/$OUT/prof -o r1 -- python $OLDPWD/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-decode > $OLDPWD/$OUT/prof.log 2>&1); echo "rc=$?"
            python scripts/prof_summary.py $(find $OUT/prof -name "*.db" | head -1) > $OUT/rocprof_kernel_stats.txt 2>&1; rm -rf $OUT/prof; head -45 $OUT/rocprof_kernel_stats.txt ;;
    profd)  (cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OLDPWD/$OUT/profd -o r1 -- python $OLDPWD/bench.py --mode decode --sentences 600 --no-cpu-baseline > $OLDPWD/$OUT/profd.log 2>&1); echo "rc=$?"
            python scripts/prof_summary.py $(find $OUT/profd -name "*.db" | head -1) 1 > $OUT/rocprof_decode.txt 2>&1; rm -rf $OUT/profd; head -40 $OUT/rocprof_decode.txt ;;
    mfma)   bash scripts/pmc_mfma.sh ;;
    traffic) bash scripts/pmc_traffic.sh ;;
    side)   timeout 600 python bench.py --sentences-per-gpu 256 --no-cpu-baseline --no-decode > $OUT/bench_b256.json 2> $OUT/bench_b256.err; echo "rc=$?"; grep -o '"ms_per_step": [0-9.]*\|"step_mfma_frac": [0-9.]*' $OUT/bench_b256.json ;;
    decode) timeout 600 python bench.py --mode decode > $OUT/bench_decode.json 2> $OUT/bench_decode.err; echo "rc=$?"; tail -c 900 $OUT/bench_decode.json ;;
  esac
done
echo "=== done $(date +%T)"
