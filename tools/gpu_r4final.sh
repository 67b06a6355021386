#!/bin/bash
# Round-4 evidence, in phases that each fit one gpurun call (PHASE = tests | bench | prof | pmc):
#   tests: the full -m gpu suite + smoke();  bench: one bench line per workload (BENCH list);
#   prof:  rocprofv3 kernel-trace summaries (PROF list);  pmc: FETCH_SIZE / WRITE_SIZE passes (PMC list).
# Everything lands under gpurun_out/r4f_* ; every GPU step has its own time limit and the script stops at the first
# failing step.
set -o pipefail
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
cd $ROOT
mkdir -p gpurun_out
case ${PHASE:-tests} in
  tests)
    timeout -k 10 720 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread -p no:cacheprovider \
      > gpurun_out/r4f_pytest_gpu.log 2>&1
    rc=$?; tail -5 gpurun_out/r4f_pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
    timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > gpurun_out/r4f_smoke.log 2>&1
    rc=$?; echo "smoke rc=$rc"; tail -3 gpurun_out/r4f_smoke.log; exit $rc ;;
  bench)
    for w in ${BENCH:-config3 config2 config3-agg config3-lds config1}; do
      timeout -k 10 ${BTIME:-400} python -u bench.py --full --workload $w --steps ${STEPS:-10} --warmup 3 --cpu-seconds ${CPU_SECS:-10} \
        > gpurun_out/r4f_bench_$w.json 2> gpurun_out/r4f_bench_$w.err
      rc=$?; echo "bench $w rc=$rc"; cat gpurun_out/r4f_bench_$w.json
      [ $rc -eq 0 ] || { tail -20 gpurun_out/r4f_bench_$w.err; exit $rc; }
    done ;;
  prof)
    for w in ${PROF:-config3 config2}; do bash tools/gpu_prof.sh $w _r4f || exit $?; done ;;
  pmc)
    for w in ${PMC:-config3}; do bash tools/gpu_pmc.sh $w || exit $?; cat gpurun_out/pmc_$w.json; done ;;
esac
