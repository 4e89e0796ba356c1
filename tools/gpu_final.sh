#!/bin/bash
# Round-end evidence in one GPU session: every gpu test, the bench lines (C3 default with the
# CPU baseline, C2/C4/C5), PMC FETCH/WRITE passes over the decode stage and kernel-trace stats.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
tag=${1:-r02c}
O=$R/gpurun_out/$tag
mkdir -p $O
cd $R
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $O/gpu_tests.log 2>&1 || { echo "gpu tests failed"; tail -30 $O/gpu_tests.log; exit 1; }
tail -1 $O/gpu_tests.log
timeout -k 10 300 python bench.py --full > $O/bench_c3.json 2> $O/bench_c3.err || { echo "bench c3 failed"; tail -20 $O/bench_c3.err; exit 1; }
for w in c2 c4 c5; do
  timeout -k 10 200 python bench.py --full --workload $w --cpu-baseline 0 > $O/bench_$w.json 2> $O/bench_$w.err || { echo "bench $w failed"; tail -20 $O/bench_$w.err; exit 1; }
done
export PMC_KERNEL="decode|spectra|apply_split"
for w in c3 c4; do
  "$R/tools/pmc_run.sh" "${tag}_${w}_fetch" "FETCH_SIZE" --workload $w || exit 1
  "$R/tools/pmc_run.sh" "${tag}_${w}_write" "WRITE_SIZE" --workload $w || exit 1
done
cd /tmp && export TMPDIR=/tmp
for w in c3 c4; do
  timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/gpurun_out/stats_${tag}_$w" -o run -- python3 "$R/bench.py" --workload $w --cpu-baseline 0 --sc16-steps 0 --steps 10 > "$R/gpurun_out/stats_${tag}_$w.log" 2>&1 || exit 1
done
echo done
