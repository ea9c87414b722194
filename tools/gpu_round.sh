#!/bin/bash
# One GPU-box session: parity tests, smoke, bench (--full), kernel-trace profile.  Later steps only run when
# the earlier ones ended normally (exit 0/1), never after a timeout or kill.
#   bash tools/gpu_round.sh TAG OUT
set -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-run}
OUT=$(mkdir -p "${2:?usage: tools/gpu_round.sh TAG OUT_DIR}" && cd "$2" && pwd)
timeout -k 10 900 python -m pytest tests -m gpu -q --maxfail=20 --timeout 400 -p no:cacheprovider > $OUT/pytest_gpu_$TAG.log 2>&1
rc=$?; echo "pytest exit $rc" | tee -a $OUT/pytest_gpu_$TAG.log
tail -5 $OUT/pytest_gpu_$TAG.log
if [ $rc -gt 1 ]; then exit $rc; fi
timeout -k 10 300 python __graft_entry__.py smoke > $OUT/smoke_$TAG.log 2>&1; rc=$?; tail -2 $OUT/smoke_$TAG.log
if [ $rc -gt 1 ]; then exit $rc; fi
timeout -k 10 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err; rc=$?
cat $OUT/bench_$TAG.json; tail -3 $OUT/bench_$TAG.err
if [ $rc -ne 0 ]; then exit $rc; fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $ROOT/bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-extra-points > $OUT/prof_$TAG.log 2>&1
echo "rocprof exit $?"
find $OUT/prof_$TAG -name "*kernel_stats.csv" | head -2 | xargs -r head -12
