#!/bin/bash
# quick GPU visit: parity tests, then the bench under rocprofv3 --kernel-trace (no CPU baseline leg)
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
mkdir -p $OUT/prof
timeout -k 10 400 python -m pytest tests -m gpu -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; tail -4 $OUT/pytest_gpu.log
if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then exit 99; fi
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu "$@" > $OUT/prof_bench.log 2>&1
echo "rocprof rc=$?"
grep '^{' $OUT/prof_bench.log | tail -1
