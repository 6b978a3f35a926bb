#!/bin/bash
# full visit: gpu tests, smoke, bench with CPU baseline (the driver's end-of-round sequence)
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
mkdir -p $OUT
timeout -k 10 500 python -m pytest tests -m gpu -q -p no:cacheprovider > $OUT/pytest_gpu.log 2>&1; echo "pytest rc=$?"; tail -2 $OUT/pytest_gpu.log
timeout -k 10 200 python __graft_entry__.py smoke > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/smoke.log
timeout -k 10 500 python bench.py --full > $OUT/bench_full.log 2>&1; echo "bench rc=$?"; grep '^{' $OUT/bench_full.log | tail -1
