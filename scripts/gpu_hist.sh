#!/bin/bash
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
mkdir -p $OUT/prof_hist
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_hist -o bench -- python3 $R/bench.py --full --steps 5 --warmup 1 --no-cpu --offsets hist > $OUT/bench_hist.log 2>&1
echo "rc=$?"; grep '^{' $OUT/bench_hist.log | tail -1 | cut -c1-600
