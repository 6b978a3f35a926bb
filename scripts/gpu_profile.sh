#!/bin/bash
# rocprofv3 kernel trace of the bench (no PMC in this pass).
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
mkdir -p $OUT/prof
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o bench -- python3 $R/bench.py --full --steps 10 --warmup 2 --no-cpu "$@" > $OUT/prof_bench.log 2>&1
echo "rocprof rc=$?"
tail -2 $OUT/prof_bench.log
find $OUT/prof -name "*stats*" | head
