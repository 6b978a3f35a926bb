#!/bin/bash
# rocprofv3 kernel trace of the bench's minibatch leg; prints the launch timeline of a few minibatch steps
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
cd /tmp && export TMPDIR=/tmp
rm -rf $OUT/mbtrace
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d $OUT/mbtrace -o mb -- python3 $R/bench.py --full --no-cpu --trained-steps 0 --steps 5 --blocks 1 > $OUT/mbtrace.log 2>&1
f=$(find $OUT/mbtrace -name "*kernel_trace.csv" | head -1)
python3 $R/scripts/mb_timeline.py $f
rm -rf $OUT/mbtrace
