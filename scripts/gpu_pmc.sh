#!/bin/bash
# PMC passes over the bench (each --pmc set in its own run, with --kernel-trace only).
set -u
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${OUT:-$R/out}
mkdir -p $OUT/pmc
cd /tmp && export TMPDIR=/tmp
if [ "${1:-}" = "list" ]; then rocprofv3 -L > $OUT/pmc/counters.txt 2>&1; grep -c "" $OUT/pmc/counters.txt; exit 0; fi
i=0
for set in "$@"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $set --output-format csv -d $OUT/pmc -o pass$i -- python3 $R/bench.py --full --steps 4 --warmup 1 --no-cpu > $OUT/pmc/pass$i.log 2>&1
  echo "pass$i ($set) rc=$?"
done
ls $OUT/pmc
