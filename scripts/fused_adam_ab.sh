#!/bin/bash
# The fused-optimizer-step measurement: the A/B run, one kernel trace per variant (no counters), the merge.
# usage: scripts/fused_adam_ab.sh <out.json> [workload]      (from the repository root)
# Every GPU step has its own time limit and the chain stops at the first failure.
R=$(pwd)
OUT=${1:-profiles/r07/fused_adam_D.json}
WL=${2:-D}
TR=$(mktemp -d)
export TMPDIR=/tmp
timeout -k 10 420 python $R/scripts/fused_adam_ab.py --workload $WL --out $R/$OUT > $TR/ab.log 2>&1 &&
(cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $TR -o a -- python $R/scripts/fused_adam_ab.py --workload $WL --variant A --iters 60 > $TR/a.log 2>&1) &&
(cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats -d $TR -o b -- python $R/scripts/fused_adam_ab.py --workload $WL --variant B --iters 60 > $TR/b.log 2>&1) &&
python $R/scripts/rocpd_stats.py $TR/a_results.db $TR/a.csv > $TR/a.txt &&
python $R/scripts/rocpd_stats.py $TR/b_results.db $TR/b.csv > $TR/b.txt &&
python $R/scripts/fused_adam_ab.py --workload $WL --merge-trace $TR/a.csv $TR/b.csv --out $R/$OUT
rc=$?
tail -n 5 $TR/ab.log $TR/a.log $TR/b.log 2>/dev/null
head -n 12 $TR/b.txt 2>/dev/null
rm -f $TR/*.db
exit $rc
