#!/bin/bash
# Alternating A/B of bench.py --full (GPT + ResNet figures) under two values of one environment
# variable; stops at the first failing run. Logs go to $OUT_DIR (default bench_logs/).
# usage: tools/ab_env.sh VAR "A B" REPS OUTFILE [extra bench args]
var=$1; vals=$2; reps=$3; out=$4; shift 4
cd ${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT_DIR:-bench_logs}
mkdir -p $O
: > $O/$out
for r in $(seq 1 $reps); do
  for v in $vals; do
    env $var=$v timeout -k 10 240 python bench.py --full --steps 10 --warmup 3 "$@" > $O/ab_tmp.log 2>&1
    rc=$?
    if [ $rc -ne 0 ]; then echo "$var=$v rc=$rc" >> $O/$out; tail -20 $O/ab_tmp.log >> $O/$out; exit $rc; fi
    echo "$var=$v $(tail -1 $O/ab_tmp.log | python3 -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["ms_per_step"], d["config"].get("resnet50_samples_per_sec"))')" >> $O/$out
  done
done
cat $O/$out
