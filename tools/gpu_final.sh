#!/bin/bash
# End-of-session evidence: smoke, the whole GPU suite, the full bench (GPT + ResNet), and a rocprofv3
# kernel profile of a short full bench (stats only). Logs go to $OUT_DIR (default bench_logs/).
cd ${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT_DIR:-bench_logs}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail -5 $O/smoke.log; exit 1; }
tail -1 $O/smoke.log
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 120 --timeout-method thread -rf > $O/pytest_gpu_final.log 2>&1
rc=$?; tail -6 $O/pytest_gpu_final.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full > $O/bench_final.log 2>&1 || { tail -5 $O/bench_final.log; exit 1; }
tail -1 $O/bench_final.log
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $O/prof_final -o run -- python bench.py --full --steps 5 --warmup 2 > $O/prof_final.log 2>&1 || { tail -5 $O/prof_final.log; exit 1; }
tail -1 $O/prof_final.log
