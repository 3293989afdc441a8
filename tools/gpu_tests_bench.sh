#!/bin/bash
# GPU test suite, then (only if the suite ended without a fault / timeout) the full bench (GPT + ResNet).
# Logs go to $OUT_DIR (default bench_logs/).
cd ${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT_DIR:-bench_logs}
mkdir -p $O
timeout -k 10 700 python -u -m pytest tests -m gpu -q -x --timeout 120 --timeout-method thread ${PYTEST_EXTRA:-} > $O/pytest_gpu.log 2>&1
rc=$?
tail -5 $O/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
timeout -k 10 300 python bench.py --full > $O/bench_default.log 2>&1
rc2=$?
tail -4 $O/bench_default.log
exit $rc2
