#!/bin/bash
# One GPU session: parity tests, smoke, bench, kernel-trace profile.  Stops at the first failure.
# Logs go to $OUT (default build/check, which git ignores).
set -o pipefail
OUT=${OUT:-build/check}
mkdir -p $OUT
STEPS=${STEPS:-30}
echo "== pytest -m gpu"
timeout -k 10 480 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1
rc=$?; tail -5 $OUT/pytest_gpu.log; [ $rc -eq 0 ] || { tail -60 $OUT/pytest_gpu.log; exit $rc; }
echo "== smoke"
timeout -k 10 180 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; tail -3 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
echo "== bench"
timeout -k 10 400 python bench.py --full --steps $STEPS > $OUT/bench.log 2>&1
rc=$?; tail -3 $OUT/bench.log; [ $rc -eq 0 ] || exit $rc
if [ -n "$PROFILE" ]; then
  echo "== rocprofv3 kernel trace"
  cd /tmp && export TMPDIR=/tmp && cd - >/dev/null
  timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 bench.py --full --steps $STEPS --no-cpu-baseline > $OUT/prof.log 2>&1
  rc=$?; tail -3 $OUT/prof.log; [ $rc -eq 0 ] || exit $rc
fi
echo "== done"
