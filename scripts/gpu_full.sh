# full GPU suite, smoke, bench --full (with CPU baseline); logs under $LOGS (default logs/)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
LOGS=${LOGS:-logs}
cd $R && mkdir -p $LOGS
timeout -k 10 1000 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread -p no:cacheprovider > $LOGS/full_tests.log 2>&1 || { echo TESTS FAILED; grep -E "FAILED|^E  " $LOGS/full_tests.log | head -20; tail -5 $LOGS/full_tests.log; exit 1; }
tail -1 $LOGS/full_tests.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $LOGS/full_smoke.log 2>&1 || { echo SMOKE FAILED; tail -5 $LOGS/full_smoke.log; exit 1; }
tail -1 $LOGS/full_smoke.log
timeout -k 10 600 python bench.py --full > $LOGS/full_bench.log 2>&1 || { echo BENCH FAILED; tail -5 $LOGS/full_bench.log; exit 1; }
tail -1 $LOGS/full_bench.log | cut -c1-400
