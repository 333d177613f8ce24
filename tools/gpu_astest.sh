#!/bin/bash
# Developer GPU script: the debug-sort graph test and the default bench line
# (trials: pure / as-test / cold).
set -o pipefail
cd "$(dirname "$0")/.."
T=${TAG:-astest}
O=${SFHE_OUT:-bench_out}
mkdir -p $O
timeout -k 10 300 python -u -m pytest -x -v --timeout 200 --timeout-method thread tests/test_gpu_graph.py tests/test_gpu_sort.py -m gpu > $O/${T}_tests.log 2>&1 || exit $?
timeout -k 10 600 python -u bench.py --full > $O/${T}_bench.json 2> $O/${T}_bench.err || exit $?
exit 0
