# Round-end check on one box: full GPU suite, smoke, the default bench line,
# then the rocprof kernel trace + PMC passes (tools/profile_round.sh <tag>).
set -e
tag=${1:-rXX}
O=${SFHE_OUT:-bench_out}
mkdir -p $O
timeout -k 10 420 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/${tag}_gpu_suite.log 2>&1
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/${tag}_smoke.log 2>&1
timeout -k 10 360 python bench.py --full > $O/${tag}_bench.log 2>&1
tail -1 $O/${tag}_bench.log > $O/${tag}_bench.json
bash tools/profile_round.sh ${tag}
