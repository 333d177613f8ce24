# Fused ModDown COL pass (k_moddown_col): parity tests, then A/B x2 on one box
# against SFHE_MODDOWN_COL=0 (k_mdrsf / k_convf + the plain COL pass).
#   bash tools/gpu_md_ab.sh <tag>
set -o pipefail
T=${1:-r05md}
mkdir -p gpurun_out/$T
export PYTHONUNBUFFERED=1
timeout -k 10 600 python -u -m pytest -x -v --timeout 300 --timeout-method thread -m gpu \
    tests/test_gpu_parity.py tests/test_gpu_parity_metric.py tests/test_gpu_parity_sort.py tests/test_gpu_graph.py \
    tests/test_gpu_stack.py tests/test_gpu_sort.py > gpurun_out/$T/gpu_tests.log 2>&1 || exit $?
B="--full --no-kway --no-hybrid1 --no-c5 --no-cpu-baseline --trials 1 --steps 20 --warmup 3"
for k in 1 2; do
  timeout -k 10 300 python -u bench.py $B > gpurun_out/$T/fused_$k.json 2>/dev/null || exit 1
  SFHE_MODDOWN_COL=0 timeout -k 10 300 python -u bench.py $B > gpurun_out/$T/unfused_$k.json 2>/dev/null || exit 1
done
