cd "$(dirname "$0")/.."; OUT=${SESSION_OUT:-session_out}; mkdir -p "$OUT"; export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests/test_gpu_rk4.py -x -v --timeout 120 --timeout-method thread > "$OUT/rk4_tests.log" 2>&1; rc=$?; tail -12 "$OUT/rk4_tests.log"; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python bench.py --full --workload c2 --integrator rk4 --secondary 0 > "$OUT/bench_c2_rk4.log" 2>&1 || exit $?
tail -1 "$OUT/bench_c2_rk4.log"
timeout -k 10 300 python bench.py --full --workload c2 --secondary 0 > "$OUT/bench_c2_ref.log" 2>&1 || exit $?
tail -1 "$OUT/bench_c2_ref.log"
