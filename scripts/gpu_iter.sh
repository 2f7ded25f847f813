#!/bin/bash
# Iteration run: GPU parity tests, general-path diagnostics, bench. Chained with && (stop at
# the first failure); every step bounded by its own timeout.
set -o pipefail
mkdir -p run_out
timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > run_out/pytest_gpu.log 2>&1
rc=$?; tail -15 run_out/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python scripts/diag_general.py ${DIAG_N:-100000 1000000 10000000} > run_out/diag.log 2>&1
rc=$?; cat run_out/diag.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 20 --warmup 5} > run_out/bench.json 2> run_out/bench.err
rc=$?; cat run_out/bench.json; tail -3 run_out/bench.err; exit $rc
