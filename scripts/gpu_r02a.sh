#!/bin/bash
# GPU suite, bench (default args), then the rocprofv3 evidence at 10^7 and 10^8.
set -o pipefail
mkdir -p run_out
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > run_out/pytest_gpu.log 2>&1
rc=$?; tail -3 run_out/pytest_gpu.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error" run_out/pytest_gpu.log | head -20; exit $rc; }
timeout -k 10 600 python bench.py --full > run_out/bench.json 2> run_out/bench.err
rc=$?; cat run_out/bench.json; [ $rc -eq 0 ] || { tail -5 run_out/bench.err; exit $rc; }
bash scripts/profile_f64.sh ${TAG:-r02a} > run_out/profile.log 2>&1; rc=$?; tail -5 run_out/profile.log; [ $rc -eq 0 ] || exit $rc
RECORDS=100000000 bash scripts/profile_f64.sh ${TAG:-r02a}_1e8 > run_out/profile_1e8.log 2>&1; rc=$?; tail -5 run_out/profile_1e8.log; exit $rc
