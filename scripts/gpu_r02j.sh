#!/bin/bash
# round evidence: GPU suite, bench (default args), rocprofv3 trace + PMC of the config-3 decode
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
mkdir -p run_out
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > run_out/pytest_gpu.log 2>&1
rc=$?; tail -3 run_out/pytest_gpu.log; [ $rc -eq 0 ] || { grep -E "FAILED|Error" run_out/pytest_gpu.log | head -20; exit $rc; }
timeout -k 10 600 python bench.py --full > run_out/bench.json 2> run_out/bench.err
rc=$?; cat run_out/bench.json; [ $rc -eq 0 ] || { tail -5 run_out/bench.err; exit $rc; }
bash scripts/profile_mixed.sh ${TAG:-r02j} > run_out/prof_mixed.log 2>&1; rc=$?; tail -3 run_out/prof_mixed.log; exit $rc
