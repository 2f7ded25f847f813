set -o pipefail
mkdir -p run_out
timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > run_out/pytest_gpu.log 2>&1
rc=$?; tail -3 run_out/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full > run_out/bench.json 2> run_out/bench.err
rc=$?; cat run_out/bench.json; [ $rc -eq 0 ] || { tail -5 run_out/bench.err; exit $rc; }
bash scripts/profile_f64.sh ${TAG:-r01f} > run_out/profile.log 2>&1; rc=$?; tail -3 run_out/profile.log; exit $rc
