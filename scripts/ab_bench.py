"""A/B of library builds (NXG_LIB) on the bench's plain command: ROUNDS rounds, in each one run of
every build in the order given, one process per run; per build the median and min-max of `value`
(profiles/seq_backlog/ab.json was made with it). Stops at the first run that fails.
usage: python3 scripts/ab_bench.py OUT.json ROUNDS STEPS name=lib [name=lib ...]   (lib: path from
the repository root)"""
import json
import os
import statistics
import subprocess
import sys

R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
out, rounds, steps = sys.argv[1], int(sys.argv[2]), sys.argv[3]
builds = [a.split("=", 1) for a in sys.argv[4:]]
runs = {n: [] for n, _ in builds}
for i in range(rounds):
    for name, lib in builds:
        env = dict(os.environ, NXG_LIB=os.path.join(R, lib))
        p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(R, "bench.py"),
                            "--gpus", "1", "--steps", steps, "--warmup", "5"],
                           env=env, capture_output=True, text=True)
        if p.returncode != 0:
            print("run failed", name, p.returncode, p.stderr[-2000:])
            sys.exit(1)
        j = json.loads(p.stdout.strip().splitlines()[-1])
        runs[name].append({"value": j["value"], "ms_per_step": j["ms_per_step"]})
        print(i, name, j["value"], j["ms_per_step"], flush=True)
res = {"command": f"bench.py --gpus 1 --steps {steps} --warmup 5", "rounds": rounds,
       "order": [n for n, _ in builds], "builds": {}}
for n, rs in runs.items():
    v = [r["value"] for r in rs]
    res["builds"][n] = {"median": statistics.median(v), "min": min(v), "max": max(v),
                        "range": round(max(v) - min(v), 2), "runs": rs}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps({n: {k: b[k] for k in ("median", "min", "max", "range")}
                  for n, b in res["builds"].items()}))
