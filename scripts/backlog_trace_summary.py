"""Where the bench's timed backlog spends its time outside the kernels
(profiles/seq_backlog/before.json, after.json). Reads a directory DIR holding
  DIR/plain.json  the line of `python3 bench.py --gpus 1 --steps 20 --warmup 5`
  DIR/trace/      rocprofv3 --kernel-trace --hip-trace --output-format csv -d DIR/trace -o t -- <that command>
  DIR/pmc/        rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY ...
                  --output-format csv -d DIR/pmc -o run -- python3 scripts/prof_f64.py 10000000 6 seq
                  (counters in a run of their own)
and prints: the timed backlog's kernel mean, first launch call -> first kernel start, and every
host call and other kernel after the last launch, relative to the end of the last
sequential-id decode kernel (nxg_f64s_kernel, one per frame, or nxg_f64s_backlog_kernel, one per
group of frames: profiles/seq_group/); the counters' means per launch.
usage: python3 scripts/backlog_trace_summary.py DIR > DIR/summary.json"""
import collections
import csv
import glob
import json
import sys

out = sys.argv[1]
res = {"plain": json.loads(open(f"{out}/plain.json").read().strip().splitlines()[-1])}
res["plain"] = {k: res["plain"][k] for k in ("value", "ms_per_step", "steps", "warmup")}


def one(pat):
    f = glob.glob(f"{out}/{pat}", recursive=True)
    return f[0] if f else None


kt, ht = one("trace/**/*kernel_trace.csv"), one("trace/**/*hip_api_trace.csv")
if kt and ht:
    ks = sorted(({"name": r["Kernel_Name"], "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"])}
                 for r in csv.DictReader(open(kt))), key=lambda r: r["s"])
    api = sorted(({"f": r["Function"], "s": int(r["Start_Timestamp"]), "e": int(r["End_Timestamp"]),
                   "tid": r["Thread_Id"]} for r in csv.DictReader(open(ht))), key=lambda r: r["s"])
    main_tid = collections.Counter(a["tid"] for a in api if "LaunchKernel" in a["f"]).most_common(1)[0][0]
    api = [a for a in api if a["tid"] == main_tid]
    # segments of launches between stream synchronizes: the timed backlog is the one whose
    # sequential-id kernels (per-frame or backlog) run longest
    f64 = [k for k in ks if "nxg_f64s_" in k["name"]]
    res["kernel"] = {"name": f64[0]["name"].split("(")[0] if f64 else None, "launches": len(f64),
                     "mean_us_all": round(sum(k["e"] - k["s"] for k in f64) / max(1, len(f64)) / 1e3, 3)}
    syncs = [a for a in api if a["f"] == "hipStreamSynchronize" or a["f"] == "hipDeviceSynchronize"]
    bounds = [0] + [a["e"] for a in syncs] + [1 << 62]
    best = None
    for lo, hi in zip(bounds, bounds[1:]):
        la = [a for a in api if "LaunchKernel" in a["f"] and lo <= a["s"] < hi]
        if not la:
            continue
        sk = [k for k in f64 if la[0]["s"] <= k["s"] < hi]
        busy = sum(k["e"] - k["s"] for k in sk)
        if sk and (best is None or busy > best[0]):
            best = (busy, la, sk)
    _, la, seg_k = best
    t_first_call = la[0]["s"]
    first_k, last_k = seg_k[0], seg_k[-1]
    burst = [k for k in ks if first_k["s"] <= k["s"] and k["s"] <= last_k["e"] + 2_000_000]
    last_any = max(k["e"] for k in burst if k["s"] <= last_k["e"] + 200_000)
    tail_api = [a for a in api if a["s"] >= la[-1]["e"]][:14]
    res["backlog"] = {
        "launch_calls_in_segment": len(la),
        "f64s_kernels": len(seg_k),
        "f64s_kernel_names": sorted({k["name"].split("(")[0] for k in seg_k}),
        "kernel_mean_us": round(sum(k["e"] - k["s"] for k in seg_k) / len(seg_k) / 1e3, 3),
        "first_launch_call_to_first_kernel_start_us": round((first_k["s"] - t_first_call) / 1e3, 2),
        "first_launch_call_to_last_launch_return_us": round((la[-1]["e"] - t_first_call) / 1e3, 2),
        "burst_first_start_to_last_f64s_end_us": round((last_k["e"] - first_k["s"]) / 1e3, 2),
        "other_kernels_after_last_f64s": [
            {"name": k["name"].split("(")[0], "start_after_us": round((k["s"] - last_k["e"]) / 1e3, 2),
             "dur_us": round((k["e"] - k["s"]) / 1e3, 2)} for k in burst if k["s"] > last_k["s"] and k is not last_k],
        "host_calls_after_last_launch": [
            {"f": a["f"], "start_rel_last_f64s_end_us": round((a["s"] - last_k["e"]) / 1e3, 2),
             "end_rel_last_f64s_end_us": round((a["e"] - last_k["e"]) / 1e3, 2),
             "dur_us": round((a["e"] - a["s"]) / 1e3, 2)} for a in tail_api],
    }

pc = one("pmc/**/*counter_collection.csv")
if pc:
    acc = collections.defaultdict(lambda: collections.defaultdict(float))
    disp = collections.defaultdict(set)
    for r in csv.DictReader(open(pc)):
        k = r["Kernel_Name"].split("(")[0]
        if "nxg_f64s" not in k:
            continue
        acc[k][r["Counter_Name"]] += float(r["Counter_Value"])
        disp[k].add(r["Dispatch_Id"])
    res["counters_per_launch"] = {k: dict({"dispatches": len(disp[k])},
                                          **{c: v / len(disp[k]) for c, v in sorted(cs.items())})
                                  for k, cs in acc.items()}
print(json.dumps(res, indent=1))
