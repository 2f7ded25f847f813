#!/usr/bin/env python3
"""Decode / encode of subscriber write batches (publisher::To) against the Update path.

Legs, each in a child process of its own, at N messages of the config-3 value mix
(netidx_amd/synth.py), ids a seeded permutation, three frames in rotation (at N = 10^7 their
bytes and columns exceed the 256 MiB last-level cache):

  A  general decode (NXG_MIXED_PATH=general) of the Update frame      nxg_decode_updates
  B  decode of the Write frame for the same (id, value) list, wid = row index
                                                                       nxg_decode_writes
  C  encode of A's columns                                             nxg_encode_updates
  D  encode of B's columns                                             nxg_encode_writes

Every call is synchronous; each is timed with a pair of HIP events on the codec's stream, after
warm-up calls. The checks (the decoded columns against the generator's, the To frame's bytes
against the Python twin for a prefix, the round trips) run outside the timed calls. A library
without the To calls runs A and C only.

  python scripts/bench_writes.py --n 1000000 --out run.json          all legs, one child each
  python scripts/bench_writes.py --leg B --n 1000000                 one leg, in this process
  python scripts/bench_writes.py --judge parent1.json parent2.json new.json
NXG_LIB=<another build of the library> measures that build (legs A and C: --legs AC).

Each child runs under `timeout -k 10`; the first failing leg ends the run.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0x5EED0003, 0x5EED0013, 0x5EED0023)


def has_to_calls():
    sys.path.insert(0, ROOT)  # (the binding only: this process does not open the GPU)
    from netidx_amd import codec as cm
    return hasattr(cm.Codec, "decode_writes")


def run_leg(leg, n, steps, warmup):
    os.environ["NXG_MIXED_PATH"] = "general"
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import Columns

    to = leg in "BD"
    codec = netidx_amd.Codec(0)
    stream = torch.cuda.Stream()
    codec.set_stream(stream.cuda_stream)
    sets = []
    for seed in SEEDS:
        m = synth.mixed_columns(n, seed)
        cols = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed,
                                              m.caux)
        heap = torch.from_numpy(m.heap.copy()).cuda()
        if to:
            wc = netidx_amd.WriteCols(n, "cuda")
            wc.wid[:n] = torch.arange(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            wire = codec.encode_writes(cols, wc, heap)
        else:
            wc = None
            wire = codec.encode_batch(cols, heap)
        sets.append((m, cols, wc, heap, wire))
    W = [int(s[4].numel()) for s in sets]
    nch = max(len(s[0].ctag) for s in sets)
    out = Columns(n, nch, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    wout = netidx_amd.WriteCols(n, "cuda") if to else None
    dout = torch.empty(max(W) + 64, dtype=torch.uint8, device="cuda")

    def call(i):
        m, cols, wc, heap, wire = sets[i % len(sets)]
        if leg == "A":
            codec.decode_into(wire, wire.numel(), out, netidx_amd.HINT_MIXED)
        elif leg == "B":
            codec.decode_writes(wire, out, wout)
        elif leg == "C":
            codec.encode_into(cols, heap, dout.data_ptr(), dout.numel())
        else:
            codec.encode_writes_into(cols, wc, heap, dout.data_ptr(), dout.numel())

    for i in range(warmup):
        call(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(steps):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call(i)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    # ---- checks, outside the timed calls: the last call used set (steps - 1) % 3 ----
    m, cols, wc, heap, wire = sets[(steps - 1) % len(sets)]
    if leg in "AB":
        g = out.numpy()
        assert len(g["id"]) == n
        assert np.array_equal(g["id"], m.id) and np.array_equal(g["tag"], m.tag)
        assert np.array_equal(g["aux"], m.aux)
        flat = np.isin(m.tag, (6, 9, 10))
        assert np.array_equal(g["fixed"][flat], m.fixed[flat])
        assert np.array_equal(g["ctag"], m.ctag) and np.array_equal(g["cfixed"], m.cfixed)
        path = codec.last_status()[2]
        assert path == (netidx_amd.PATH_WRITES if to else 2), path
        if to:
            w = wout.numpy(n)
            assert np.array_equal(w["wid"], np.arange(n, dtype=np.uint64))
            assert not w["wflags"].any()
    else:
        assert dout[: wire.numel()].equal(wire)
    if to:  # the To frame's first messages, byte for byte, against the Python twin
        import to_twin
        k = min(n, 2000)
        exp = b"".join(
            to_twin.write(int(m.id[i]), False, to_twin.value_of_columns(m, i), wid=i)
            for i in range(k))
        assert wire[: len(exp)].cpu().numpy().tobytes() == exp
    ms.sort()
    res = {"leg": leg, "n": n, "wire_bytes": W, "steps": steps, "warmup": warmup,
           "ms_mean": round(sum(ms) / len(ms), 4), "ms_median": round(ms[len(ms) // 2], 4),
           "ms_min": round(ms[0], 4), "ms_max": round(ms[-1], 4)}
    codec.close()
    return res


def judge(files):
    p1, p2, new = (json.load(open(f)) for f in files)
    out = {"parent_runs": [p1, p2], "new": new, "verdict": {}}
    for key in sorted(new["legs"]):
        leg, n = key.split("@")
        base = {"B": "A", "D": "C"}.get(leg, leg) + "@" + n
        a, b = p1["legs"][base]["ms_mean"], p2["legs"][base]["ms_mean"]
        mean, spread = (a + b) / 2, abs(a - b)
        scale = 1.0
        if leg in "BD":  # algorithmic traffic: the frame plus the columns, To over From
            wt = sum(new["legs"][key]["wire_bytes"]) / 3
            wf = sum(p1["legs"][base]["wire_bytes"]) / 3
            scale = (wt + 25 * int(n)) / (wf + 16 * int(n))
        bound = mean * scale + 2 * spread
        got = new["legs"][key]["ms_mean"]
        out["verdict"][key] = {"parent_mean_ms": round(mean, 4), "parent_spread_ms": round(spread, 4),
                               "scale": round(scale, 4), "bound_ms": round(bound, 4),
                               "new_ms": got, "ok": got <= bound}
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=list("ABCD"))
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per leg (timeout -k 10)")
    ap.add_argument("--legs", help="legs to run (default: ABCD, or AC without the To calls)")
    ap.add_argument("--label", default="")
    ap.add_argument("--out")
    ap.add_argument("--judge", nargs=3, metavar=("PARENT1", "PARENT2", "NEW"))
    a = ap.parse_args()
    if a.judge:
        return judge(a.judge)
    if a.leg:
        print(json.dumps(run_leg(a.leg, a.n[0], a.steps, a.warmup)), flush=True)
        return 0
    legs = a.legs or ("ABCD" if has_to_calls() else "AC")
    res = {"label": a.label, "legs": {}}
    for n in a.n:
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__),
                   "--leg", leg, "--n", str(n), "--steps", str(a.steps), "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:  # nothing more on the GPU after a failed leg
                print(f"leg {leg} at n={n} failed with exit status {p.returncode}", file=sys.stderr)
                return p.returncode
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res["legs"][f"{leg}@{n}"] = json.loads(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
