#!/usr/bin/env python3
"""A/B timing of the commit's per-client encode: (a) nxg_encode_clients, one call for all
clients, against (b) what the library offered before it: per client, torch.index_select of every
column by the client's ent_row segment, then nxg_encode_updates into that client's slice of the
output. Two shapes: bench.py's commit shape (F64 layout), and config 3's mixed columns under the
same routing. Both runs must produce identical bytes before anything is timed; they are warmed,
alternated in one process, each window at least 0.25 s of wall time ending in a device
synchronise; medians of 7 windows.
usage: python3 scripts/ab_client_frames.py [--n 10000000] [--only-a] [--shape f64|mixed]
       python3 scripts/ab_client_frames.py --share RESULTS.db ONLY_A.jsonl
--only-a: a few calls of (a) alone, for a separate `rocprofv3 --kernel-trace --stats` run; --share
then reads that run's database and the lines it printed and states each new kernel's time and
its share of 8 TB/s from the algorithmic bytes (8 E of ent_row, 16 E or 21 E of gathered columns
plus the text, Decimal, Abstract and array-element bytes the entries name, and the output)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


KERNEL_OF = {"f64": "nxg_enc_f64_gather_kernel", "mixed": "nxg_enc_rows_gather_kernel"}


def share(db, jsonl):
    """Per shape: the new kernel's launches in a rocprofv3 database (the median is a writing
    launch: one sizing launch, six writing ones) against the algorithmic bytes."""
    import sqlite3
    con = sqlite3.connect(db)
    for line in open(jsonl):
        if not line.startswith("{"):
            continue
        r = json.loads(line)
        ns = sorted(x[0] for x in con.execute(
            "select end - start from kernels where name like ?", (KERNEL_OF[r["shape"]] + "%",)))
        med = statistics.median(ns) * 1e-6
        print(json.dumps({"shape": r["shape"], "kernel": KERNEL_OF[r["shape"]], "launches": len(ns),
                          "kernel_ms_median": round(med, 4), "kernel_ms_min": round(ns[0] * 1e-6, 4),
                          "kernel_ms_max": round(ns[-1] * 1e-6, 4),
                          "algorithmic_bytes": r["algorithmic_bytes"],
                          "kernel_share_of_8TBps": round(
                              r["algorithmic_bytes"] / (med * 1e-3) / 8e12, 4)}), flush=True)


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--share":
        return share(sys.argv[2], sys.argv[3])
    import numpy as np
    import torch
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import Columns
    import client_frames_cases as cfc

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--shape", choices=("f64", "mixed"), default=None)
    args = ap.parse_args()
    n = args.n
    codec = netidx_amd.Codec(0)
    s = cfc.commit_shape(n)
    tab = netidx_amd.PubTable(s.slot_of_id, s.off, s.client, s.n_clients, None, s.cur)
    fbatch = netidx_amd.columns_from_arrays(s.ids, s.vals)
    d = codec.publish_commit(tab, fbatch, torch.from_numpy(s.kind).cuda(), cap=int(s.off[-1]))
    E = int(d.n_entries)
    chan = d.chan_off.cpu().numpy().view(np.uint64).astype(np.int64)
    segs = [d.ent_row[chan[c]:chan[c + 1]] for c in range(s.n_clients)]

    def shape(name):
        if name == "f64":
            return fbatch, None, ("id", "fixed"), 16 * E, 0
        m = synth.mixed_columns(n)
        mc = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
        heap = torch.from_numpy(m.heap.copy()).cuda()
        # what the entries' values name beyond their row: text / Abstract bytes, a Decimal's 16,
        # an array's elements (13 bytes of child columns each)
        aux = m.aux.astype(np.int64)
        per_row = (np.where(np.isin(m.tag, (12, 13, 18, 27)), aux, 0) +
                   np.where(m.tag == 20, 16, 0) + np.where(m.tag == 19, 13 * aux, 0))
        rows = d.ent_row[:E].cpu().numpy().view(np.uint64).astype(np.int64)
        return mc, heap, ("id", "fixed", "tag", "aux"), 21 * E, int(per_row[rows].sum())

    for name in ([args.shape] if args.shape else ["f64", "mixed"]):
        batch, heap, fields, col_bytes, value_bytes = shape(name)
        nb, off = codec.encoded_clients_len(batch, d, heap)
        algo = 8 * E + col_bytes + value_bytes + nb  # ent_row, gathered columns, output
        out_a = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
        out_b = torch.empty(nb + 64, dtype=torch.uint8, device="cuda")
        hoff = off.cpu().numpy().view(np.uint64).astype(np.int64)
        # (b)'s per-client column sets, allocated once; the children stay the batch's
        per = []
        for c in range(s.n_clients):
            k = int(segs[c].numel())
            cc = Columns(max(k, 1), 0, 0, batch.s.layout, "cuda")
            cc.s.n_rows = k
            if batch.s.layout != netidx_amd.LAYOUT_F64:
                cc.s.ctag, cc.s.cfixed, cc.s.caux = batch.s.ctag, batch.s.cfixed, batch.s.caux
                cc.s.cap_children, cc.s.n_children = batch.s.cap_children, batch.s.n_children
            per.append(cc)

        def run_a():
            codec.encode_clients_into(batch, d, heap, out_a.data_ptr(), nb, off)

        def run_b():
            for c in range(s.n_clients):
                k = int(segs[c].numel())
                if not k:
                    continue
                for f in fields:
                    torch.index_select(getattr(batch, f)[: batch.s.n_rows], 0, segs[c],
                                       out=getattr(per[c], f)[:k])
                torch.cuda.synchronize()  # torch's stream before the codec's
                codec.encode_into(per[c], heap, out_b.data_ptr() + int(hoff[c]),
                                  int(hoff[c + 1] - hoff[c]))

        run_a()
        torch.cuda.synchronize()
        if args.only_a:
            for _ in range(5):
                run_a()
            torch.cuda.synchronize()
            print(json.dumps({"shape": name, "n": n, "entries": E, "bytes": nb, "only_a": True,
                              "algorithmic_bytes": algo}),
                  flush=True)
            continue
        run_b()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a[:nb], out_b[:nb]))
        assert same, "the two runs differ"

        def window(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            while True:
                fn()
                k += 1
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= 0.25:
                    return dt / k * 1e3

        for fn in (run_a, run_b):
            for _ in range(3):
                fn()
        ta, tb = [], []
        for _ in range(7):
            ta.append(window(run_a))
            tb.append(window(run_b))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps({"shape": name, "n": n, "clients": s.n_clients, "entries": E,
                          "bytes": nb, "identical": same, "a_ms": round(ma, 4),
                          "b_ms": round(mb, 4), "a_windows_ms": [round(x, 4) for x in ta],
                          "b_windows_ms": [round(x, 4) for x in tb],
                          "speedup": round(mb / ma, 2), "algorithmic_bytes": algo,
                          # (host wall time of the synchronous call, not the kernel's: --share)
                          "a_call_wall_bytes_over_8TBps": round(algo / (ma * 1e-3) / 8e12, 4)}),
              flush=True)
    codec.close()


if __name__ == "__main__":
    main()
