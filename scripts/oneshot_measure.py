#!/usr/bin/env python3
"""Timing of nxg_oneshot_pack_deltas and nxg_oneshot_pack_pathmap against what a caller had before
them. Shapes:
  1-3  deltas: a window of R records x M items (oneshot's own window: 1000 x 1000), F64 values,
       Ids drawn from 1.25 M, with a filter that keeps 1 %, 50 % and 100 % of the Ids
  4-5  pathmap: N Ids (10^6) with paths of 20 to 60 bytes, 1 % and 100 % kept
Other legs, in the same process and alternated with the call:
  deltas   the calls the library had before: nxg_replay_window as the row filter (a table that
           maps a selected Id to itself and every other Id to NXG_REPLAY_DROP), rec_off read back,
           one nxg_encode_archive_batch per kept record 12 bytes behind the end of the record
           before, the timestamps glued in by one scatter from the host. The same bytes.
           Reported beside it (host_ms): the columns copied to the host and the numpy / oracle
           restatement of tests/oneshot_model.py.
  pathmap  the numpy restatement of tests/oneshot_model.py over arrays already on the host
Before timing, the call's results must equal the model's (and the other leg's bytes the call's).
Windows of at least 0.25 s of calls, each ending in a device synchronise; medians of 7.
usage: python3 scripts/oneshot_measure.py [--records 1000] [--items 1000] [--ids 1000000]
       [--shapes 1,2,3,4,5] [--only-a]
--only-a: the check and three calls per shape, no other leg, for a separate `rocprofv3
--kernel-trace --stats` run (its kernel_stats.csv gives the per-kernel times)."""
import argparse
import json
import os
import statistics
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import netidx_amd
    import oneshot_model as om
    from netidx_amd.codec import REPLAY_DROP, ReplayRows
    from value_table_model import Source

    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=1000)
    ap.add_argument("--items", type=int, default=1000)
    ap.add_argument("--ids", type=int, default=1_000_000)
    ap.add_argument("--shapes", default="1,2,3,4,5")
    ap.add_argument("--only-a", action="store_true")
    args = ap.parse_args()
    shapes = [int(x) for x in args.shapes.split(",")]
    codec = netidx_amd.Codec(0)
    cu = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a).view(dt) if dt else a).cuda()

    def window(fn):
        total, k = 0.0, 0
        while total < 0.25:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
            k += 1
        return total / k * 1e3

    def report(a, b, common, **more):
        if args.only_a:
            for _ in range(3):
                a()
            torch.cuda.synchronize()
            print(json.dumps(dict(only_a=True, **common)), flush=True)
            return
        ta, tb = [], []
        for _ in range(7):
            ta.append(window(a))
            tb.append(window(b))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(json.dumps(dict(a_ms=round(ma, 4), b_ms=round(mb, 4),
                              a_range=[round(min(ta), 4), round(max(ta), 4)],
                              b_range=[round(min(tb), 4), round(max(tb), 4)],
                              b_over_a=round(mb / ma, 2), **common, **more)), flush=True)

    def deltas(shape, frac):
        R, M = args.records, args.items
        n, n_ids = R * M, 1_250_000
        rng = np.random.default_rng(0x0E50 + shape)
        ids = rng.integers(0, n_ids, n, dtype=np.uint64)
        vals = rng.standard_normal(n).view(np.uint64)
        sel = (rng.random(n_ids) < frac).astype(np.uint8) if frac < 1 else np.ones(n_ids, np.uint8)
        recs = [(i * M, M) for i in range(R)]
        secs = [1_700_000_000 + i for i in range(R)]
        nanos = [(i * 999_983) % 1_000_000_000 for i in range(R)]
        cols = netidx_amd.columns_from_arrays(ids, vals, np.full(n, 9, np.uint8),
                                              np.zeros(n, np.uint32))
        dsel = cu(sel)
        nb, rec_off, rec_items, _, _, kept_recs = codec.oneshot_pack_deltas_into(
            cols, recs, secs, nanos, dsel, None, None, 0)
        out = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def a():
            codec.oneshot_pack_deltas_into(cols, recs, secs, nanos, dsel, None, out.data_ptr(), nb,
                                           rec_off, rec_items)

        # the library before this call
        table = cu(np.where(sel != 0, np.arange(n_ids, dtype=np.uint64), np.uint64(REPLAY_DROP)),
                   np.int64)
        rows = ReplayRows(n, R, 0, "cuda")
        out_b = torch.empty(max(nb, 16) + 16, dtype=torch.uint8, device="cuda")
        stamps = [np.frombuffer(struct.pack(">qI", secs[i], nanos[i]), np.uint8) for i in range(R)]
        twelve = np.arange(12)

        def b():
            codec.replay_window(cols, recs, table, out=rows)
            off = rows.offsets()
            p, at, ts = 0, [], []
            for i in range(R):
                if off[i + 1] > off[i]:
                    ln = codec.encode_archive(rows.record(i, cols), None, out=out_b[p + 12:])
                    at.append(p + twelve)
                    ts.append(stamps[i])
                    p += 12 + ln
            if at:
                out_b[torch.from_numpy(np.concatenate(at)).cuda()] = \
                    torch.from_numpy(np.concatenate(ts)).cuda()
            return p

        win = om.Window(Source(np.full(n, 9, np.uint8), vals, np.zeros(n, np.uint32)), ids, recs,
                        secs, nanos, n_ids, np.flatnonzero(sel))

        def host():
            g = cols.numpy()
            w = om.Window(Source(g["tag"], g["fixed"], g["aux"]), g["id"], recs, secs, nanos,
                          n_ids, win.selected)
            return b"".join(om.deltas_oracle(w))

        a()
        torch.cuda.synchronize()
        want = host()
        assert out[:nb].cpu().numpy().tobytes() == want, shape
        common = dict(shape=shape, what=f"deltas, {R} records x {M} items, {frac:g} of the Ids kept",
                      rows=n, n_bytes=nb, kept_records=kept_recs)
        if args.only_a:
            report(a, None, common)
            return
        assert b() == nb and out_b[:nb].cpu().numpy().tobytes() == want, shape
        report(a, b, common, b_what="replay_window + encode_archive_batch per record + timestamps",
               host_ms=round(min(window(host) for _ in range(2)), 2))

    def pathmap(shape, frac):
        n = args.ids
        rng = np.random.default_rng(0x0E60 + shape)
        plen = rng.integers(20, 61, n)
        off = np.concatenate([[0], np.cumsum(plen)]).astype(np.uint64)
        blob = rng.integers(97, 123, int(off[-1]), dtype=np.uint8)
        keep = (rng.random(n) < frac).astype(np.uint8) if frac < 1 else np.ones(n, np.uint8)
        doff, dblob, dkeep = cu(off, np.int64), cu(blob), cu(keep)
        nb, sel, n_sel = codec.oneshot_pack_pathmap_into(doff, dblob, dkeep, None, 0)
        out = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def a():
            codec.oneshot_pack_pathmap_into(doff, dblob, dkeep, out.data_ptr(), nb, sel)

        class P:  # (om.Paths without a list of a million bytes objects)
            n_ids = n
            path_off = staticmethod(lambda: off)
            path_bytes = staticmethod(lambda: blob)
        P.keep = keep

        def host():
            return om.pathmap_numpy(P)

        a()
        torch.cuda.synchronize()
        want, wsel, wn = host()
        assert out[:nb].cpu().numpy().tobytes() == want and wn == n_sel, shape
        assert np.array_equal(sel.cpu().numpy()[:n], wsel)
        common = dict(shape=shape, what=f"pathmap, {n} Ids, {frac:g} kept", ids=n, n_sel=n_sel,
                      n_bytes=nb, path_bytes=int(off[-1]))
        report(a, host, common, b_what="numpy restatement on the host")

    for shape, frac in ((1, 0.01), (2, 0.5), (3, 1.0)):
        if shape in shapes:
            deltas(shape, frac)
    for shape, frac in ((4, 0.01), (5, 1.0)):
        if shape in shapes:
            pathmap(shape, frac)
    codec.close()


if __name__ == "__main__":
    main()
