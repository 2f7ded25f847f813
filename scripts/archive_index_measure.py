#!/usr/bin/env python3
"""Timing of nxg_archive_index_records and nxg_archive_scan_index against the host paths they
replace. Shapes:
  1  writer: N positions in 16 records, Ids drawn from N/8 (each record repeats Ids)
  2  writer: N positions in 1000 records
  3  scan: a window of R records with 1000-Id indexes (each in front of a 4 KiB batch), a filter
     that keeps 1 % of the Ids (nearly every record matches, most of them early)
  4  shape 3 with a filter that keeps one Id in 10^5 (nearly every index is walked to its end)
Host paths, in the same process and alternated with the call:
  writer  the keys copied to the host, then per record numpy's first occurrences (np.unique with
          return_index, sorted back into position order); the varints are not even encoded
  scan    the walk of tests/archive_index_model.py's scan_index_at (Python), and a numpy walk
          (terminator bytes -> varint starts -> values by reduceat -> keep gather, per record),
          both over bytes already on the host
Before timing, the call's results must equal the model's. Windows of at least 0.25 s of calls, each
ending in a device synchronise; medians of 7.
usage: python3 scripts/archive_index_measure.py [--n 10000000] [--records 10000] [--shapes 1,2,3,4]
       [--only-a]
--only-a: the check and three calls per shape, no host timing, for a separate `rocprofv3
--kernel-trace --stats` run (its kernel_stats.csv gives the per-kernel times)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import torch
    import netidx_amd
    import archive_index_model as am

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--records", type=int, default=10_000)
    ap.add_argument("--shapes", default="1,2,3,4")
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

    def writer(shape, n, n_recs):
        rng = np.random.default_rng(0xA1D0 + shape)
        key = rng.integers(0, max(n // 8, 1), n, dtype=np.uint64)
        cuts = np.sort(rng.integers(0, n + 1, n_recs - 1))
        seg = np.concatenate([[0], cuts, [n]]).astype(np.uint64)
        dkey, dseg = cu(key, np.int64), cu(seg, np.int64)
        nb, idx_off, idx_ids, total = codec.index_records_into(dkey, dseg, None, None, 0)
        out = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def a():
            codec.index_records_into(dkey, dseg, None, out.data_ptr(), nb, idx_off, idx_ids)

        def host_firsts():
            k = dkey.cpu().numpy()
            s = dseg.cpu().numpy()
            res = []
            for c in range(n_recs):
                r = k[s[c]:s[c + 1]]
                _, first = np.unique(r, return_index=True)
                res.append(r[np.sort(first)])
            return res

        a()
        torch.cuda.synchronize()
        blob, woff, wids = am.indexes_numpy(am.Case(key, seg))
        assert out[:nb].cpu().numpy().tobytes() == blob, shape
        assert np.array_equal(idx_off.cpu().numpy().view(np.uint64), woff)
        assert np.array_equal(idx_ids.cpu().numpy().view(np.uint64), wids)
        firsts = host_firsts()
        assert [len(f) for f in firsts] == [int(x) for x in wids]
        bits = 10
        while (1 << bits) < 2 * n:
            bits += 1
        common = dict(shape=shape, what=f"writer, {n_recs} records", n=n, records=n_recs,
                      ids=int(total), n_bytes=nb, table_bytes=12 << bits)
        report(a, host_firsts, common)

    def scan(shape, n_recs, frac):
        rng = np.random.default_rng(0xA1D3)
        n_ids = 1 << 20
        keep = (rng.random(n_ids) < frac).astype(np.uint8)
        buf, offs, ends = bytearray(), [], []
        for _ in range(n_recs):
            ids = rng.choice(n_ids, 1000, replace=False)
            buf += b"\0" * (4 + int(rng.integers(0, 16)))  # (the u32 of a compressed record)
            offs.append(len(buf))
            buf += am.record_index([int(i) for i in ids])
            buf += bytes(4096)  # the batch
            ends.append(len(buf))
        host = bytes(buf)
        dbuf, dkeep = cu(np.frombuffer(host, np.uint8).copy()), cu(keep)
        offs, ends = np.array(offs, np.uint64), np.array(ends, np.uint64)
        torch.cuda.synchronize()
        res = {}

        def a():
            res["a"] = codec.scan_index(dbuf, offs, ends, dkeep)

        def python_walk():
            return [am.scan_index_at(host, int(o), int(e), keep) for o, e in zip(offs, ends)]

        hb = np.frombuffer(host, np.uint8)

        def numpy_walk():
            """Well-formed indexes only: the starts from the terminator bytes, the values from the
            7-bit groups (at most 3 bytes here), one keep gather per record."""
            out = np.zeros(n_recs, np.uint8)
            for i in range(n_recs):
                o = int(offs[i])
                L, p = am.decode_varint(host[o:o + 10], 0)
                body = hb[o + p:o + p + L - am.varint_len(L)]
                term = body < 0x80
                start = np.concatenate([[0], np.flatnonzero(term)[:-1] + 1])
                pos = np.arange(len(body)) - np.repeat(start, np.diff(np.append(start, len(body))))
                val = np.add.reduceat((body & 0x7F).astype(np.int64) << (7 * pos), start)
                out[i] = keep[val[val < n_ids]].any()
            return out

        a()
        want = python_walk()
        assert res["a"][0].tolist() == want and res["a"][1] == want.count(am.MATCH)
        assert numpy_walk().tolist() == want
        common = dict(shape=shape,
                      what=f"scan, {n_recs} records of 1000 Ids, {frac:g} of the Ids kept",
                      records=n_recs, buffer_bytes=len(host), matches=want.count(am.MATCH))
        if args.only_a:
            report(a, None, common)
            return
        report(a, numpy_walk, common, b_what="numpy walk",
               python_walk_ms=round(min(window(python_walk) for _ in range(3)), 2))

    if 1 in shapes:
        writer(1, args.n, 16)
    if 2 in shapes:
        writer(2, args.n, 1000)
    if 3 in shapes:
        scan(3, args.records, 0.01)
    if 4 in shapes:
        scan(4, args.records, 1e-5)
    codec.close()


if __name__ == "__main__":
    main()
