#!/usr/bin/env python3
"""Timing of nxg_record_entries against what a caller had to do before it. Shapes (N rows, every
Id subscribed once with one stream, SubIds a permutation of 0..N-1, dispatched on the device):
  1  F64 rows, 16 channels (the bench's dispatch shape)
  2  config 3's mixed rows, 16 channels
  3  shape 2 with half of the SubIds unmapped
  4  shape 2 over 1000 channels
Baseline, in the same process and alternated with the call, on the device: per channel, torch
gathers of the columns by ent_row, a translated and masked id column, and one
nxg_encode_archive_batch (size, allocate, encode, as Codec.encode_archive does); an F64 batch is
widened to MIXED columns first, inside the timed part. Before timing, the call's records must equal
the baseline's byte for byte. Windows of at least 0.25 s of calls, each ending in a device
synchronise; medians of 7.
usage: python3 scripts/record_measure.py [--n 10000000] [--shapes 1,2,3,4] [--only-a]
--only-a: the check and three calls per shape, no baseline timing, for a separate `rocprofv3
--kernel-trace --stats` run (its kernel_stats.csv gives the per-kernel times); every line states
the bytes each kernel moves, computed here from the shape, to put beside them."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    import netidx_amd
    from netidx_amd import synth
    from netidx_amd.codec import Columns, LAYOUT_MIXED, SubTable

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="1,2,3,4")
    ap.add_argument("--only-a", action="store_true")
    args = ap.parse_args()
    n = args.n
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

    def baseline(cols, heap, disp, tab64, n_chans, spare):
        """[record tensor per channel] by the calls the library had: gathers and one
        nxg_encode_archive_batch per channel."""
        f64 = cols.t.get("tag") is None
        off = disp.chan_off.cpu().tolist()
        out = []
        if f64:  # widened to MIXED columns first
            wtag = torch.full((int(cols.s.n_rows),), 9, dtype=torch.uint8, device="cuda")
            waux = torch.zeros(int(cols.s.n_rows), dtype=torch.int32, device="cuda")
        for c in range(n_chans):
            sub, row = disp.ent_sub[off[c]:off[c + 1]], disp.ent_row[off[c]:off[c + 1]]
            known = (sub >= 0) & (sub < tab64.numel())
            aid = torch.where(known, tab64[torch.where(known, sub, 0)], 0xFFFFFFFF)
            keep = aid != 0xFFFFFFFF
            aid, row = aid[keep], row[keep]
            if not aid.numel():
                out.append(None)
                continue
            tag = (wtag if f64 else cols.tag)[row]
            fixed = cols.fixed[row]
            aux = (waux if f64 else cols.aux)[row]
            s = spare.s
            s.cap_rows = s.n_rows = aid.numel()
            s.id, s.tag, s.fixed, s.aux = (aid.data_ptr(), tag.data_ptr(), fixed.data_ptr(),
                                           aux.data_ptr())
            if not f64 and cols.s.n_children:
                s.cap_children = s.n_children = cols.s.n_children
                s.ctag, s.cfixed, s.caux = cols.s.ctag, cols.s.cfixed, cols.s.caux
            torch.cuda.synchronize()  # (torch's stream before the codec's)
            out.append(codec.encode_archive(types.SimpleNamespace(s=s, id=aid), heap))
        return out

    def run(shape, what, cols, heap, n_rows, n_chans, unmapped):
        rng = np.random.default_rng(0x5EED0008 + shape)
        sub_id = rng.permutation(n_rows).astype(np.uint64)
        tab = SubTable(np.arange(n_rows, dtype=np.uint32), sub_id,
                       np.arange(n_rows + 1, dtype=np.uint32),
                       rng.integers(0, n_chans, n_rows, dtype=np.uint32),
                       np.zeros(n_rows, np.uint8), n_chans)
        disp = codec.dispatch_updates(tab, cols.id, n_rows, cap=n_rows)
        arch = (np.arange(n_rows, dtype=np.uint64) * 2654435761 % (1 << 28)).astype(np.uint32)
        if unmapped:
            arch[rng.random(n_rows) < unmapped] = 0xFFFFFFFF
        table = cu(arch, np.int32)
        tab64 = table.to(torch.int64) & 0xFFFFFFFF
        spare = Columns(1, 1, 1, LAYOUT_MIXED, "cuda")
        nb, rec_off, rec_items, dropped = codec.recorded_len(cols, disp, table, heap)
        out = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def a():
            codec.record_entries_into(cols, disp, table, heap, out.data_ptr(), nb, rec_off,
                                      rec_items)

        def b():
            baseline(cols, heap, disp, tab64, n_chans, spare)

        a()
        torch.cuda.synchronize()
        off = rec_off.cpu().tolist()
        for c, rec in enumerate(baseline(cols, heap, disp, tab64, n_chans, spare)):
            mine = out[off[c]:off[c + 1]]
            assert (rec is None and mine.numel() == 0) or torch.equal(mine, rec), (shape, c)
        ne = int(disp.n_entries)
        kept = ne - dropped
        f64 = cols.t.get("tag") is None
        row_b = 8 if f64 else 13
        # per kernel: what it reads and writes (entry list, table lookups, the rows' columns, the
        # per-entry lengths, the output); children and payload bytes are inside (nb - 5 * kept)
        kb = dict(size=16 * ne + 4 * kept + row_b * kept + 4 * ne,
                  top=2 * 16 * (ne // 256 + 1),
                  emit=4 * ne + 16 * kept + 4 * kept + row_b * kept + 2 * nb)
        common = dict(shape=shape, what=what, n=n_rows, channels=n_chans, entries=ne, kept=kept,
                      n_bytes=nb, kernel_bytes=kb)
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
        algo = sum(kb.values())
        print(json.dumps(dict(a_ms=round(ma, 4), b_ms=round(mb, 4),
                              a_range=[round(min(ta), 4), round(max(ta), 4)],
                              b_range=[round(min(tb), 4), round(max(tb), 4)],
                              b_over_a=round(mb / ma, 2),
                              a_call_share_of_8TBps=round(algo / (ma * 1e-3) / 8e12, 4),
                              **common)), flush=True)

    if 1 in shapes:
        ids, vals = synth.f64_columns(n)
        ids = np.arange(n, dtype=np.uint64)  # every Id subscribed once: Ids 0..n-1
        cols = netidx_amd.columns_from_arrays(ids, vals)
        run(1, "f64, 16 channels", cols, None, n, 16, 0)
        del cols
    if any(s in shapes for s in (2, 3, 4)):
        m = synth.mixed_columns(n)
        cols = netidx_amd.columns_from_arrays(m.id, m.fixed, m.tag, m.aux, m.ctag, m.cfixed, m.caux)
        heap = cu(m.heap.copy())
        if 2 in shapes:
            run(2, "config 3 mixed, 16 channels", cols, heap, n, 16, 0)
        if 3 in shapes:
            run(3, "config 3 mixed, 16 channels, half unmapped", cols, heap, n, 16, 0.5)
        if 4 in shapes:
            run(4, "config 3 mixed, 1000 channels", cols, heap, n, 1000, 0)
    codec.close()


if __name__ == "__main__":
    main()
