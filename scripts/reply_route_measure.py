#!/usr/bin/env python3
"""Times nxg_route_replies (include/nxg_codec.h) on a GPU, two cases, one JSON line each:

  burst   a frame of --n Subscribed(path, id, f64) spans, paths of 24-40 bytes, against --n pending
          requests (the reply to a reconnecting subscriber's Subscribe burst): every span SUBSCRIBED
  mixed   a frame of --n Updates over --n subscriptions (one stream each, 16 channels) with 1 %
          control messages among them: half Heartbeats, a quarter Unsubscribed of distinct live
          Ids, a quarter Subscribed of pending paths

  call_ms   the whole synchronous call, median of --reps (at least 20), wall clock around the C call
            after 2 * --rot warm-up calls, with its output arrays allocated beforehand. --rot
            frames, decoded columns and output buffers are used in turn.
Before anything is timed one call's counts are compared with what the frame was built to give."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vi(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def msg(body):
    return vi(len(body) + 1) + body if len(body) < 126 else vi(len(body) + 2) + body


def subscribed(path, id):
    return msg(b"\x03" + vi(len(path)) + path + vi(id) + b"\x09" + struct.pack(">Q", id))


def update(id):
    return msg(b"\x04" + vi(id) + b"\x09" + struct.pack(">Q", id))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rot", type=int, default=3)
    a = ap.parse_args()
    assert a.reps >= 20
    import torch
    import netidx_amd
    from netidx_amd import codec as cm
    from netidx_amd.codec import Columns, PathTable, ReplyTable, SubTable, HINT_MIXED, LAYOUT_MIXED
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    rng = np.random.default_rng(0x5EED0013)
    n = a.n

    def paths_of(m, tag):
        plen = rng.integers(24, 41, m)
        return [(b"/%s/%08x/" % (tag, i)).ljust(int(l), b"x") for i, l in enumerate(plen)]

    def pending_of(paths):
        pt = PathTable(codec, len(paths), sum(len(p) for p in paths))
        assert pt.insert(paths, np.arange(len(paths), dtype=np.uint64)) == 0
        return pt

    def measure(name, table, wires, n_slots, n_chans, want):
        tab = table.c_struct()
        sets = []
        for wire in wires:
            frame = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda()
            cols = Columns(n + 1, 1, n + 1, LAYOUT_MIXED, "cuda")
            codec.decode_into(frame, len(wire), cols, flags=HINT_MIXED)
            R, K = int(cols.s.n_rows), int(cols.s.n_ctl)
            t = lambda m, dt=torch.int64: torch.empty(max(m, 1), dtype=dt, device="cuda")
            bufs = [t(K, torch.uint8), t(K), t(K), t(n_chans + 1), t(R + K), t(R + K), t(n_slots),
                    t(K), t(K), t(K), t(K), t(K, torch.int32), t(12 * (R + K), torch.uint8)]
            o = cm.NxgReplyRoute()
            o.cap_spans, o.outcome, o.span_q, o.span_id = (max(K, 1), bufs[0].data_ptr(),
                                                           bufs[1].data_ptr(), bufs[2].data_ptr())
            o.disp = cm.NxgDispatch(R + K, bufs[3].data_ptr(), bufs[4].data_ptr(), bufs[5].data_ptr(),
                                    bufs[6].data_ptr(), 0, 0)
            o.cap_sub, o.sub_span, o.sub_q, o.sub_id = (K, bufs[7].data_ptr(), bufs[8].data_ptr(),
                                                        bufs[9].data_ptr())
            o.cap_unsub, o.unsub_id, o.unsub_slot = K, bufs[10].data_ptr(), bufs[11].data_ptr()
            o.cap_reply, o.reply = 12 * (R + K), bufs[12].data_ptr()
            sets.append((frame, cols, o, bufs, len(wire)))
        torch.cuda.synchronize()

        def call(s):
            err = cm.NetidxError()
            ok = cm.lib().nxg_route_replies(codec.ctx, C.byref(tab), C.c_void_p(s[0].data_ptr()),
                                            C.byref(s[1].s), 0, 0, C.byref(s[2]), C.byref(err))
            assert ok, err.msg

        call(sets[0])
        o = sets[0][2]
        got = {"n_entries": int(o.n_entries), "n_sub": int(o.n_sub), "n_unsub": int(o.n_unsub),
               "n_unmatched": int(o.disp.n_unmatched), "stopped": int(o.stopped)}
        assert got == want, (got, want)
        for k in range(2 * a.rot):
            call(sets[k % a.rot])
        ts = []
        for k in range(a.reps):
            t0 = time.perf_counter()
            call(sets[k % a.rot])
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"case": name, "rows": int(sets[0][1].s.n_rows),
                          "spans": int(sets[0][1].s.n_ctl), "frame_bytes": sets[0][4],
                          "rot": a.rot, "reps": a.reps,
                          "call_ms": round(statistics.median(ts) * 1e3, 3),
                          "call_ms_min": round(min(ts) * 1e3, 3), **got}), flush=True)

    # ---- burst: n Subscribed spans against n pending requests, Id i for request i -----------------
    paths = paths_of(n, b"stream")
    subs = SubTable(np.full(n, cm.NO_SLOT, np.uint32), np.arange(n, dtype=np.uint64) + 7,
                    np.arange(n + 1, dtype=np.uint32), np.arange(n, dtype=np.uint32) % 16,
                    np.ones(n, np.uint8), 16)
    table = ReplyTable(subs, pending_of(paths), np.arange(n, dtype=np.uint32))
    wires = [b"".join(subscribed(paths[i], int(i)) for i in rng.permutation(n)) for _ in range(a.rot)]
    measure("burst", table, wires, n, 16,
            {"n_entries": 0, "n_sub": n, "n_unsub": 0, "n_unmatched": 0, "stopped": 0})
    table.pending.close()
    del table, subs, wires

    # ---- mixed: n Updates over n subscriptions, 1 % control messages --------------------------------
    nc = max(n // 100, 4)
    nq = nc // 4
    ppaths = paths_of(nq, b"late")
    # slots 0 .. n - 1 the subscriptions of Ids 0 .. n - 1, then one per request; Ids n .. are new
    slots = n + nq
    subs = SubTable(np.concatenate([np.arange(n, dtype=np.uint32), np.full(nq, cm.NO_SLOT, np.uint32)]),
                    np.arange(slots, dtype=np.uint64) + 7, np.arange(slots + 1, dtype=np.uint32),
                    np.arange(slots, dtype=np.uint32) % 16, np.ones(slots, np.uint8), 16)
    table = ReplyTable(subs, pending_of(ppaths), np.arange(n, n + nq, dtype=np.uint32))
    wires = []
    for _ in range(a.rot):
        ids = rng.integers(0, n, n)
        gone = rng.permutation(n)[: nc // 4]
        ctl = [b"\x02\x05"] * (nc - nc // 4 - nq)  # Heartbeat: varint(L = 2) 05
        ctl += [msg(b"\x02" + vi(int(i))) for i in gone]
        ctl += [subscribed(ppaths[q], n + q) for q in range(nq)]
        order = rng.permutation(len(ctl))
        step = n // len(ctl)
        parts = []
        for j, c in enumerate(order):
            parts.append(b"".join(update(int(i)) for i in ids[j * step:(j + 1) * step]))
            parts.append(ctl[c])
        parts.append(b"".join(update(int(i)) for i in ids[len(ctl) * step:]))
        wires.append(b"".join(parts))
    # (the first frame's counts: how many rows follow their Id's Unsubscribed is not worth restating
    # here, so entries + unmatched = rows + unsubscribed spans is what is checked)
    measure_mixed_check = {"n_sub": nq, "n_unsub": nc // 4, "stopped": 0}

    def measure_mixed():
        # measure() with the split of entries / unmatched taken from the call itself
        frame = torch.from_numpy(np.frombuffer(wires[0], np.uint8).copy()).cuda()
        cols = Columns(n + 1, 1, n + 1, LAYOUT_MIXED, "cuda")
        codec.decode_into(frame, len(wires[0]), cols, flags=HINT_MIXED)
        r = codec.route_replies(table, frame, cols)
        assert r.n_entries + r.n_unmatched == n + nc // 4
        for k, v in measure_mixed_check.items():
            assert getattr(r, k) == v, k
        return {"n_entries": r.n_entries, "n_unmatched": r.n_unmatched, **measure_mixed_check}

    measure("mixed", table, wires, slots, 16, measure_mixed())
    codec.close()


if __name__ == "__main__":
    main()
