#!/usr/bin/env python3
"""Times nxg_route_subscribes (include/nxg_codec.h) on a GPU: a burst of --n anonymous Subscribes
with paths of 24-40 bytes against a table of --n published f64 values, every path published (the
durable subscriber's reconnect). Prints one JSON line.

  route_ms        the whole synchronous call, median of --reps, wall clock around the C call with
                  its output arrays allocated beforehand. --rot frames, decoded columns and reply
                  buffers are used in turn, so that with the table and the scratch the working set
                  is past the 256 MiB cache.
  insert_ms       nxg_path_table_insert of the --n paths into an empty table (host arrays in, one
                  call), median of 3 tables
  host_ms         the same burst on one host thread: unordered_map lookups plus nxg_msg_subscribed
                  (scripts/subscribe_host_baseline.cpp, compiled on first use), median of 5 passes
  bytes           the algorithmic bytes of a call: the spans' frame bytes and control columns, a
                  probe per span (hash word, key length, offset, Id and the key's bytes), slot_of_id
                  and cur_fixed, the reply, outcome / span_id / sub_id / sub_perm
Before anything is timed one call's reply, sub_id and counts are compared with replies built here.
--calls N: only N untimed calls (for a kernel trace)."""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
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


def host_baseline(paths, reps):
    exe = os.path.join(ROOT, "scripts", "subscribe_host_baseline")
    src = exe + ".cpp"
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", exe, "-ldl"], check=True)
    from netidx_amd.codec import LIB_PATH
    off = np.zeros(len(paths) + 1, np.uint64)
    off[1:] = np.cumsum([len(p) for p in paths], dtype=np.uint64)
    with tempfile.NamedTemporaryFile(suffix=".paths") as f:
        f.write(struct.pack("<Q", len(paths)) + off.tobytes() + b"".join(paths))
        f.flush()
        out = subprocess.run([exe, LIB_PATH, f.name, str(reps)], check=True, capture_output=True)
    return json.loads(out.stdout)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--rot", type=int, default=4)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch
    import netidx_amd
    from netidx_amd import codec as cm
    from netidx_amd.codec import Columns, WriteCols, PathTable, PubTable, SubscribeTable, LAYOUT_MIXED
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    rng = np.random.default_rng(0x5EED0012)
    n = a.n
    # /stream/<8 hex>/<filler>: 24-40 bytes, unique through the index
    plen = rng.integers(24, 41, n)
    paths = [(b"/stream/%08x/" % i + b"abcdefghijklmnopqrstuvwxyz"[: int(l) - 17]) for i, l in enumerate(plen)]
    assert all(len(p) == l for p, l in zip(paths, plen))
    total = int(plen.sum())
    # the table: path i -> Id i, current value the F64 with bit pattern i
    t_ins = []
    for _ in range(3):
        pt = PathTable(codec, n, total)
        ps, heap, off = cm._pack_paths(paths)
        ids = np.arange(n, dtype=np.uint64)
        dup, err = C.c_uint64(), cm.NetidxError()
        t0 = time.perf_counter()
        ok = cm.lib().nxg_path_table_insert(codec.ctx, pt.h, heap.ctypes.data, off.ctypes.data,
                                            ids.ctypes.data, n, C.byref(dup), C.byref(err))
        t_ins.append(time.perf_counter() - t0)
        assert ok and dup.value == 0 and len(pt) == n
    pub = PubTable(np.arange(n, dtype=np.uint32), [0] * (n + 1), [], 0, None,
                   np.arange(n, dtype=np.uint64))
    table = SubscribeTable(pt, pub)
    tab = table.c_struct()
    # --rot frames of the same burst in different orders, decoded
    sets = []
    tail = b"\x00" + struct.pack(">IH", 0x7F000001, 4242)  # the resolver's SocketAddr
    for r in range(a.rot):
        order = rng.permutation(n)
        msgs = []
        for k, i in enumerate(order):
            p = paths[i]
            body = b"\x00" + vi(len(p)) + p + tail + struct.pack(">QI", k, 0x3F) + b"\x04tokn"
            msgs.append(vi(len(body) + 1) + body)  # L = lw(|body|): one byte here
        wire = b"".join(msgs)
        frame = torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda()
        cols = Columns(1, 1, n + 1, LAYOUT_MIXED, "cuda")
        wcols = WriteCols(1, "cuda")
        codec.decode_writes(frame, cols, wcols)
        assert cols.s.n_ctl == n and cols.s.n_rows == 0
        out = cm.NxgSubscribeRoute()
        bufs = [torch.empty(n, dtype=torch.uint8, device="cuda"),
                torch.empty(n, dtype=torch.int64, device="cuda"),
                torch.empty(n, dtype=torch.int64, device="cuda"),
                torch.empty(n, dtype=torch.int32, device="cuda"),
                torch.empty(len(wire), dtype=torch.uint8, device="cuda")]
        out.cap_spans, out.outcome, out.span_id = n, bufs[0].data_ptr(), bufs[1].data_ptr()
        out.cap_sub, out.sub_id, out.sub_perm = n, bufs[2].data_ptr(), bufs[3].data_ptr()
        out.cap_reply, out.reply = len(wire), bufs[4].data_ptr()
        sets.append((frame, cols, wcols, out, bufs, order, len(wire)))
    torch.cuda.synchronize()

    def call(s):
        err = cm.NetidxError()
        ok = cm.lib().nxg_route_subscribes(codec.ctx, C.byref(tab), C.c_void_p(s[0].data_ptr()),
                                           C.byref(s[1].s), 0, 0, None, C.byref(s[3]), C.byref(err))
        assert ok, err.msg

    # check one call: Subscribed(path, id, F64 bits = id) in the frame's order
    s = sets[0]
    call(s)
    order = s[5]
    want = bytearray()
    for i in order[:2000]:
        body = b"\x03" + vi(len(paths[i])) + paths[i] + vi(int(i)) + b"\x09" + struct.pack(">Q", int(i))
        want += vi(len(body) + 1) + body
    o = s[3]
    assert (o.n_sub, o.n_replies, o.next_ctl, o.stopped) == (n, n, n, 0)
    assert s[4][4][: len(want)].cpu().numpy().tobytes() == bytes(want)
    assert np.array_equal(s[4][2].cpu().numpy(), order.astype(np.int64))
    if a.calls:
        for k in range(a.calls):
            call(sets[k % a.rot])
        codec.close()
        return
    for k in range(2 * a.rot):
        call(sets[k % a.rot])
    t = []
    for k in range(a.reps):
        t0 = time.perf_counter()
        call(sets[k % a.rot])
        t.append(time.perf_counter() - t0)
    ms = statistics.median(t) * 1e3
    span_bytes = s[6]
    algo = (span_bytes + n * 21                    # the frame's spans, ctl_variant / row / off / len
            + n * (8 + 4 + 8 + 8) + total          # a probe: hash, key_len, key_off, id, the key
            + n * (4 + 8)                          # slot_of_id, cur_fixed
            + int(o.reply_len) + n * (1 + 8 + 8 + 4))  # the reply, outcome, span_id, sub_id, sub_perm
    res = {"subscribes": n, "frame_bytes": span_bytes, "path_bytes": total,
           "reply_bytes": int(o.reply_len), "rot": a.rot, "reps": a.reps,
           "route_ms": round(ms, 3), "route_ms_min": round(min(t) * 1e3, 3),
           "insert_ms": round(statistics.median(t_ins) * 1e3, 3),
           "algorithmic_bytes": algo, "gb_per_s": round(algo / ms / 1e6, 1),
           "fraction_of_8_tb_s": round(algo / ms / 1e6 / 8000, 4)}
    if not a.no_host:
        res.update(host_baseline(paths, 5))
        res["host_over_route"] = round(res["host_ms"] / ms, 1)
    print(json.dumps(res), flush=True)
    codec.close()


if __name__ == "__main__":
    main()
