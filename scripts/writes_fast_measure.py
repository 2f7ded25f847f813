#!/usr/bin/env python3
"""Times Codec.decode_writes(fast=True) (nxg_decode_writes_opts, the fast To decoder) against
fast=False (nxg_decode_writes, the general decoder) on a GPU, on two frames:

  subscribes   the burst of scripts/subscribe_route_measure.py: --n anonymous Subscribes with
               paths of 24-40 bytes
  writes       the frame of scripts/write_route_measure.py: --n To::Write messages (f64 values,
               one Id in a hundred wider than 35 bits) with one To::Unsubscribe per 100 writes

Per frame, --rot copies in different orders / from different draws are decoded in turn, so that
with their columns the working set is not simply cache-resident. First fast=True is compared with
fast=False array for array (every column, wflags, wid, the control spans, the counts) and must
report path 8. Then each leg is the median of --reps synchronous calls, the two legs alternating
in one process; before each timed call comes an untimed call of the same kind on the previous
copy. Wall clock around the Python call (a ctypes call and a status read; the same for both legs).
Prints one JSON line per frame.

--calls N --leg fast|general: only N untimed calls of one leg on one frame (for a kernel trace:
rocprofv3 --kernel-trace --stats -- python scripts/writes_fast_measure.py --frame writes --calls 8
--leg fast). Run every invocation under a time limit of its own."""
import argparse
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


def subscribe_frames(n, rot, rng):
    """The burst of subscribe_route_measure.py, in `rot` different orders."""
    import torch
    plen = rng.integers(24, 41, n)
    paths = [(b"/stream/%08x/" % i + b"abcdefghijklmnopqrstuvwxyz"[: int(l) - 17])
             for i, l in enumerate(plen)]
    tail = b"\x00" + struct.pack(">IH", 0x7F000001, 4242)  # the resolver's SocketAddr
    frames = []
    for _ in range(rot):
        msgs = []
        for k, i in enumerate(rng.permutation(n)):
            p = paths[i]
            body = b"\x00" + vi(len(p)) + p + tail + struct.pack(">QI", k, 0x3F) + b"\x04tokn"
            msgs.append(vi(len(body) + 1) + body)  # L = lw(|body|): one byte here
        wire = b"".join(msgs)
        frames.append((torch.from_numpy(np.frombuffer(wire, np.uint8).copy()).cuda(), 0, n))
    return frames


def write_frames(codec, n, rot, rng):
    """The frame of write_route_measure.py, from `rot` different draws."""
    import torch
    import netidx_amd
    from netidx_amd.codec import WriteCols
    n_ids = 100_000
    frames = []
    for _ in range(rot):
        ids = rng.integers(0, n_ids + n_ids // 20, n).astype(np.uint64)
        ids[rng.random(n) < 0.01] = np.uint64(2**40 + 5)
        wfl = (rng.random(n) < 0.5).astype(np.uint8)
        wid = rng.integers(0, 2**62, n).astype(np.uint64) >> rng.integers(0, 60, n).astype(np.uint64)
        n_un = n // 100
        ctl_row = np.sort(rng.integers(0, n + 1, n_un)).astype(np.uint64)
        uid = rng.integers(0, n_ids + 50, n_un).astype(np.uint64)
        msgs = [b"\x01" + vi(int(x)) for x in uid]
        msgs = [vi(len(m) + 1) + m for m in msgs]
        ctl_len = np.array([len(m) for m in msgs], np.uint32)
        ctl_off = (np.cumsum(ctl_len) - ctl_len).astype(np.uint64)
        heap = torch.from_numpy(np.frombuffer(b"".join(msgs), np.uint8).copy()).cuda()
        src = netidx_amd.columns_from_arrays(
            ids, rng.integers(0, 2**63, n).astype(np.uint64), np.full(n, 9, np.uint8),
            np.zeros(n, np.uint32), ctl_row=ctl_row, ctl_off=ctl_off, ctl_len=ctl_len,
            ctl_variant=np.ones(n_un, np.uint8))
        swc = WriteCols(n, "cuda")
        swc.wflags[:n].copy_(torch.from_numpy(wfl))
        swc.wid[:n].copy_(torch.from_numpy(wid.view(np.int64)))
        torch.cuda.synchronize()
        frames.append((codec.encode_writes(src, swc, heap).clone(), n, n_un))
    return frames


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rot", type=int, default=3)
    ap.add_argument("--frame", choices=["subscribes", "writes", "both"], default="both")
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--leg", choices=["fast", "general"], default="fast")
    a = ap.parse_args()
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns, WriteCols, LAYOUT_MIXED
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    for name in (["subscribes", "writes"] if a.frame == "both" else [a.frame]):
        rng = np.random.default_rng(0x5EED0013)
        frames = (subscribe_frames(a.n, a.rot, rng) if name == "subscribes"
                  else write_frames(codec, a.n, a.rot, rng))
        n_rows, n_ctl = frames[0][1], frames[0][2]
        # a set of columns per copy and leg
        outs = {leg: [(Columns(n_rows + 1, 1, n_ctl + 1, LAYOUT_MIXED, "cuda"),
                       WriteCols(n_rows + 1, "cuda")) for _ in frames]
                for leg in ("fast", "general")}
        torch.cuda.synchronize()

        def call(leg, k):
            cols, wc = outs[leg][k % a.rot]
            codec.decode_writes(frames[k % a.rot][0], cols, wc, fast=leg == "fast")
            return codec.writes_status.path

        if a.calls:
            for k in range(a.calls):
                call(a.leg, k)
            continue
        # fast against general, array for array, on every copy
        for k in range(a.rot):
            assert call("fast", k) == 8, "the fast decoder declined the frame"
            assert call("general", k) == 6
            (cf, wf), (cg, wg) = outs["fast"][k], outs["general"][k]
            assert (cf.s.n_rows, cf.s.n_children, cf.s.n_ctl) == (n_rows, 0, n_ctl)
            assert (cg.s.n_rows, cg.s.n_children, cg.s.n_ctl) == (n_rows, 0, n_ctl)
            kinds = {"rows": n_rows, "children": 0, "ctl": n_ctl}
            for field, _, kind in Columns.FIELDS:
                assert torch.equal(cf.t[field][: kinds[kind]], cg.t[field][: kinds[kind]]), field
            assert torch.equal(wf.wflags[:n_rows], wg.wflags[:n_rows])
            assert torch.equal(wf.wid[:n_rows], wg.wid[:n_rows])
        t = {"fast": [], "general": []}
        k = 0
        for _ in range(a.reps):
            for leg in ("general", "fast"):
                call(leg, k)  # untimed, the previous copy
                k += 1
                t0 = time.perf_counter()
                call(leg, k)
                t[leg].append(time.perf_counter() - t0)
        ms = {leg: statistics.median(v) * 1e3 for leg, v in t.items()}
        print(json.dumps({
            "frame": name, "messages": n_rows + n_ctl, "writes": n_rows, "control": n_ctl,
            "frame_bytes": int(frames[0][0].numel()), "rot": a.rot, "reps": a.reps,
            "general_ms": round(ms["general"], 3), "fast_ms": round(ms["fast"], 3),
            "general_ms_min": round(min(t["general"]) * 1e3, 3),
            "fast_ms_min": round(min(t["fast"]) * 1e3, 3),
            "general_over_fast": round(ms["general"] / ms["fast"], 1)}), flush=True)
        del frames, outs
    codec.close()


if __name__ == "__main__":
    main()
