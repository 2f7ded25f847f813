#!/usr/bin/env python3
"""Times nxg_decode_writes + nxg_route_writes (include/nxg_codec.h) on a GPU against a one-core
vectorised numpy fold of the same rules over the same columns on the host. Prints one JSON line.

The batch: --n To::Write messages (F64 values, half of them asking for a WriteResult) with one
To::Unsubscribe per 100 writes in between, ids over a table of --ids Ids (some past it), 16
channels, on_write lists of 0-3 channels and permissions with and without WRITE, so that every
outcome occurs. The frame is made by nxg_encode_writes.

Timed, each the median of --reps synchronous calls (wall clock around the call; a GPU call is
timed right after an untimed one of its kind, because the GPU idles through the host folds):
  decode          codec.decode_writes of the device frame
  route           codec.route_writes of the decoded columns (its output tensors allocated per call)
  decode_route    both
  host_fold       the numpy fold: outcomes, per-channel requests, reply bytes, wait list, unsub ids
  host_copy_fold  the same after copying the decoded columns it reads to the host
Before anything is timed the fold's outputs are compared with the GPU's, all of them."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MSG = [b"cannot write to unsubscribed value", b"write permission denied", b"writes not accepted"]
NOT_SUB, NO_SLOT = 0xFFFFFFFF, 0xFFFFFFFF


def vi(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def vl(x):
    """varint_len of a u64 array (pack.rs:472-474)."""
    n = np.ones(len(x), np.int64)
    for k in range(1, 10):
        n += x >= np.uint64(1 << (7 * k))
    return n


def put_varints(out, pos, x, n):
    """The varints of x (lengths n) into out at pos."""
    x = x.copy()
    for j in range(10):
        sel = n > j
        if not sel.any():
            break
        last = n[sel] == j + 1
        out[pos[sel] + j] = (x[sel] & np.uint64(0x7F)).astype(np.uint8) | np.where(last, 0, 0x80).astype(np.uint8)
        x >>= np.uint64(7)


def host_fold(tab, n_chans, ids, wflags, wid, ctl_row, uid):
    """handle_batch_inner's Write / Unsubscribe arms (publisher/server.rs:171-245, 497-576) over
    columns, vectorised. No Subscribe spans, no NO_WID rows (the encoder writes every WriteId)."""
    perm_of, slot_of, off, chan = tab
    n, n_ids = len(ids), len(perm_of)
    ctl_row = ctl_row.astype(np.int64)
    rows = np.arange(n, dtype=np.int64)
    first = np.full(n_ids, np.iinfo(np.int64).max, np.int64)
    inr = uid < n_ids
    np.minimum.at(first, uid[inr].astype(np.int64), ctl_row[inr].astype(np.int64))
    known = ids < n_ids
    idc = np.where(known, ids, 0).astype(np.int64)
    perm = np.where(known, perm_of[idc], NOT_SUB)
    unsub = (perm == NOT_SUB) | (known & (first[idc] <= rows))
    slot = slot_of[idc].astype(np.int64)
    sc = np.where(slot == NO_SLOT, 0, slot)
    cnt = np.where(slot == NO_SLOT, 0, off[sc + 1].astype(np.int64) - off[sc])
    outcome = np.where(unsub, 1, np.where((perm & 4) == 0, 2, np.where(cnt == 0, 3, 0))).astype(np.uint8)
    r = (wflags & 1) != 0
    routed = outcome == 0
    w = routed & r
    wait = (rows[w], ids[w], wid[w])
    # per-channel requests: (row, channel) pairs in row order, then a stable sort by channel
    rr = rows[routed]
    k = cnt[routed]
    pr = np.repeat(rr, k)
    start = np.repeat(off[sc[routed]].astype(np.int64), k)
    within = np.arange(len(pr)) - np.repeat(np.cumsum(k) - k, k)
    pc = chan[start + within].astype(np.int64)
    order = np.argsort(pc, kind="stable")
    chan_off = np.concatenate([[0], np.cumsum(np.bincount(pc, minlength=n_chans))])
    ent_row = pr[order]
    ent_id = ids[ent_row]
    # replies: sizes, places in message order, bytes
    rep = ~routed & r
    ri, rw, ro = ids[rep], wid[rep], outcome[rep].astype(np.int64) - 1
    li, lw = vl(ri), vl(rw)
    ml = np.array([len(m) for m in MSG], np.int64)[ro]
    rsize = 1 + 1 + li + 2 + ml + lw
    ul = vl(uid)
    usize = 2 + ul
    rrow = rows[rep]
    rpre = np.concatenate([[0], np.cumsum(rsize)])
    upre = np.concatenate([[0], np.cumsum(usize)])
    rpos = rpre[:-1] + upre[np.searchsorted(ctl_row, rrow, side="right")]
    upos = upre[:-1] + rpre[np.searchsorted(rrow, ctl_row, side="left")]
    out = np.zeros(rpre[-1] + upre[-1], np.uint8)
    out[upos] = usize  # L = |body| + 1: the message's whole length
    out[upos + 1] = 2
    put_varints(out, upos + 2, uid, ul)
    out[rpos] = rsize
    out[rpos + 1] = 6
    put_varints(out, rpos + 2, ri, li)
    p = rpos + 2 + li
    out[p] = 0x12
    out[p + 1] = ml
    mat = np.zeros((3, 34), np.uint8)
    for i, m in enumerate(MSG):
        mat[i, : len(m)] = np.frombuffer(m, np.uint8)
    for j in range(34):
        sel = ml > j
        out[p[sel] + 2 + j] = mat[ro[sel], j]
    put_varints(out, p + 2 + ml, rw, lw)
    return outcome, chan_off, ent_id, ent_row, wait, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--ids", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns, WriteCols, WriteTable, LAYOUT_MIXED
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    rng = np.random.default_rng(0x5EED0011)
    n, n_ids, n_chans = a.n, a.ids, 16
    ids = rng.integers(0, n_ids + n_ids // 20, n).astype(np.uint64)
    ids[rng.random(n) < 0.01] = np.uint64(2**40 + 5)
    wfl = (rng.random(n) < 0.5).astype(np.uint8)
    wid = rng.integers(0, 2**62, n).astype(np.uint64) >> rng.integers(0, 60, n).astype(np.uint64)
    n_un = n // 100
    ctl_row = np.sort(rng.integers(0, n + 1, n_un)).astype(np.uint64)
    uid = rng.integers(0, n_ids + 50, n_un).astype(np.uint64)
    msgs = [b"\x01" + vi(int(x)) for x in uid]
    msgs = [vi(len(m) + 1) + m for m in msgs]  # L = lw(|variant + fields|): one byte here
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
    frame = codec.encode_writes(src, swc, heap)
    # the client's state: nine Ids in ten subscribed, a fifth without WRITE, on_write lists of 0-3
    perm = rng.choice(np.array([4, 5, 7, 1, NOT_SUB], np.uint32), n_ids, p=[.3, .2, .2, .2, .1])
    has = rng.random(n_ids) < 0.8
    k = np.where(has, rng.integers(0, 4, n_ids), 0)
    slot_of = np.where(has, np.cumsum(has) - 1, NO_SLOT).astype(np.uint32)
    off = np.concatenate([[0], np.cumsum(k[has])]).astype(np.uint32)
    chan = ((np.arange(off[-1]) * 7 + np.repeat(np.arange(int(has.sum())), k[has])) % n_chans).astype(np.uint32)
    table = WriteTable(perm, slot_of, off, chan, n_chans)
    W = frame.numel()
    cols = Columns(n + 1, 1, n_un + 1, LAYOUT_MIXED, "cuda")
    wcols = WriteCols(n + 1, "cuda")

    def decode():
        codec.decode_writes(frame, cols, wcols)

    def route():
        return codec.route_writes(table, frame, cols, wcols)

    def copy_back():
        return (cols.id[:n].cpu().numpy().view(np.uint64), wcols.wflags[:n].cpu().numpy(),
                wcols.wid[:n].cpu().numpy().view(np.uint64),
                cols.ctl_row[:n_un].cpu().numpy().view(np.uint64))

    def fold(c):
        # (the Unsubscribe Ids: the host has them from its own parse of the spans)
        return host_fold((perm, slot_of, off, chan), n_chans, c[0], c[1], c[2], c[3], uid)

    decode()
    assert (cols.s.n_rows, cols.s.n_ctl) == (n, n_un)
    r = route()
    host = copy_back()
    outcome, chan_off, ent_id, ent_row, wait, reply = fold(host)
    h = r.numpy()
    assert np.array_equal(h["outcome"], outcome)
    assert h["reply"] == reply.tobytes()
    assert h["unsub_id"] == uid.tolist()
    assert h["wait"] == list(zip(*(x.tolist() for x in wait)))
    assert np.array_equal(r.chan_off.cpu().numpy(), chan_off)
    assert np.array_equal(r.ent_id[: r.n_entries].cpu().numpy().view(np.uint64), ent_id)
    assert np.array_equal(r.ent_row[: r.n_entries].cpu().numpy(), ent_row)
    fns = {"decode": decode, "route": route, "decode_route": lambda: (decode(), route()),
           "host_fold": lambda: fold(host), "host_copy_fold": lambda: fold(copy_back())}
    for f in fns.values():
        f()
    t = {name: [] for name in fns}
    for _ in range(a.reps):
        for name, f in fns.items():
            if not name.startswith("host"):
                f()  # (the GPU has idled through the host fold: one untimed call first)
            t0 = time.perf_counter()
            f()
            t[name].append(time.perf_counter() - t0)
    ms = {name: round(statistics.median(v) * 1e3, 3) for name, v in t.items()}
    print(json.dumps({"writes": n, "unsubscribes": n_un, "n_ids": n_ids, "channels": n_chans,
                      "frame_bytes": W, "outcomes": r.n_outcome, "entries": r.n_entries,
                      "replies": r.n_replies, "reply_bytes": r.reply_len, "wait": r.n_wait,
                      "reps": a.reps, "ms": ms,
                      "host_fold_over_decode_route": round(ms["host_fold"] / ms["decode_route"], 1)}),
          flush=True)
    codec.close()


if __name__ == "__main__":
    main()
