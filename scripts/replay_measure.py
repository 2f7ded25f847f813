#!/usr/bin/env python3
"""Times nxg_replay_window and nxg_replay_image (include/nxg_codec.h) on a GPU against what they
replace. Prints one JSON line per window.

Windows: those of scripts/archive_window_measure.py (fixtures x 10,000 records; synthetic: one
10^5-item record, then 10,000 records of 1-64 items), decoded by nxg_archive_decode_window. The
table publishes every archive Id but one in sixteen, which has no path (dropped); nothing misses.
Comparisons, each the median of --reps runs after a warm-up, the variants taken in turn inside
every repetition:
  replay_gpu            the host clock around the synchronous call (structs built beforehand)
  host_model            the vectorised host model (numpy: the table gather, the mask, the
                        Unsubscribed rewrite, four masked gathers, the per-record counts) over
                        columns that already lie in host memory
  host_copy_and_model   the same after copying the window's id / tag / fixed / aux to the host
  image_*               likewise nxg_replay_image over the window's image, `order` a permutation
                        of every Id
The device rows are compared with the host model's before anything is timed. --calls-only runs the
calls alone on the synthetic window (for a kernel trace in a run of its own)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import archive_window_measure as awm  # noqa: E402  (the windows and the timing loop)

DROP = np.uint64(0xFFFFFFFFFFFFFFFF)
UNSUB, NULL = 0x40, 16


def host_window(ids, tag, fixed, aux, table, row_off, n_rows):
    p = table[ids]
    kept = p != DROP
    src = np.flatnonzero(kept)
    t = tag[src]
    un = t == UNSUB
    rows = (p[src], np.where(un, NULL, t), np.where(un, 0, fixed[src]), np.where(un, 0, aux[src]),
            src)
    before = np.concatenate([[0], np.cumsum(kept)])
    rec_off = np.concatenate([before[row_off], before[row_off[-1:] + n_rows[-1:]]])
    return rows, rec_off


def host_image(img, order, table):
    p = table[order]
    kept = p != DROP
    a = order[kept]
    k = np.minimum(np.searchsorted(img["id"], a), len(img["id"]) - 1)
    have = (img["id"][k] == a) & (img["tag"][k] != UNSUB)
    return (p[kept], np.where(have, img["tag"][k], NULL), np.where(have, img["fixed"][k], 0),
            np.where(have, img["aux"][k], 0), np.where(have, k, -1))


def measure(codec, name, records, reps, calls_only=False):
    import torch
    import netidx_amd
    from netidx_amd.codec import (Columns, NetidxError, NxgArchiveBatchInfo, NxgReplayTable,
                                  ReplayRows, lib)
    offs, off = [], 0
    for r in records:
        offs.append((off, len(r)))
        off += len(r)
    buf = np.frombuffer(b"".join(records), np.uint8)
    dbuf = torch.from_numpy(buf.copy()).cuda()
    cols = Columns(len(buf) // 2 + 1, len(buf) + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    infos = codec.archive_decode_window(dbuf, offs, cols, 0)
    n, n_recs = int(cols.s.n_rows), len(infos)
    dev_cols = [x[:n] for x in (cols.id, cols.tag, cols.fixed, cols.aux)]
    ids, tag, fixed, aux = (x.cpu().numpy() for x in dev_cols)
    n_ids = int(ids.max()) + 1
    table = (np.arange(n_ids, dtype=np.uint64) * np.uint64(3) + np.uint64(1))
    table[::16] = DROP
    dtable = torch.from_numpy(table.view(np.int64)).cuda()
    row_off = np.array([f.row_off for f in infos], np.int64)
    n_rows = np.array([f.n_rows for f in infos], np.int64)
    info = (NxgArchiveBatchInfo * n_recs)(*infos)
    rows = ReplayRows(n, n_recs, 64, "cuda")
    tab = NxgReplayTable(n_ids, dtable.data_ptr())
    L, err = lib(), NetidxError()

    def gpu():
        assert L.nxg_replay_window(codec.ctx, C.byref(cols.s), info, n_recs, C.byref(tab),
                                   C.byref(rows.s), C.byref(err))

    img = codec.archive_build_image(cols, n_ids)
    order = np.random.default_rng(5).permutation(n_ids).astype(np.uint32)
    dorder = torch.from_numpy(order.view(np.int32)).cuda()
    irows = ReplayRows(n_ids, 1, 64, "cuda")

    def gpu_image():
        assert L.nxg_replay_image(codec.ctx, C.byref(img.s), C.c_void_p(dorder.data_ptr()), n_ids,
                                  C.byref(tab), C.byref(irows.s), C.byref(err))

    if calls_only:
        for _ in range(reps + 1):
            gpu()
            gpu_image()
        return None
    # the same rows either way
    gpu()
    want, want_off = host_window(ids.view(np.int64), tag, fixed, aux, table, row_off, n_rows)
    rows._off = None
    got = rows.numpy()
    for k, w in zip(("id", "tag", "fixed", "aux", "src_row"), want):
        assert np.array_equal(got[k], w.astype(got[k].dtype)), k
    assert np.array_equal(rows.offsets(), want_off.astype(np.uint64))
    assert rows.n_done == n_recs and rows.n_dropped == n - rows.n_rows
    gpu_image()
    image = img.numpy()
    wi = host_image(image, order.astype(np.uint64), table)
    gi = irows.numpy()
    for k, w in zip(("id", "tag", "fixed", "aux", "src_row"), wi):
        assert np.array_equal(gi[k], w.astype(gi[k].dtype)), k
    idev = [getattr(img, k)[:img.n_rows] for k in ("id", "tag", "fixed", "aux")]

    def host_copy_and_model():
        i, t, f, a = (x.cpu().numpy() for x in dev_cols)
        host_window(i.view(np.int64), t, f, a, table, row_off, n_rows)

    def image_copy_and_model():
        i, t, f, a = (x.cpu().numpy() for x in idev)
        host_image({"id": i.view(np.uint64), "tag": t, "fixed": f, "aux": a},
                   order.astype(np.uint64), table)

    t = awm.timed({
        "replay_gpu": gpu,
        "host_model": lambda: host_window(ids.view(np.int64), tag, fixed, aux, table, row_off,
                                          n_rows),
        "host_copy_and_model": host_copy_and_model,
        "image_gpu": gpu_image,
        "image_host_model": lambda: host_image(image, order.astype(np.uint64), table),
        "image_host_copy_and_model": image_copy_and_model}, reps)
    out = {"window": name, "records": n_recs, "rows": n, "kept": int(rows.n_rows), "n_ids": n_ids,
           "image_rows": int(img.n_rows), "image_kept": int(irows.n_rows), "reps": reps,
           "ms": {k: round(v * 1e3, 3) for k, v in t.items()}}
    out["host_copy_and_model_over_gpu"] = round(t["host_copy_and_model"] / t["replay_gpu"], 2)
    out["gpu_bytes"] = 29 * n + 29 * int(rows.n_rows)  # 21 + the table gather; 29 per kept row
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--records", type=int, default=10_000)
    ap.add_argument("--image-items", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls-only", action="store_true")
    a = ap.parse_args()
    import torch
    import netidx_amd
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    recs, _ = awm.synthetic_window(a.image_items, a.records, 0x5EED0007)
    if not a.calls_only:
        measure(codec, "fixtures", awm.fixture_window(codec, a.records), a.reps)
    measure(codec, "synthetic", recs, a.reps, a.calls_only)
    codec.close()


if __name__ == "__main__":
    main()
