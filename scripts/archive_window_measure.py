#!/usr/bin/env python3
"""Times nxg_archive_decode_window and nxg_archive_build_image (include/nxg_codec.h) on a GPU
against what they replace. Prints one JSON line per window.

Windows:
  fixtures   the batch + dict records of tests/golden/zstd_manifest.json, decompressed by
             nxg_archive_decompress and repeated to 10,000 records
  synthetic  synth.archive_columns: one 10^5-item record (the image record), then 10,000 records
             of 1-64 items (the deltas)
Comparisons, each the median of --reps synchronous calls after a warm-up, the variants taken in
turn inside every repetition:
  loop       nxg_decode_archive_batch once per record (the only way before the window call)
  window     the window call with the default big_record_bytes, with 1 (every record through the
             single-batch decoder), with UINT64_MAX (every record through the wave kernels) and
             with the values of --sweep in between: what picks the default
  image      nxg_archive_build_image against a one-core host fold of the same rows (numpy: the
             last row per Id by an ordered scatter, then a gather), with and without the copy of
             the rows to the host
The rows of the loop and of the window call are compared before anything is timed."""
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
GOLD = os.path.join(ROOT, "tests", "golden")
U64_MAX = 2**64 - 1


def vi(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def encode_rows(m, a, b):
    """Rows [a, b) of synth.archive_columns as an archive batch (the tags of that mix: I64 6, F64
    9, DateTime 10, String 12, Array 19 of I64 / F64, Unsubscribed 0x40)."""
    out = [vi(b - a)]
    heap = m.heap
    for r in range(a, b):
        t, f, x = int(m.tag[r]), int(m.fixed[r]), int(m.aux[r])
        out.append(vi(int(m.id[r])))
        if t == 0x40:
            out.append(b"\x40")
        elif t in (6, 9):
            out.append(bytes([t]) + struct.pack(">Q", f))
        elif t == 10:
            out.append(b"\x0a" + struct.pack(">QI", f, x))
        elif t == 12:
            out.append(b"\x0c" + vi(x) + heap[f:f + x].tobytes())
        elif t == 19:
            out.append(b"\x13" + vi(x) + b"".join(
                bytes([int(m.ctag[j])]) + struct.pack(">Q", int(m.cfixed[j])) for j in range(f, f + x)))
        else:
            raise ValueError(t)
    return b"".join(out)


def synthetic_window(n_image, n_deltas, seed):
    from netidx_amd import synth
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 65, n_deltas)
    total = n_image + int(sizes.sum())
    m = synth.archive_columns(total, seed=seed)
    records, a = [encode_rows(m, 0, n_image)], n_image
    for s in sizes.tolist():
        records.append(encode_rows(m, a, a + s))
        a += s
    return records, total  # Ids are a permutation of 0 .. total - 1


def fixture_window(codec, n_records):
    ents = json.load(open(os.path.join(GOLD, "zstd_manifest.json")))["records"]
    rec = np.frombuffer(open(os.path.join(GOLD, "zstd_records.bin"), "rb").read(), np.uint8)
    zd = codec.zstd_dict(open(os.path.join(GOLD, "zstd_dict.bin"), "rb").read())
    records = []
    for indexed in (False, True):
        es = [e for e in ents if e["batch"] and e["dict"] and e["indexed"] == indexed]
        out, res = codec.archive_decompress(rec, [(e["rec_off"], e["rec_len"]) for e in es],
                                            indexed, zd)
        host = out.cpu().numpy()
        records += [host[o:o + n].tobytes() for o, n, er in res if er == 0]
    return [records[i % len(records)] for i in range(n_records)]


def timed(fns, reps):
    """Median seconds of each of `fns` (name -> callable ending in a device synchronise), the
    callables taken in turn inside every repetition."""
    for f in fns.values():
        f()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            t0 = time.perf_counter()
            f()
            t[k].append(time.perf_counter() - t0)
    return {k: statistics.median(v) for k, v in t.items()}


def measure(codec, name, records, n_ids, reps, sweep=()):
    import torch
    import netidx_amd
    from netidx_amd.codec import Columns, NxgStatus, NetidxError, lib
    offs, off = [], 0
    for r in records:
        offs.append((off, len(r)))
        off += len(r)
    buf = np.frombuffer(b"".join(records), np.uint8)
    dbuf = torch.from_numpy(buf.copy()).cuda()
    total = len(buf)
    cols = Columns(total // 2 + 1, total + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    longest = max(n for _, n in offs)
    one = Columns(longest // 2 + 1, longest + 1, 1, netidx_amd.LAYOUT_MIXED, "cuda")
    L, base = lib(), dbuf.data_ptr()
    st, err, used = NxgStatus(), NetidxError(), C.c_uint64(0)

    def loop(collect=None):
        for o, n in offs:
            ok = L.nxg_decode_archive_batch(codec.ctx, C.c_void_p(base + o), n, C.byref(one.s),
                                            C.byref(st), C.byref(used), C.byref(err))
            assert ok and st.err_kind == 0
            if collect is not None:
                g = one.numpy()
                collect.append((g["id"], g["tag"]))

    def window(big):
        return codec.archive_decode_window(dbuf, offs, cols, big)

    # the same rows either way
    parts = []
    loop(parts)
    infos = window(0)
    g = cols.numpy()
    assert np.array_equal(g["id"], np.concatenate([p[0] for p in parts]))
    assert np.array_equal(g["tag"], np.concatenate([p[1] for p in parts]))
    n_rows = cols.s.n_rows
    if n_ids is None:  # the reader's max_id + 1 (reader.rs:226-237)
        n_ids = int(g["id"].max()) + 1
    by_wave = sum(1 for f in infos if f.path == 7)
    fns = {"loop": loop, "window_default": lambda: window(0), "window_decoder": lambda: window(1),
           "window_wave": lambda: window(U64_MAX)}
    for big in sweep:  # big_record_bytes between the two forced routes
        fns["window_big_%d" % big] = lambda big=big: window(big)
    t = timed(fns, reps)
    window(0)
    ids_dev = cols.id[:n_rows]
    tag_h, fix_h, aux_h = (x[:n_rows].cpu().numpy() for x in (cols.tag, cols.fixed, cols.aux))

    def host_fold(ids):
        last = np.zeros(n_ids, np.int64)
        last[ids] = np.arange(1, len(ids) + 1)  # an ordered scatter: the last row of an Id stays
        win = np.flatnonzero(last)
        src = last[win] - 1
        return win, tag_h[src], fix_h[src], aux_h[src]

    ids_h = ids_dev.cpu().numpy()
    img = codec.archive_build_image(cols, n_ids)
    win, *_ = host_fold(ids_h)
    assert np.array_equal(img.numpy()["id"], win.astype(np.uint64))
    ti = timed({"image_gpu": lambda: codec.archive_build_image(cols, n_ids),
                "image_host_fold": lambda: host_fold(ids_h),
                "image_host_copy_and_fold": lambda: host_fold(ids_dev.cpu().numpy())}, reps)
    out = {"window": name, "records": len(records), "bytes": total, "rows": int(n_rows),
           "records_by_wave_default": by_wave, "n_ids": n_ids, "image_rows": int(img.n_rows),
           "reps": reps, "ms": {k: round(v * 1e3, 3) for k, v in {**t, **ti}.items()}}
    out["loop_over_window_default"] = round(t["loop"] / t["window_default"], 2)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--records", type=int, default=10_000)
    ap.add_argument("--image-items", type=int, default=100_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sweep", default="2048,8192,32768,131072,524288",
                    help="big_record_bytes values timed on the two whole windows")
    a = ap.parse_args()
    import torch
    import netidx_amd
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    codec = netidx_amd.Codec(0)
    fx = fixture_window(codec, a.records)
    sweep = [int(x) for x in a.sweep.split(",") if x]
    measure(codec, "fixtures", fx, None, a.reps, sweep)
    recs, n_ids = synthetic_window(a.image_items, a.records, 0x5EED0007)
    measure(codec, "synthetic", recs, n_ids, a.reps, sweep)
    # the deltas alone: what picks the default big_record_bytes between the two routes
    measure(codec, "synthetic_deltas", recs[1:], n_ids, a.reps)
    measure(codec, "synthetic_image_record", recs[:1], n_ids, a.reps)
    codec.close()


if __name__ == "__main__":
    main()
