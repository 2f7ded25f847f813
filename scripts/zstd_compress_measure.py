#!/usr/bin/env python3
"""Ratio and throughput of the GPU zstd compressor (nxg_archive_compress_opts), for DESIGN.md 4.8.1.

Ratio: the 37 dictionary batch fixtures of tests/golden/zstd_manifest.json compressed on the GPU,
their frames' total against libzstd's level-19 total recorded in the manifest and, where libzstd
loads, against libzstd level 1 with the same dictionary. --literals chooses the literals mode
(0: the dictionary's tree only, 1: block trees); the same fixtures are also compressed with a
raw-content dictionary and with none, and by libzstd without the dictionary.

Throughput: one call over --records records cut from those fixtures, cycling --buffers distinct
source buffers so that no call finds its source in the 256 MiB cache; the compressor kernel's time
(events around the kernel) and the whole call's wall time are reported separately, then one core
of libzstd at levels 1 and 19 over the same fixtures (or that libzstd did not load).

Usage: python scripts/zstd_compress_measure.py [--literals 0|1] [--records 10000] [--buffers 3]
       [--json FILE]
With NXG_LIB naming a library built from an older source, --literals 0 goes through
nxg_archive_compress, which every build has.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import zstd_enc_cases as zc  # noqa: E402


def libzstd_compressor(d):
    try:
        z = C.CDLL("libzstd.so.1")
    except OSError:
        return None
    z.ZSTD_createCCtx.restype = C.c_void_p
    z.ZSTD_compress_usingDict.restype = C.c_size_t
    z.ZSTD_compress_usingDict.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                          C.c_size_t, C.c_char_p, C.c_size_t, C.c_int]
    z.ZSTD_createCDict.restype = C.c_void_p
    z.ZSTD_createCDict.argtypes = [C.c_char_p, C.c_size_t, C.c_int]
    z.ZSTD_compress_usingCDict.restype = C.c_size_t
    z.ZSTD_compress_usingCDict.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                           C.c_size_t, C.c_void_p]
    z.ZSTD_isError.argtypes = [C.c_size_t]
    cctx = z.ZSTD_createCCtx()
    cdicts = {}

    def run(payloads, level, use_dict=True):
        """(total compressed bytes, seconds) on this core, the dictionary prepared once"""
        if not use_dict:
            z.ZSTD_compressCCtx.restype = C.c_size_t
            z.ZSTD_compressCCtx.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p,
                                            C.c_size_t, C.c_int]
            out = C.create_string_buffer(max(len(p) for p in payloads) * 2 + 1024)
            total = 0
            t0 = time.perf_counter()
            for p in payloads:
                r = z.ZSTD_compressCCtx(cctx, out, len(out), p, len(p), level)
                assert not z.ZSTD_isError(r)
                total += r
            return total, time.perf_counter() - t0
        if level not in cdicts:
            cdicts[level] = z.ZSTD_createCDict(d, len(d), level)
        out = C.create_string_buffer(max(len(p) for p in payloads) * 2 + 1024)
        total = 0
        t0 = time.perf_counter()
        for p in payloads:
            r = z.ZSTD_compress_usingCDict(cctx, out, len(out), p, len(p), cdicts[level])
            assert not z.ZSTD_isError(r)
            total += r
        return total, time.perf_counter() - t0

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=10000)
    ap.add_argument("--buffers", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--literals", type=int, default=0, choices=(0, 1))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import netidx_amd
    from netidx_amd.codec import lib
    ents, rec, plain, d = zc.load_fixtures()
    es = [e for e in ents if e["dict"] and e["batch"]]
    pay = [plain[e["plain_off"]:e["plain_off"] + e["plain_len"]] for e in es]
    res = {"literals": a.literals, "fixtures": len(es), "plain_bytes": sum(map(len, pay)),
           "libzstd_l19_manifest_bytes": sum(e["frame_len"] for e in es)}
    codec = netidx_amd.Codec(0)
    zd = codec.zstd_dict(d)

    def gpu(payloads):
        offs, o = [], 0
        for p in payloads:
            offs.append((o, len(p)))
            o += len(p)
        src = np.frombuffer(b"".join(payloads) + b"\0", np.uint8)
        return src, offs

    src, offs = gpu(pay)
    has_opts = hasattr(lib(), "nxg_archive_compress_opts")
    assert has_opts or a.literals == 0, "this library has no nxg_archive_compress_opts"

    def frames_bytes(zdict):
        if has_opts:
            out, r = codec.archive_compress(src, offs, False, zdict, a.literals)
        else:  # an older library: nxg_archive_compress itself
            from netidx_amd.codec import NxgArchiveRecord, NetidxError
            recs = (NxgArchiveRecord * len(offs))()
            for i, (off, ln) in enumerate(offs):
                recs[i].off, recs[i].len = off, ln
            need, err = C.c_uint64(0), NetidxError()
            dh = zdict.h if zdict else None
            g0 = lib().nxg_archive_compress
            assert g0(codec.ctx, dh, C.c_void_p(src.ctypes.data), len(src), recs, len(offs), False,
                      None, 0, C.byref(need), C.byref(err))
            out = np.zeros(need.value, np.uint8)
            assert g0(codec.ctx, dh, C.c_void_p(src.ctypes.data), len(src), recs, len(offs), False,
                      C.c_void_p(out.ctypes.data), need.value, C.byref(need), C.byref(err))
            r = [(x.out_off, x.out_len, x.err) for x in recs]
        assert all(x[2] == 0 for x in r)
        return sum(x[1] - 4 for x in r)

    res["gpu_frame_bytes"] = frames_bytes(zd)
    res["gpu_frame_bytes_no_dict"] = frames_bytes(None)
    raw = codec.zstd_dict(zc.dict_parts(d)[2])
    res["gpu_frame_bytes_raw_content_dict"] = frames_bytes(raw)
    raw.close()
    zrun = libzstd_compressor(d)
    if zrun:
        res["libzstd_l1_bytes"], _ = zrun(pay, 1)
        res["libzstd_l19_bytes"], _ = zrun(pay, 19)
        res["libzstd_l1_no_dict_bytes"], _ = zrun(pay, 1, False)
        res["libzstd_l19_no_dict_bytes"], _ = zrun(pay, 19, False)
    else:
        res["libzstd"] = "did not load"
    # ---- throughput
    bufs = []
    for k in range(a.buffers):
        ps = [pay[(i + 7 * k) % len(pay)] for i in range(a.records)]
        bufs.append(gpu(ps))
    nbytes = sum(ln for _, ln in bufs[0][1])
    res["call_records"] = a.records
    res["call_plain_bytes"] = nbytes
    res["source_bytes_cycled"] = sum(len(s) for s, _ in bufs)
    kms = lib().nxg_debug_zstd_compress_kernel_ms
    kms.restype = C.c_double
    kms.argtypes = [C.c_void_p]
    from netidx_amd.codec import NxgArchiveRecord, NetidxError
    if has_opts:
        from netidx_amd.codec import NxgZstdCompressOpts
        opts = NxgZstdCompressOpts(literals=a.literals)
        g = lib().nxg_archive_compress_opts

        def f(ctx, dh, sp, sl, recs, n, indexed, out, cap, need, err):
            return g(ctx, dh, sp, sl, recs, n, indexed, C.byref(opts), out, cap, need, err)
    else:
        f = lib().nxg_archive_compress
    prepared = []
    for s, o in bufs:  # the C call itself is timed: descriptors and the output buffer are ready
        recs = (NxgArchiveRecord * len(o))()
        for i, (off, ln) in enumerate(o):
            recs[i].off, recs[i].len = off, ln
        prepared.append((s, recs, len(o)))
    need, err = C.c_uint64(0), NetidxError()
    cap = 0
    for s, recs, n in prepared:
        assert f(codec.ctx, zd.h, C.c_void_p(s.ctypes.data), len(s), recs, n, False, None, 0,
                 C.byref(need), C.byref(err))
        cap = max(cap, need.value)
    outbuf = np.zeros(cap, np.uint8)
    calls = []
    for i in range(a.reps + 1):
        s, recs, n = prepared[i % len(prepared)]
        t0 = time.perf_counter()
        ok = f(codec.ctx, zd.h, C.c_void_p(s.ctypes.data), len(s), recs, n, False,
               C.c_void_p(outbuf.ctypes.data), len(outbuf), C.byref(need), C.byref(err))
        wall = time.perf_counter() - t0
        assert ok, err.msg
        if i:  # the first call allocates
            calls.append((kms(codec.ctx), wall * 1e3, sum(recs[j].out_len for j in range(n))))
        print("call", i, "kernel %.2f ms, whole call %.2f ms" % (kms(codec.ctx), wall * 1e3),
              flush=True)
    calls.sort()
    k, w, ob = calls[len(calls) // 2]
    res["kernel_ms_median"] = k
    res["call_ms_of_that_call"] = w
    res["call_ms_median"] = sorted(c[1] for c in calls)[len(calls) // 2]
    res["kernel_GBps"] = nbytes / k / 1e6
    res["call_GBps"] = nbytes / res["call_ms_median"] / 1e6
    res["call_compressed_bytes"] = ob
    res["note"] = ("the whole call (the C entry point) includes the index parse, the copy to the "
                   "device, the packed copy back and the host's scatter into the slots")
    if zrun:
        for level in (1, 19):
            reps = 20 if level == 1 else 2
            t = min(zrun(pay, level)[1] for _ in range(reps))
            res["libzstd_l%d_one_core_MBps" % level] = res["plain_bytes"] / t / 1e6
    zd.close()
    codec.close()
    print(json.dumps(res, indent=1))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
