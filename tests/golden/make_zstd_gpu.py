#!/usr/bin/env python3
"""The golden pin of the GPU zstd compressor (nxg_archive_compress, netidx_amd/csrc/nxg_zstd_enc.hip).

Run once on the MI355X. Compresses a subset of the zstd fixtures (tests/golden/make_zstd.py) and
the crafted payloads of tests/zstd_enc_cases.py on the GPU and writes

  zstd_gpu_records.bin    the compressed records (u32 BE length | index | zstd frame), back to back
  zstd_gpu_plain.bin      the crafted payloads' plain bytes (the fixtures' are in zstd_plain.bin)
  zstd_gpu_manifest.json  per record: name, dict, indexed, index (hex), where its plain bytes are
                          (plain_src "fixture" or "own", plain_off, plain_len), rec_off, rec_len

tests/test_gpu_zstd_compress.py asserts that the compressor still produces exactly these bytes;
tests/test_zstd_gpu_golden_cpu.py asserts, without a GPU, that libzstd decompresses every committed
frame to its plain bytes. The compressor's bytes are its own: ANY later change to the encoder (the
matcher, the tables' sizes, the literals or sequences coding) changes them, and these files must
then be regenerated with this script and committed with the change.

Usage: python tests/golden/make_zstd_gpu.py [--out DIR]   (DIR defaults to tests/golden)
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import zstd_enc_cases as zc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    import netidx_amd
    ents, rec, plain, d = zc.load_fixtures()
    crafted = zc.crafted(d)

    def first(pred):
        return [e for e in ents if pred(e)][0]

    picks = [
        ("empty", first(lambda e: e["kind"] == "empty")),
        ("tiny", first(lambda e: e["dict"] and not e["indexed"] and 0 < e["plain_len"] < 16)),
        ("indexed", first(lambda e: e["dict"] and e["indexed"] and e["plain_len"] > 2000)),
        ("two_blocks", first(lambda e: e["kind"] == "multiblock_dict")),
        ("no_dict", first(lambda e: e["kind"] == "nodict_l1")),
    ]
    items = []  # (name, dict, indexed, index, plain_src, plain_off, batch)
    for name, e in picks:
        idx, b = zc.fixture_record(e, rec, plain)
        items.append((name, e["dict"], e["indexed"], idx, "fixture", e["plain_off"], b))
    own = b""
    for name in ("huf1", "huf4", "dict_slice", "pattern64", "one_byte"):
        items.append((name, True, False, b"", "own", len(own), crafted[name]))
        own += crafted[name]

    codec = netidx_amd.Codec(0)
    zd = codec.zstd_dict(d)
    blob, man = b"", []
    for name, use_dict, indexed, idx, psrc, poff, b in items:
        src = np.frombuffer(idx + b + b"\0", np.uint8)
        out, res = codec.archive_compress(src, [(0, len(idx) + len(b))], indexed,
                                          zd if use_dict else None)
        oo, ol, er = res[0]
        assert er == 0, name
        cr = bytes(out[oo:oo + ol])
        man.append({"name": name, "dict": use_dict, "indexed": indexed, "index": idx.hex(),
                    "plain_src": psrc, "plain_off": poff, "plain_len": len(b),
                    "rec_off": len(blob), "rec_len": len(cr)})
        blob += cr
        print(name, len(b), "->", len(cr))
    zd.close()
    codec.close()
    assert len(blob) + len(own) <= 512 * 1024
    os.makedirs(a.out, exist_ok=True)
    open(os.path.join(a.out, "zstd_gpu_records.bin"), "wb").write(blob)
    open(os.path.join(a.out, "zstd_gpu_plain.bin"), "wb").write(own)
    json.dump({"records": man}, open(os.path.join(a.out, "zstd_gpu_manifest.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
