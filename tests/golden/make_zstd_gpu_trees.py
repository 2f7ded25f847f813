#!/usr/bin/env python3
"""The golden pin of the GPU zstd compressor with block trees (nxg_archive_compress_opts, literals
= 1; netidx_amd/csrc/nxg_zstd_enc.hip).

Run once on the MI355X. Compresses a handful of the records of tests/zstd_tree_cases.py and two
fixture records (tests/golden/make_zstd.py) on the GPU and writes

  zstd_gpu_tree_records.bin     the compressed records (u32 BE length | index | zstd frame)
  zstd_gpu_tree_manifest.json   per record: name, dict, indexed, index (hex), source (a name of
                                zstd_tree_cases.tree_records, or "fixture" and its number),
                                plain_len, plain_sha256, rec_off, rec_len

The plain bytes are not stored: tests/zstd_tree_cases.py regenerates them and the manifest holds
their hashes. tests/test_gpu_zstd_compress_trees.py asserts that the compressor still produces
exactly these bytes; tests/test_zstd_gpu_trees_golden_cpu.py decodes every committed frame with
libzstd and tests/zstd_model.py without a GPU. ANY later change to the encoder changes the bytes:
regenerate with this script and commit the files with the change.

Usage: python tests/golden/make_zstd_gpu_trees.py [--out DIR]   (DIR defaults to tests/golden)
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import zstd_enc_cases as zc  # noqa: E402
import zstd_tree_cases as tc  # noqa: E402


def picks(ents):
    """[(name, dict, source, fixture number or None)]"""
    def first(pred):
        return [k for k, e in enumerate(ents) if pred(e)][0]
    out = [(n, False, n, None) for n in ("low64", "skewed", "tiny8", "lits1023", "lits1024",
                                          "two_blocks_reuse", "two_blocks_new_tree")]
    out += [("huf1:dict", True, "huf1", None), ("two_blocks_reuse:dict", True, "two_blocks_reuse",
                                                None)]
    # an indexed dictionary batch large enough for its own tree, and a small one that keeps the
    # dictionary's
    out.append(("fixture_tree", True, "fixture",
                first(lambda e: e["dict"] and e["indexed"] and 6000 < e["plain_len"] < 7000)))
    out.append(("fixture_treeless", True, "fixture",
                first(lambda e: e["dict"] and e["indexed"] and 500 < e["plain_len"] < 1000)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    import netidx_amd
    ents, rec, plain, d = zc.load_fixtures()
    crafted = tc.tree_records(d)
    codec = netidx_amd.Codec(0)
    zd = codec.zstd_dict(d)
    blob, man = b"", []
    for name, use_dict, source, k in picks(ents):
        idx, b = zc.fixture_record(ents[k], rec, plain) if source == "fixture" else (b"", crafted[source])
        indexed = bool(ents[k]["indexed"]) if source == "fixture" else False
        src = np.frombuffer(idx + b + b"\0", np.uint8)
        out, res = codec.archive_compress(src, [(0, len(idx) + len(b))], indexed,
                                          zd if use_dict else None, tc.BLOCK_TREES)
        oo, ol, er = res[0]
        assert er == 0, name
        cr = bytes(out[oo:oo + ol])
        e = {"name": name, "dict": use_dict, "indexed": indexed, "index": idx.hex(),
             "source": source, "plain_len": len(b), "plain_sha256": hashlib.sha256(b).hexdigest(),
             "rec_off": len(blob), "rec_len": len(cr)}
        if source == "fixture":
            e["fixture"] = k
        man.append(e)
        blob += cr
        print(name, len(b), "->", len(cr))
    zd.close()
    codec.close()
    assert len(blob) < os.path.getsize(os.path.join(HERE, "zstd_gpu_records.bin"))
    os.makedirs(a.out, exist_ok=True)
    open(os.path.join(a.out, "zstd_gpu_tree_records.bin"), "wb").write(blob)
    json.dump({"records": man}, open(os.path.join(a.out, "zstd_gpu_tree_manifest.json"), "w"),
              indent=1)


if __name__ == "__main__":
    main()
