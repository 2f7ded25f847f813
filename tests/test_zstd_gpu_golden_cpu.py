"""The GPU zstd compressor's golden pin (tests/golden/zstd_gpu_records.bin, written on the MI355X by
tests/golden/make_zstd_gpu.py) checked on the CPU: libzstd decompresses every committed frame to
its recorded plain bytes, and the records' layout and frame headers are what compress_task writes.
tests/test_gpu_zstd_compress.py asserts the GPU still produces exactly these bytes, so what the
GPU produces is what libzstd here reads. Skips only where libzstd is absent."""
import json
import os

import pytest

import zstd_enc_cases as zc

G = zc.G


def load():
    ents, rec, plain, d = zc.load_fixtures()
    m = json.load(open(os.path.join(G, "zstd_gpu_manifest.json")))["records"]
    blob = open(os.path.join(G, "zstd_gpu_records.bin"), "rb").read()
    own = open(os.path.join(G, "zstd_gpu_plain.bin"), "rb").read()
    out = []
    for e in m:
        src = plain if e["plain_src"] == "fixture" else own
        out.append((e, blob[e["rec_off"]:e["rec_off"] + e["rec_len"]],
                    src[e["plain_off"]:e["plain_off"] + e["plain_len"]]))
    return out, d, len(blob) + len(own)


def test_the_pin_covers_what_it_must():
    recs, d, size = load()
    assert size <= 512 * 1024
    by = {e["name"]: (e, cr, b) for e, cr, b in recs}
    assert len(by["empty"][2]) == 0 and 0 < len(by["tiny"][2]) < 16
    assert by["indexed"][0]["indexed"] and by["indexed"][0]["index"]
    assert len(zc.blocks(by["two_blocks"][1][4:])) == 2
    assert not by["no_dict"][0]["dict"]
    crafted = zc.crafted(d)
    for name in ("huf1", "huf4", "dict_slice", "pattern64", "one_byte"):
        assert by[name][2] == crafted[name]


def test_layout_and_frame_headers():
    recs, d, _ = load()
    did = zc.dict_parts(d)[0]
    for e, cr, b in recs:
        idx = bytes.fromhex(e["index"])
        assert int.from_bytes(cr[:4], "big") == len(idx) + len(b), e["name"]
        assert cr[4:4 + len(idx)] == idx
        assert len(cr) <= zc.worst_case(len(idx), len(b))
        zc.check_frame_header(cr[4 + len(idx):], len(b), did if e["dict"] else 0)
        zc.blocks(cr[4 + len(idx):])  # the blocks end where the frame ends


def test_libzstd_decompresses_every_committed_frame():
    z = zc.Libzstd.load()
    if z is None:
        pytest.skip("libzstd.so.1 does not load here")
    recs, d, _ = load()
    for e, cr, b in recs:
        f = cr[4 + len(e["index"]) // 2:]
        assert z.decompress(f, len(b), d if e["dict"] else None) == b, e["name"]
